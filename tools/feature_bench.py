#!/usr/bin/env python3
"""Device time of the feature planes (zrt_context_features) on a config's
frame (--config cfg3, cfg2: scene, camera, size and sample count), in two
comparisons:

  frame    the feature call with device pointers (zrt_stats.trace_kernel_ms:
           the frustum bounds, the walk and the resolve of every pass) beside
           the exclusive time of the primary launches of a render of the same
           frame (ZRT_FLAG_ONE_SET | ZRT_FLAG_KERNEL_TIMES, class "primary" of
           zrt_context_profile), which walk the same camera rays.  Per round
           the two calls alternate in this process; the medians are reported.
           The split of the call into its walk and resolve kernels is not
           visible to a caller: run this tool with --frame-only --rounds 1
           under a kernel trace (rocprofv3 --kernel-trace --stats) and read
           feature_walk_kernel, feature_resolve_kernel and wf_kernel there.
  compose  at a frame --compose-size (512) pixels high (and wide, unless the
           camera has an aspect ratio of its own) and --compose-spp (16) samples, the
           call against what a caller had to run before: w * h * spp host-made
           camera rays (numpy jitter: another stream than the library's, the
           same distribution) uploaded once, zrt_context_surface over them with
           device pointers, and the per-pixel sums as a torch reduction on the
           device.  Reported: the feature call; the surface call alone; the
           surface call plus the reduction (device events around both); and
           the bytes the composition moves over the bus each frame (24 B per
           ray up) against the 100-byte camera.

A time is measured on the GPU or not at all.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libzrt then binds to torch's HIP runtime, as in bench.py)

from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402

WIDTH = dict(native.FEATURE_PLANES)


def device_planes(n, dev):
    return {k: torch.empty((n * WIDTH[k],), dtype=torch.int32 if k == "hits" else torch.float32, device=dev)
            for k in WIDTH}


def pixel_major_rays(cam, spp, seed):
    """(w * h * spp, 6) float32: `spp` jittered rays per pixel, a pixel's
    consecutive, pixels in tile_pixels order (Camera.getRay, stage3.zig:27-35)."""
    pix = np.repeat(native.tile_pixels(cam.w, cam.h), spp)
    rng = np.random.default_rng(seed)
    x = (pix % cam.w).astype(np.float32) + rng.random(pix.size, dtype=np.float32)
    y = (pix // cam.w).astype(np.float32) + rng.random(pix.size, dtype=np.float32)
    llc, right, up = (np.array(list(v), np.float32) for v in (cam.lower_left_corner, cam.right, cam.up))
    d = llc + x[:, None] * right + y[:, None] * up
    d /= np.sqrt((d * d).sum(1))[:, None]
    o = np.tile(np.array(list(cam.origin), np.float32), (pix.size, 1))
    return np.ascontiguousarray(np.concatenate([o, d.astype(np.float32)], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", choices=sorted(scenes.CONFIGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3, help="calls of each variant per round")
    ap.add_argument("--spp", type=int, default=0, help="samples of the frame (0: the config's)")
    ap.add_argument("--compose-size", type=int, default=512)
    ap.add_argument("--compose-spp", type=int, default=16)
    ap.add_argument("--frame-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("feature_bench: no HIP device (a time is measured on the GPU or not at all)")
    out = a.out or os.path.join(ROOT, "profiles", f"feature_bench_{a.config}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    log = open(os.path.splitext(out)[0] + ".log", "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    cfgd = dict(scenes.CONFIGS[a.config])
    soup = scenes.get_scene(cfgd["scene"])
    cam = camera_for(soup, cfgd["camera"], cfgd["width"], cfgd["height"])
    spp, mb = a.spp or cfgd["spp"], cfgd["max_bounce"]
    rs = RenderScene(soup, Config.load(os.path.join(ROOT, "config.json")).grid_resolution, device=0)
    ctx = rs.context
    dev = torch.device("cuda", 0)
    say(f"{a.config} scene ({cfgd['scene']}), {soup.num_triangles} triangles, frame {cam.w}x{cam.h} at {spp} spp "
        f"({cam.w * cam.h * spp / 1e6:.1f} M camera rays)")
    result = {"config": a.config, "scene": cfgd["scene"], "w": cam.w, "h": cam.h, "spp": spp, "rounds": a.rounds,
              "calls_per_round": a.calls}

    def fmt(v):
        return " / ".join(f"{x:.3f}" for x in v)

    # ---- the frame: the feature call beside the render's primary launches
    n = cam.w * cam.h
    planes = device_planes(n, dev)
    ptr = {k: v.data_ptr() for k, v in planes.items()}
    torch.cuda.synchronize()
    times = native.FLAG_ONE_SET | native.FLAG_KERNEL_TIMES

    def primary_ms():
        ctx.render(cam, spp, mb, flags=times)
        k = ctx.profile()["kernels"]["primary"]
        return k["ms"], k["launches"]

    def feature_call():
        return ctx.features_raw(cam, spp, ptr, True)

    primary_ms()                                               # warm-up: buffers grown, tables built
    feature_call()
    med = {"primary": [], "features": []}
    launches = {}
    for _ in range(a.rounds):
        ms = {k: [] for k in med}
        for _ in range(a.calls):
            t, launches["primary"] = primary_ms()
            ms["primary"].append(t)
            st = feature_call()
            launches["features"] = st["trace_launches"]
            ms["features"].append(st["trace_kernel_ms"])
        for k in med:
            med[k].append(float(np.median(ms[k])))
    hit = int(planes["hits"].sum(dtype=torch.int64).item())
    assert hit == st["hits"] and st["segments"] == n * spp
    result["frame"] = {"ms": med, "launches": launches, "hit_fraction": hit / (n * spp),
                       "features_over_primary": [f / p for f, p in zip(med["features"], med["primary"])]}
    say(f"frame    primary launches of a render {fmt(med['primary'])} ms ({launches['primary']} launches)  "
        f"feature call {fmt(med['features'])} ms ({launches['features']} launches)  "
        f"call / primary {fmt(result['frame']['features_over_primary'])}  hit fraction {hit / (n * spp):.3f}")
    del planes

    # ---- the composition a caller ran before
    if not a.frame_only:
        cs, cspp = a.compose_size, a.compose_spp
        # (a camera with an aspect ratio of its own takes the height alone, as the config's frame does)
        ccam = camera_for(soup, cfgd["camera"], None if cfgd["width"] is None else cs, cs)
        cw = ccam.w
        n = cw * cs
        planes = device_planes(n, dev)
        ptr = {k: v.data_ptr() for k, v in planes.items()}
        host_rays = pixel_major_rays(ccam, cspp, 1)
        rays = torch.from_numpy(host_rays).to(dev)
        surf = torch.empty((n * cspp, 16), dtype=torch.float32, device=dev)
        hits = torch.empty((n * cspp, 4), dtype=torch.float32, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()

        def surface_call():
            return ctx.surface_raw(n * cspp, rays.data_ptr(), surf.data_ptr(), hits.data_ptr(), True)["trace_kernel_ms"]

        def composed():
            ev[0].record()
            surface_call()
            rec = surf.view(n, cspp, 16)
            hit = (rec[:, :, 3].view(torch.int32) != -1)
            w = hit.to(torch.float32).unsqueeze(-1)
            sums = [(rec[:, :, 8:11] * w).sum(1), (rec[:, :, 4:7] * w).sum(1), (rec[:, :, 12:15] * w).sum(1),
                    (hits.view(n, cspp, 4)[:, :, 0].nan_to_num(posinf=0.0) * w[..., 0]).sum(1),
                    (rec[:, :, 7] * w[..., 0]).sum(1), hit.sum(1)]
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]), sums

        def features():
            return ctx.features_raw(ccam, cspp, ptr, True)["trace_kernel_ms"]

        for f in (surface_call, composed, features) * 2:        # warm-up
            f()
        med = {"features": [], "surface": [], "composed": []}
        for _ in range(a.rounds):
            ms = {k: [] for k in med}
            for _ in range(max(a.calls, 5)):
                ms["features"].append(features())
                ms["surface"].append(surface_call())
                ms["composed"].append(composed()[0])
            for k in med:
                med[k].append(float(np.median(ms[k])))
        result["compose"] = {"w": cw, "h": cs, "spp": cspp, "rays": n * cspp, "ms": med,
                             "bus_bytes_per_frame": {"composition_rays_up": 24 * n * cspp, "features_camera": 100},
                             "surface_over_features": [s / f for s, f in zip(med["surface"], med["features"])],
                             "composed_over_features": [c / f for c, f in zip(med["composed"], med["features"])]}
        say(f"compose  {cw}x{cs} at {cspp} spp ({n * cspp / 1e6:.1f} M rays): feature call {fmt(med['features'])} ms  "
            f"surface call alone {fmt(med['surface'])} ms  surface + sums {fmt(med['composed'])} ms  "
            f"surface / features {fmt(result['compose']['surface_over_features'])}  "
            f"composed / features {fmt(result['compose']['composed_over_features'])}  "
            f"(the composition also uploads {24 * n * cspp / 1e6:.0f} MB of rays per frame)")

    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    log.close()
    rs.close()


if __name__ == "__main__":
    main()
