#!/usr/bin/env python3
"""Time of occlusion queries (zrt_context_occlusion) against the loop a caller
runs without them, in the same process, device batches (torch tensors), lane
walk and park path both forced:

  the call      Context.occlusion, S samples per ray within a radius;
  the composed  Context.surface -> S directions per hit made with torch on the
                device (normalize(normal + normalize(randn))) -> the hit points
                repeated S times -> Context.segments any-hit over those items ->
                a torch reduction per ray.  Its directions are torch's, not the
                library's stream, so its counts agree with the call's in the
                mean only; the work is the same.

Two scenes, each through a camera 512 pixels high (910 x 512 at 16:9): the cfg3 contest scene (about 41%
of the first rays miss: their items are never made) and the Cornell box (every
ray hits).  Sizes are ITEMS (rays x samples): 2^lg / S rays per call.  Radii are
fractions of the scene's diagonal, and +inf.

`lane` and `park` force the path of the first hits and of the samples alike;
`samples_lane` / `samples_park` leave the first hits to zrt_context_trace's own
rule and set only the samples' path (ZRT_OCCLUSION_PARK_MIN), which is what the
library's unasked threshold decides; `unasked` is what a caller gets.

Both are timed by the host clock around a synchronised call.  Per case: two
warm-up calls per variant, then `--rounds` rounds alternating all variants, the
median of each round kept.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402
from segment_bench import camera_rays  # noqa: E402

PATHS = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}
H = 512


def composed(ctx, o, d, S, radius, flags, gen):
    """What a caller writes today; (occluded int32, visibility float32) torch tensors."""
    n = o.shape[0]
    surf = ctx.surface(o, d, flags=flags)["surfaces"]
    hit = surf[:, 3].view(torch.int32) != -1
    pos, nrm = surf[hit, 0:3], surf[hit, 4:7]
    nh = pos.shape[0]
    u = torch.randn((nh, S, 3), dtype=torch.float32, device=o.device, generator=gen)
    u = u / torch.sqrt((u * u).sum(-1, keepdim=True))
    ds = nrm[:, None, :] + u
    ds = (ds / torch.sqrt((ds * ds).sum(-1, keepdim=True))).reshape(-1, 3).contiguous()
    ps = pos[:, None, :].expand(nh, S, 3).reshape(-1, 3).contiguous()
    occ = torch.zeros(n, dtype=torch.int32, device=o.device)
    if nh:
        seg = ctx.segments(ps, ds, radius, any_hit=True, flags=flags)["occluded"]
        occ[hit] = seg.view(nh, S).sum(1, dtype=torch.int32)
    return occ, (S - occ).float() / float(S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20], help="items (rays x samples) per call")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--radii", type=float, nargs="+", default=[0.25, float("inf")], help="fractions of the diagonal")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_bench.json"))
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("occlusion_bench: no HIP device (a time is measured on the GPU or not at all)")
    dev = torch.device("cuda", 0)
    log_path = os.path.splitext(a.out)[0] + ".log"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(log_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def measure(variants, calls):
        for f in variants.values():
            f()
            f()
        med = {k: [] for k in variants}
        for _ in range(a.rounds):
            ms = {k: [] for k in variants}
            for _ in range(calls):
                for k, f in variants.items():
                    ms[k].append(f())
            for k in variants:
                med[k].append(float(np.median(ms[k])))
        return med

    def park_min(items, f):
        """f timed with the samples' unasked park threshold at `items`."""
        os.environ["ZRT_OCCLUSION_PARK_MIN"] = str(items)
        try:
            return wall(f)
        finally:
            os.environ.pop("ZRT_OCCLUSION_PARK_MIN", None)

    S = a.samples
    out = {"rounds": a.rounds, "samples": S, "cases": []}
    cfgd = dict(scenes.CONFIGS["cfg3"])
    todo = (("cfg3", scenes.get_scene(cfgd["scene"]), cfgd["camera"],
             Config.load(os.path.join(ROOT, "config.json")).grid_resolution),
            ("cornell", scenes.get_scene("cornell"), None, (16, 16, 16)))
    for sname, soup, camera, res in todo:
        cam = camera_for(soup, camera, None if soup.camera(camera).aspect else H, H)   # (910 x 512 at 16:9)
        rs = RenderScene(soup, res, device=0)
        ctx = rs.context
        xyz = soup.pos.reshape(-1, 3)
        diag = float(np.linalg.norm(xyz.max(0).astype(np.float64) - xyz.min(0)))
        for lg in a.log2:
            n = (1 << lg) // S
            rays = torch.from_numpy(camera_rays(cam, n, 1)).to(dev)
            o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
            for frac in a.radii:
                radius = frac * diag
                gen = torch.Generator(device=dev)
                gen.manual_seed(1)
                res_c = {p: ctx.occlusion(o, d, S, radius, flags=f) for p, f in PATHS.items()}
                assert torch.equal(res_c["lane"]["occluded"], res_c["park"]["occluded"]), "park = lane"
                occ_c, vis_c = composed(ctx, o, d, S, radius, 0, gen)
                st = res_c["lane"]["stats"]
                mean_call = float(res_c["lane"]["visibility"].mean())
                mean_comp = float(vis_c.mean())
                assert abs(mean_call - mean_comp) < 0.02, (mean_call, mean_comp)
                variants = {}
                for p, f in PATHS.items():
                    variants[f"{p}_call"] = lambda f=f: wall(lambda: ctx.occlusion(o, d, S, radius, flags=f))
                    variants[f"{p}_composed"] = lambda f=f: wall(lambda: composed(ctx, o, d, S, radius, f, gen))
                # the samples' path alone: the first hits by zrt_context_trace's own rule in both
                for p, lim in (("lane", 1 << 62), ("park", 0)):
                    variants[f"samples_{p}"] = lambda lim=lim: park_min(lim, lambda: ctx.occlusion(o, d, S, radius))
                variants["unasked_call"] = lambda: wall(lambda: ctx.occlusion(o, d, S, radius))
                variants["unasked_composed"] = lambda: wall(lambda: composed(ctx, o, d, S, radius, 0, gen))
                med = measure(variants, min(100, max(5, (1 << 23) >> lg)))
                row = {"scene": sname, "items": n * S, "rays": n, "radius_fraction": frac,
                       "traced_items": st["segments"] - n, "mean_visibility": mean_call,
                       "mean_visibility_composed": mean_comp,
                       "launches": {p: res_c[p]["stats"]["trace_launches"] for p in PATHS},
                       "device_ms_once": {p: res_c[p]["stats"]["trace_kernel_ms"] for p in PATHS}, "host_clock_ms": med}
                row["park_wins"] = all(x < y for x, y in zip(med["samples_park"], med["samples_lane"]))
                row["faster_than_composed"] = {p: all(x < y for x, y in zip(med[f"{p}_call"], med[f"{p}_composed"]))
                                               for p in list(PATHS) + ["unasked"]}
                out["cases"].append(row)
                say(f"{sname:8s} 2^{lg:<2d} items S {S} radius {frac:<5} " +
                    "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                    f" ms (host clock)  traced {row['traced_items']} visibility {mean_call:.3f} (composed {mean_comp:.3f})"
                    f" park wins {row['park_wins']} faster than composed {row['faster_than_composed']}")
        rs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    log.close()


if __name__ == "__main__":
    main()
