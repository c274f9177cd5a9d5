#!/usr/bin/env python3
"""Time and error of sky-light queries (zrt_context_sky_light), device batches
(torch tensors), in one process:

  the call        Context.sky_light, S samples per ray, 16 crossings at most;
  unshadowed      the same call with ZRT_SKY_UNSHADOWED (no chain is walked);
  the composed    Context.surface -> per (ray, sample) the direction
                  normalize(N + normalize(torch.randn(3))) and the sky's colour,
                  all with torch on the device -> the traced items' rays
                  gathered -> Context.transmittance over them -> the samples
                  summed per ray with torch.  Its draws are torch's, so its sums
                  are another estimate of the same integral.

Two scenes, each through a camera 512 pixels high: the cfg3 contest scene and
the Cornell box (cfg2).  Sizes are ITEMS (rays x samples): 2^lg / S rays per
call.  Times are the host clock around a synchronised call (two warm-up calls
per variant, then `--rounds` rounds alternating all variants, the median of
each round kept) and the call's own device time once (zrt_stats.render_ms).

Then the park question: Context.transmittance over 2^20 of the call's own
hemisphere rays (unbounded, incoherent) on cfg3 with the lane chains and with
ZRT_TRACE_PARK, alternating.

Then, on cfg2, the mean absolute error of area_lights.radiance +
sky_light.radiance - emissive against a 4096-sample
Context.radiance(max_bounce = 2) run over 16,384 camera rays at S = 4, 16 and
64, beside the area-light call's alone (DESIGN 5.25's numbers).
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

H = 512
CAP = 16


def unit(v):
    return v / torch.sqrt((v * v).sum(-1, keepdim=True))


def hemisphere(ctx, o, d, S):
    """(pos (n, 3), D (n, S, 3), traced (n, S), the surfaces) with torch's draws."""
    surf = ctx.surface(o, d)["surfaces"]
    hit = surf[:, 3].view(torch.int32) != -1
    pos, N = surf[:, 0:3], unit(surf[:, 4:7])
    shaded = hit & torch.isfinite(pos).all(1) & torch.isfinite(N).all(1)
    D = unit(N[:, None, :] + unit(torch.randn((o.shape[0], S, 3), device=o.device)))
    TR = shaded[:, None] & torch.isfinite(D).all(2) & (D != 0).any(2)
    return pos, D, TR, surf


def composed(ctx, o, d, S):
    """What a caller writes without the call; (radiance (n, 3), visibility (n,), traced items) on the device."""
    n = o.shape[0]
    pos, D, TR, surf = hemisphere(ctx, o, d, S)
    t = 0.5 * (D[..., 1] + 1.0)
    L = (1.0 - t)[..., None] + torch.tensor([0.5, 0.7, 1.0], device=o.device) * t[..., None]
    T = torch.zeros((n, S), dtype=torch.float32, device=o.device)
    po = pos[:, None, :].expand(n, S, 3)[TR].contiguous()
    if po.shape[0]:
        T[TR] = ctx.transmittance(po, D[TR].contiguous(), max_crossings=CAP)["transmittance"]
    mean = (L * T[..., None]).sum(1) / S
    return surf[:, 12:15] + surf[:, 8:11] * mean, T.sum(1) / S, int(po.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 18, 20], help="items (rays x samples) per call")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_light_bench.json"))
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("sky_light_bench: no HIP device (a time is measured on the GPU or not at all)")
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

    out = {"rounds": a.rounds, "max_crossings": CAP, "cases": [], "park": [], "error": []}
    cfgd = dict(scenes.CONFIGS["cfg3"])
    todo = (("cfg3", scenes.get_scene(cfgd["scene"]), cfgd["camera"],
             Config.load(os.path.join(ROOT, "config.json")).grid_resolution),
            ("cfg2", scenes.get_scene("cornell"), None, (16, 16, 16)))
    for sname, soup, camera, res in todo:
        cam = camera_for(soup, camera, None if soup.camera(camera).aspect else H, H)
        rs = RenderScene(soup, res, device=0)
        ctx = rs.context
        for S in a.samples:
            for lg in a.log2:
                n = (1 << lg) // S
                rays = torch.from_numpy(camera_rays(cam, n, 1)).to(dev)
                o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
                res_c = ctx.sky_light(o, d, S, max_crossings=CAP)
                res_u = ctx.sky_light(o, d, S, max_crossings=CAP, unshadowed=True)
                R_c, V_c, traced = composed(ctx, o, d, S)
                st = res_c["stats"]
                variants = {"call": lambda: wall(lambda: ctx.sky_light(o, d, S, max_crossings=CAP)),
                            "unshadowed": lambda: wall(lambda: ctx.sky_light(o, d, S, max_crossings=CAP, unshadowed=True)),
                            "composed": lambda: wall(lambda: composed(ctx, o, d, S))}
                med = measure(variants, min(30, max(5, (1 << 22) >> lg)))
                ratio = [y / x for x, y in zip(med["call"], med["composed"])]
                row = {"scene": sname, "items": n * S, "rays": n, "samples": S, "traced_items": st["samples"],
                       "composed_traced_items": traced, "chain_segments": st["segments"] - n, "crossings": st["hits"],
                       "launches": st["trace_launches"], "device_ms_once": st["render_ms"],
                       "unshadowed_device_ms_once": res_u["stats"]["render_ms"],
                       "mean_visibility": float(res_c["visibility"].mean()), "composed_mean_visibility": float(V_c.mean()),
                       "mean_radiance": float(res_c["radiance"].mean()), "composed_mean_radiance": float(R_c.mean()),
                       "host_clock_ms": med, "composed_over_call": ratio,
                       "faster_than_composed": all(x > 1 for x in ratio)}
                out["cases"].append(row)
                say(f"{sname:5s} 2^{lg:<2d} items S {S:<2d} " +
                    "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                    f" ms (host clock)  composed / call {' / '.join(f'{x:.2f}' for x in ratio)}"
                    f"  device once {st['render_ms']:.4f} / unshadowed {res_u['stats']['render_ms']:.4f} ms"
                    f"  traced {st['samples']} (composed {traced}) chain segments {row['chain_segments']}"
                    f" crossings {st['hits']} launches {st['trace_launches']}"
                    f" mean visibility {row['mean_visibility']:.5f} (composed {row['composed_mean_visibility']:.5f})"
                    f" faster than composed {row['faster_than_composed']}")
        if sname == "cfg3":
            # the park question: 2^20 unbounded hemisphere rays as a transmittance call's, lane chains against park
            rays = torch.from_numpy(camera_rays(cam, 1 << 18, 1)).to(dev)
            pos, D, TR, _ = hemisphere(ctx, rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), 8)
            po, pd = pos[:, None, :].expand(-1, 8, 3)[TR].contiguous()[:1 << 20], D[TR].contiguous()[:1 << 20]
            lane = ctx.transmittance(po, pd, max_crossings=CAP)
            park = ctx.transmittance(po, pd, max_crossings=CAP, flags=native.TRACE_PARK)
            same = bool(torch.equal(lane["transmittance"], park["transmittance"]))
            med = measure({"lane": lambda: wall(lambda: ctx.transmittance(po, pd, max_crossings=CAP)),
                           "park": lambda: wall(lambda: ctx.transmittance(po, pd, max_crossings=CAP,
                                                                          flags=native.TRACE_PARK))}, 10)
            out["park"].append({"scene": sname, "rays": int(po.shape[0]), "host_clock_ms": med, "same_bits": same,
                                "lane_launches": lane["stats"]["trace_launches"],
                                "park_launches": park["stats"]["trace_launches"],
                                "segments": lane["stats"]["segments"], "crossings": lane["stats"]["hits"]})
            say(f"cfg3 transmittance over {po.shape[0]} hemisphere rays (t_max inf, cap {CAP}): " +
                "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                f" ms (host clock)  launches {lane['stats']['trace_launches']} / {park['stats']['trace_launches']}"
                f"  segments {lane['stats']['segments']} crossings {lane['stats']['hits']}  same bits {same}")
        if sname == "cfg2":
            n = 1 << 14
            em = rs.emitters()
            rays = torch.from_numpy(camera_rays(cam, n, 2)).to(dev)
            o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
            want = ctx.radiance(o, d, 4096, 2, seed=99)["radiance"]
            emis = ctx.surface(o, d)["surfaces"][:, 12:15]
            mae = lambda x: float((x - want).abs().mean())
            for S in (4, 16, 64):
                ar = ctx.area_lights(o, d, em, S, max_crossings=CAP, seed=5, irradiance=False, radiance=True)
                sk = ctx.sky_light(o, d, S, max_crossings=CAP, seed=6, irradiance=False, visibility=False)
                pt = ctx.radiance(o, d, S, 2, seed=5, stats=True)
                both = ar["radiance"] + sk["radiance"] - emis
                row = {"rays": n, "samples": S, "area_lights_ms": ar["stats"]["render_ms"],
                       "sky_light_ms": sk["stats"]["render_ms"], "radiance_ms": pt["stats"]["render_ms"],
                       "mae_area_lights": mae(ar["radiance"]), "mae_area_lights_plus_sky": mae(both),
                       "mae_radiance_equal_samples": mae(pt["radiance"]), "bias_area_lights_plus_sky": float((both - want).mean()),
                       "reference_mean": float(want.mean())}
                out["error"].append(row)
                say(f"cfg2 error, {n} rays, S {S}: area_lights {row['area_lights_ms']:.3f} ms MAE {row['mae_area_lights']:.6f};"
                    f" + sky_light {row['sky_light_ms']:.3f} ms MAE {row['mae_area_lights_plus_sky']:.6f}"
                    f" (mean difference {row['bias_area_lights_plus_sky']:+.6f});"
                    f" radiance(mb 2) S {S} {row['radiance_ms']:.3f} ms MAE {row['mae_radiance_equal_samples']:.6f}"
                    f" (4096-sample reference mean {row['reference_mean']:.5f})")
        rs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    log.close()


if __name__ == "__main__":
    main()
