#!/usr/bin/env python3
"""Time of direct-light queries (zrt_context_direct) against the loop a caller
runs without them, in the same process, device batches (torch tensors):

  the call        Context.direct, L lights per ray, 16 crossings at most;
  unshadowed      the same call with ZRT_DIRECT_UNSHADOWED (no chain is walked);
  the composed    Context.surface -> per light w, b, f and the traced mask made
                  with torch on the device -> the traced items' rays gathered ->
                  Context.transmittance over them -> the lights summed per ray
                  in order with torch.  Its arithmetic is torch's (a*b+c may be
                  contracted there), so its sums agree with the call's to
                  rounding only; the work is the same.

Two scenes, each through a camera 512 pixels high (910 x 512 at 16:9): the cfg3
contest scene and the Cornell box.  Sizes are ITEMS (rays x lights): 2^lg / L
rays per call.  The lights are drawn inside the scene's box: points,
directionals and spots in turn.

All are timed by the host clock around a synchronised call.  Per case: two
warm-up calls per variant, then `--rounds` rounds alternating all variants, the
median of each round kept.
"""
import argparse
import json
import math
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


def box_lights(soup, L, seed):
    rng = np.random.default_rng(seed)
    p = np.asarray(soup.pos, np.float64).reshape(-1, 3)
    lo, ext = p.min(0), p.max(0) - p.min(0)
    out = []
    for l in range(L):
        at = lo + (0.1 + 0.8 * rng.random(3)) * ext
        aim = rng.normal(size=3)
        col = 0.25 + rng.random(3) * 4
        if l % 3 == 0:
            out.append(native.Light.point(at, col))
        elif l % 3 == 1:
            out.append(native.Light.directional(aim, col / 8))
        else:
            out.append(native.Light.spot(at, aim, col, math.radians(25), math.radians(60)))
    return out


def unit(v):
    return v / torch.sqrt((v * v).sum(-1, keepdim=True))


def composed(ctx, o, d, lights):
    """What a caller writes today; (irradiance (n, 3), traced items) on the device."""
    n, L = o.shape[0], len(lights)
    surf = ctx.surface(o, d)["surfaces"]
    hit = surf[:, 3].view(torch.int32) != -1
    pos, N = surf[:, 0:3], unit(surf[:, 4:7])
    shaded = hit & torch.isfinite(pos).all(1) & torch.isfinite(N).all(1)
    W = torch.empty((n, L, 3), dtype=torch.float32, device=o.device)
    B = torch.empty((n, L), dtype=torch.float32, device=o.device)
    Fm = torch.empty((n, L), dtype=torch.float32, device=o.device)
    TR = torch.empty((n, L), dtype=torch.bool, device=o.device)
    for l, lt in enumerate(lights):
        if lt.type == native.LIGHT_DIRECTIONAL:
            w = unit(-torch.tensor(list(lt.direction), dtype=torch.float32, device=o.device)).expand(n, 3)
            b = torch.full((n,), float("inf"), dtype=torch.float32, device=o.device)
            c = (N * w).sum(1)
            f = c
        else:
            v = torch.tensor(list(lt.position), dtype=torch.float32, device=o.device) - pos
            d2 = (v * v).sum(1)
            b = torch.sqrt(d2)
            w = v / b[:, None]
            c = (N * w).sum(1)
            f = c / d2
        tr = shaded & (c > 0)
        if lt.type == native.LIGHT_SPOT:
            s = -(unit(torch.tensor(list(lt.direction), dtype=torch.float32, device=o.device)) * w).sum(1)
            k = torch.clamp(torch.nan_to_num(s * lt.angle_scale + lt.angle_offset, nan=0.0), 0.0, 1.0)
            f = f * (k * k)
            tr = tr & (k > 0)
        W[:, l], B[:, l], Fm[:, l], TR[:, l] = w, b, f, tr
    T = torch.ones((n, L), dtype=torch.float32, device=o.device)
    po = pos[:, None, :].expand(n, L, 3)[TR].contiguous()
    if po.shape[0]:
        T[TR] = ctx.transmittance(po, W[TR].contiguous(), B[TR].contiguous(), max_crossings=CAP)["transmittance"]
    E = torch.zeros((n, 3), dtype=torch.float32, device=o.device)
    for l, lt in enumerate(lights):
        g = torch.where(TR[:, l], Fm[:, l] * T[:, l], torch.zeros((), dtype=torch.float32, device=o.device))
        E = E + torch.tensor(list(lt.color), dtype=torch.float32, device=o.device)[None, :] * g[:, None]
    return E, int(po.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 18, 20], help="items (rays x lights) per call")
    ap.add_argument("--lights", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct_bench.json"))
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("direct_bench: no HIP device (a time is measured on the GPU or not at all)")
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

    out = {"rounds": a.rounds, "max_crossings": CAP, "cases": []}
    cfgd = dict(scenes.CONFIGS["cfg3"])
    todo = (("cfg3", scenes.get_scene(cfgd["scene"]), cfgd["camera"],
             Config.load(os.path.join(ROOT, "config.json")).grid_resolution),
            ("cornell", scenes.get_scene("cornell"), None, (16, 16, 16)))
    for sname, soup, camera, res in todo:
        cam = camera_for(soup, camera, None if soup.camera(camera).aspect else H, H)   # (910 x 512 at 16:9)
        rs = RenderScene(soup, res, device=0)
        ctx = rs.context
        for L in a.lights:
            lights = box_lights(soup, L, 40 + L)
            for lg in a.log2:
                n = (1 << lg) // L
                rays = torch.from_numpy(camera_rays(cam, n, 1)).to(dev)
                o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
                res_c = ctx.direct(o, d, lights, max_crossings=CAP)
                E_c, traced = composed(ctx, o, d, lights)
                st = res_c["stats"]
                assert abs(st["samples"] - traced) <= max(8, traced // 1000), (st["samples"], traced)   # (torch rounds its own way)
                # (a chain that grazes an edge may end differently under torch's rounding of w: the mean decides)
                err = float((res_c["irradiance"] - E_c).abs().sum() / max(float(E_c.abs().sum()), 1e-30))
                assert err < 1e-3, err
                variants = {"call": lambda: wall(lambda: ctx.direct(o, d, lights, max_crossings=CAP)),
                            "unshadowed": lambda: wall(lambda: ctx.direct(o, d, lights, max_crossings=CAP, unshadowed=True)),
                            "composed": lambda: wall(lambda: composed(ctx, o, d, lights))}
                med = measure(variants, min(50, max(5, (1 << 22) >> lg)))
                row = {"scene": sname, "items": n * L, "rays": n, "lights": L, "traced_items": traced,
                       "chain_segments": st["segments"] - n, "crossings": st["hits"], "launches": st["trace_launches"],
                       "device_ms_once": st["trace_kernel_ms"], "mean_relative_difference": err, "host_clock_ms": med,
                       "faster_than_composed": all(x < y for x, y in zip(med["call"], med["composed"]))}
                out["cases"].append(row)
                say(f"{sname:8s} 2^{lg:<2d} items L {L:<2d} " +
                    "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                    f" ms (host clock)  traced {traced} chain segments {row['chain_segments']} crossings {st['hits']}"
                    f" launches {st['trace_launches']} faster than composed {row['faster_than_composed']}")
        rs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    log.close()


if __name__ == "__main__":
    main()
