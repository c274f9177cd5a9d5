#!/usr/bin/env python3
"""Time of light-probe queries (zrt_context_light_probes) against the loop a
caller runs without them, in the same process, device batches (torch tensors):

  the call        Context.light_probes, the SH rows only: D directions per probe
                  made, traced, projected and summed on the device;
  the composed    torch.randn + normalise for the N x D directions (timed: the
                  caller has to draw them; the directions traced are the call's
                  own `directions` output, so that both sides trace the same
                  rays) -> the rays built from them -> Context.radiance with the
                  same keys -> the nine basis functions and the weighted sum per
                  probe with torch.  Its sum is torch's (a tree, a*b+c may be
                  contracted), so it agrees with the call's to rounding only;
                  the work is the same.

Two scenes: the cfg3 contest scene and the Cornell box, the probes drawn at 0.15
.. 0.85 of the scene's box.  max_bounce 4.

All are timed by the host clock around a synchronised call.  Per case: two
warm-up calls per variant, then `--rounds` rounds alternating the variants, the
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
from zig_raytracing_contest_amd import Config, RenderScene, scenes  # noqa: E402

MB = 4
SEED = 3
C0, C1, C2, C3, C4 = (float.fromhex(h) for h in ("0x1.20dd76p-2", "0x1.f45438p-2", "0x1.17b142p+0", "0x1.42f602p-2",
                                                 "0x1.17b142p-1"))
FOUR_PI = float.fromhex("0x1.921fb6p+3")


def box_probes(soup, n, seed):
    rng = np.random.default_rng(seed)
    p = np.asarray(soup.pos, np.float64).reshape(-1, 3)
    lo, ext = p.min(0), p.max(0) - p.min(0)
    return np.ascontiguousarray(lo + (0.15 + 0.7 * rng.random((n, 3))) * ext, np.float32)


def composed(ctx, pos, dirs, S):
    """What a caller writes today; sh (n, 9, 3) on the device.  dirs: (n, D, 3)."""
    n, D = dirs.shape[0], dirs.shape[1]
    g = torch.randn((n, D, 3), dtype=torch.float32, device=pos.device)
    g = g / torch.sqrt((g * g).sum(-1, keepdim=True))      # (drawn and dropped: see the docstring)
    o = pos[:, None, :].expand(n, D, 3).reshape(n * D, 3).contiguous()
    L = ctx.radiance(o, dirs.reshape(n * D, 3), S, MB, seed=SEED)["radiance"].reshape(n, D, 3)
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    Y = torch.stack([torch.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2 * x * y, C2 * y * z, C3 * (3.0 * z * z - 1.0),
                     C2 * x * z, C4 * (x * x - y * y)], dim=-1)               # (n, D, 9)
    return torch.einsum("ndk,ndc->nkc", Y, L) * (FOUR_PI / D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--directions", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--spp", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_probe_bench.json"))
    a = ap.parse_args()
    from zig_raytracing_contest_amd import native
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("light_probe_bench: no HIP device (a time is measured on the GPU or not at all)")
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

    out = {"rounds": a.rounds, "max_bounce": MB, "cases": []}
    cfgd = dict(scenes.CONFIGS["cfg3"])
    todo = (("cfg3", scenes.get_scene(cfgd["scene"]), Config.load(os.path.join(ROOT, "config.json")).grid_resolution),
            ("cornell", scenes.get_scene("cornell"), (16, 16, 16)))
    for sname, soup, res in todo:
        rs = RenderScene(soup, res, device=0)
        ctx = rs.context
        for n in a.probes:
            pos = torch.from_numpy(box_probes(soup, n, 50 + n)).to(dev)
            for D in a.directions:
                for S in a.spp:
                    r = ctx.light_probes(pos, D, S, MB, seed=SEED, directions=True, hits=True)
                    dirs, st = r["directions"], r["stats"]
                    sh_c = composed(ctx, pos, dirs, S)
                    err = float((r["sh"] - sh_c).abs().sum() / max(float(sh_c.abs().sum()), 1e-30))
                    assert err < 1e-4, err
                    variants = {"call": lambda: wall(lambda: ctx.light_probes(pos, D, S, MB, seed=SEED)),
                                "composed": lambda: wall(lambda: composed(ctx, pos, dirs, S))}
                    med = measure(variants, min(20, max(3, (1 << 22) // (n * D * S))))
                    row = {"scene": sname, "probes": n, "directions": D, "spp": S, "items": n * D,
                           "segments": st["segments"], "first_hits": st["hits"], "launches": st["trace_launches"],
                           "device_ms_once": st["trace_kernel_ms"], "mean_relative_difference": err,
                           "host_clock_ms": med,
                           "at_or_below_composed": all(x <= y for x, y in zip(med["call"], med["composed"]))}
                    out["cases"].append(row)
                    say(f"{sname:8s} {n:5d} probes x {D:4d} directions x {S} spp  " +
                        "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                        f" ms (host clock)  segments {st['segments']} first hits {st['hits']}"
                        f" launches {st['trace_launches']} at or below composed {row['at_or_below_composed']}")
        rs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    log.close()


if __name__ == "__main__":
    main()
