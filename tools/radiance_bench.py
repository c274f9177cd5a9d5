#!/usr/bin/env python3
"""Radiance queries (zrt_context_radiance) on the cfg3 contest scene: the
shared first segment (traced once per ray, fanned out into spp shaded
continuations) against ZRT_RADIANCE_PER_SAMPLE (traced once per sample).

2^16 probe rays -- origins uniform in the scene's bbox, uniform directions,
fixed seed -- at 16 and 64 spp, max_bounce 4.  Two flag sets: "default" (the
first segment's kernel by zrt_context_trace's size rule: the lane walk for
2^16 shared rays, the park kernel for the 2^20 .. 2^22 per-sample records) and
"park" (ZRT_TRACE_PARK: the park kernel in both modes).

No bar to pass: the segment count says the shared mode traces rays * (spp - 1)
fewer segments; this prints what the clock says.  Per (spp, flag set): one
warm-up call per mode, their results compared bit for bit (radiance, RGB8 and
the reported segments), then `--rounds` rounds, each alternating shared and
per-sample calls in this one process and keeping the median of each mode's
device time (zrt_stats.trace_kernel_ms: events around the chunk's kernels, the
host copies left out).  "shared_wins": its median is below the other's in
every round.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zig_raytracing_contest_amd import Config, RenderScene, native, scenes  # noqa: E402


def probe_rays(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    o = lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(1))[:, None]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rays", type=int, default=16)
    ap.add_argument("--spp", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--max-bounce", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10, help="calls per mode and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_bench_cfg3.json"))
    a = ap.parse_args()
    if native.device_count() < 1:
        sys.exit("radiance_bench: no HIP device (a rate is measured on the GPU or not at all)")
    cfgd = dict(scenes.CONFIGS["cfg3"])
    soup = scenes.get_scene(cfgd["scene"])
    rs = RenderScene(soup, Config.load(os.path.join(ROOT, "config.json")).grid_resolution, device=0)
    xyz = soup.pos.reshape(-1, 3)
    n = 1 << a.log2_rays
    o, d = probe_rays(xyz.min(0).astype(np.float32), xyz.max(0).astype(np.float32), n, 2)
    modes = {"shared": 0, "per_sample": native.RADIANCE_PER_SAMPLE}
    rows = []
    for spp in a.spp:
        for fname, extra in (("default", 0), ("park", native.TRACE_PARK)):
            warm = {m: rs.radiance(o, d, spp, a.max_bounce, seed=1, flags=f | extra, rgb=True) for m, f in modes.items()}
            same = bool(np.array_equal(warm["shared"]["radiance"].view(np.uint32),
                                       warm["per_sample"]["radiance"].view(np.uint32)) and
                        np.array_equal(warm["shared"]["rgb"], warm["per_sample"]["rgb"]) and
                        warm["shared"]["stats"]["segments"] == warm["per_sample"]["stats"]["segments"])
            if not same:
                sys.exit(f"radiance_bench: spp {spp} {fname}: the two modes differ; nothing timed")
            med = {m: [] for m in modes}
            for _ in range(a.rounds):
                ms = {m: [] for m in modes}
                for _ in range(a.calls):
                    for m, f in modes.items():
                        ms[m].append(rs.radiance(o, d, spp, a.max_bounce, seed=1, flags=f | extra)["stats"]["trace_kernel_ms"])
                for m in modes:
                    med[m].append(float(np.median(ms[m])))
            segments = warm["shared"]["stats"]["segments"]
            row = {"spp": spp, "flags": fname, "rays": n, "paths": n * spp, "max_bounce": a.max_bounce,
                   "segments": segments, "segments_traced_shared": segments - n * (spp - 1),
                   "results_identical": same, "calls_per_round": a.calls,
                   "launches": {m: warm[m]["stats"]["trace_launches"] for m in modes},
                   "shared_ms": med["shared"], "per_sample_ms": med["per_sample"],
                   "shared_mpaths_s": [n * spp / t * 1e-3 for t in med["shared"]],
                   "per_sample_mpaths_s": [n * spp / t * 1e-3 for t in med["per_sample"]],
                   "shared_wins": all(s < p for s, p in zip(med["shared"], med["per_sample"]))}
            rows.append(row)
            print(f"spp {spp:3d} {fname:8s} segments {segments} (shared traces {row['segments_traced_shared']})  "
                  f"shared {' / '.join(f'{x:7.3f}' for x in med['shared'])} ms "
                  f"({' / '.join(f'{x:7.1f}' for x in row['shared_mpaths_s'])} Mpaths/s)  "
                  f"per-sample {' / '.join(f'{x:7.3f}' for x in med['per_sample'])} ms "
                  f"({' / '.join(f'{x:7.1f}' for x in row['per_sample_mpaths_s'])} Mpaths/s)  "
                  f"{'shared' if row['shared_wins'] else 'not shared'}  same={same}", flush=True)
    out = {"scene": "cfg3 contest stand-in, grid from config.json", "rays": "uniform origins in the bbox, uniform directions",
           "rounds": a.rounds, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    rs.close()


if __name__ == "__main__":
    main()
