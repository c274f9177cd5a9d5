#!/usr/bin/env python3
"""Mrays/s of batch ray queries (zrt_context_trace) on the cfg3 contest scene:
lane walk against the park path, for batch sizes 2^10 .. 2^22, on

  camera      the cfg3 camera's own primary rays (jittered, seeded), in the
              render's packed pixel order, a pixel's samples side by side;
  incoherent  uniform points in the scene's bbox with uniform directions
              (fixed seed).

No bar to pass: the table says where the park path starts to win, which is
what kTraceParkMin (render.hip) rests on.  The yardstick printed beside it is
the render's own per-launch segment rate: the kernel durations of
profiles/r06/r06bl_kernel_stats_onestream_cfg3.csv (one cfg3 frame, one
stream) over that frame's segment counts, which a counting render gives here.

Per (set, size): two warm-up calls per mode (their hits compared bit for bit),
then `--rounds` rounds, each alternating lane and park calls and keeping the
median of each mode's device time (zrt_stats.trace_kernel_ms: events around
the chunk's kernels, the host copies left out).  A round times at least
2^24 rays or 5 calls per mode, at most 1000 calls.  Park "wins" a size when
its median is below the lane walk's in every round.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402

YARDSTICK = os.path.join(ROOT, "profiles", "r06", "r06bl_kernel_stats_onestream_cfg3.csv")


def camera_rays(cam, n, seed):
    """n primary rays of `cam` (Camera.getRay, stage3.zig:27-35), item = pixel * S + sample."""
    order = native.tile_pixels(cam.w, cam.h)
    S = max(1, -(-n // order.size))
    pix = order[np.arange(n) // S]
    rng = np.random.default_rng(seed)
    x = (pix % cam.w).astype(np.float32) + rng.random(n, dtype=np.float32)
    y = (pix // cam.w).astype(np.float32) + rng.random(n, dtype=np.float32)
    llc, right, up = (np.array(list(v), np.float32) for v in (cam.lower_left_corner, cam.right, cam.up))
    d = llc + x[:, None] * right + y[:, None] * up
    d /= np.sqrt((d * d).sum(1))[:, None]
    o = np.tile(np.array(list(cam.origin), np.float32), (n, 1))
    return np.ascontiguousarray(np.concatenate([o, d.astype(np.float32)], axis=1))


def incoherent_rays(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    o = lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(1))[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(np.float32))


def yardstick(rs, cam, cfgd):
    """Segments per second of the render's primary and park launches: the CSV's
    kernel durations over the segment counts of the same frame."""
    ns = {}
    with open(YARDSTICK) as f:
        for row in csv.DictReader(f):
            for key in ("wf_park_kernel", "wf_kernel<"):
                if key in row["Name"]:
                    ns[key] = ns.get(key, 0) + int(row["TotalDurationNs"])
    _, res = rs.render(cam, num_samples=cfgd["spp"], max_bounce=cfgd["max_bounce"], stats=True)
    total = res["stats"]["segments"]
    primary = rs.context.profile()["primary"]["segments"]
    return {"source": os.path.relpath(YARDSTICK, ROOT), "frame_segments": total, "primary_segments": primary,
            "primary_mrays_s": primary / ns["wf_kernel<"] * 1e3, "park_mrays_s": (total - primary) / ns["wf_park_kernel"] * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log2", type=int, default=10)
    ap.add_argument("--max-log2", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench_cfg3.json"))
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    if native.device_count() < 1:
        sys.exit("trace_bench: no HIP device (a rate is measured on the GPU or not at all)")
    cfgd = dict(scenes.CONFIGS["cfg3"])
    soup = scenes.get_scene(cfgd["scene"])
    cam = camera_for(soup, cfgd["camera"], cfgd["width"], cfgd["height"])
    rs = RenderScene(soup, Config.load(os.path.join(ROOT, "config.json")).grid_resolution, device=0)
    ctx = rs.context
    xyz = soup.pos.reshape(-1, 3)
    lo, hi = xyz.min(0).astype(np.float32), xyz.max(0).astype(np.float32)
    nmax = 1 << a.max_log2
    # (a batch of n camera rays is its own pixel-major list, made per size; the incoherent ones are a prefix)
    sets = {"camera": None, "incoherent": incoherent_rays(lo, hi, nmax, 2)}
    modes = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}      # both forced: no size threshold
    hits = {m: np.zeros(nmax, native.HIT_DTYPE) for m in modes}
    rows = []
    for sname, rays in sets.items():
        for lg in range(a.min_log2, a.max_log2 + 1):
            n = 1 << lg
            batch = camera_rays(cam, n, 1) if sname == "camera" else rays[:n]
            for m, f in modes.items():
                for _ in range(2):
                    st = ctx.trace_raw(n, batch.ctypes.data, hits[m].ctypes.data, False, f)
            same = bool(np.array_equal(hits["lane"][:n].view(np.uint32), hits["park"][:n].view(np.uint32)))
            calls = min(1000, max(5, (1 << 24) // n))
            med = {m: [] for m in modes}
            for _ in range(a.rounds):
                ms = {m: [] for m in modes}
                for _ in range(calls):
                    for m, f in modes.items():
                        st = ctx.trace_raw(n, batch.ctypes.data, hits[m].ctypes.data, False, f)
                        ms[m].append(st["trace_kernel_ms"])
                for m in modes:
                    med[m].append(float(np.median(ms[m])))
            row = {"set": sname, "rays": n, "calls_per_round": calls, "park_equals_lane": same,
                   "hit_fraction": float((hits["lane"]["triangle"][:n] != native.MISS).mean()),
                   "lane_ms": med["lane"], "park_ms": med["park"],
                   "lane_mrays_s": [n / t * 1e-3 for t in med["lane"]],
                   "park_mrays_s": [n / t * 1e-3 for t in med["park"]],
                   "park_wins": all(p < l for p, l in zip(med["park"], med["lane"]))}
            rows.append(row)
            print(f"{sname:10s} 2^{lg:<2d} lane {' / '.join(f'{x:8.1f}' for x in row['lane_mrays_s'])}  "
                  f"park {' / '.join(f'{x:8.1f}' for x in row['park_mrays_s'])} Mrays/s  "
                  f"{'park' if row['park_wins'] else 'lane'}  same={same}", flush=True)
    out = {"scene": "cfg3 contest stand-in, grid from config.json", "rounds": a.rounds, "rows": rows,
           "crossover": {s: next((r["rays"] for r in rows if r["set"] == s and r["park_wins"]), None) for s in sets}}
    if not a.no_yardstick:
        out["yardstick"] = yardstick(rs, cam, cfgd)
        print("render yardstick:", json.dumps(out["yardstick"]))
    print("crossover (smallest size at which park wins in every round):", out["crossover"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    rs.close()


if __name__ == "__main__":
    main()
