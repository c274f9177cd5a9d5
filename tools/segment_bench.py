#!/usr/bin/env python3
"""Device time of segment queries (zrt_context_segments) on the cfg3 contest
scene against zrt_context_trace on the same rays in the same process -- the
yardstick: its kernels compile in none of the bound's code -- for 2^16, 2^20 and
2^22 rays, lane walk and park path, on

  control   trace_bench.py's incoherent set at t_max = +inf (the new call must
            cost what the old one does);
  ao_0.05   origins: the hit points of the cfg3 camera's rays (one
  ao_0.25   zrt_context_trace), moved 1e-4 bbox diagonals back along the ray;
            unit directions, cosine-distributed about the reversed ray;
            t_max = 0.05 and 0.25 diagonals;
  shadow    the same origins, unit directions towards one fixed point inside
            the bbox, t_max = the distance to it.

Per (set, size): two warm-up calls per variant with the results cross-checked
(park = lane bit for bit, any = closest's hit / miss, +inf = the unbounded
call), then `--rounds` rounds, each alternating all six variants (lane, park)
x (trace, closest, any) and keeping the median of each one's
zrt_stats.trace_kernel_ms.  A round times at least 2^24 rays or 5 calls per
variant, at most 1000.  At 2^20 rays one counting call per form gives the cells
visited and refs tested per ray.  The decisions DESIGN 5.13 takes from the
table are printed at the end: any_<path>_stays says whether an any-hit kernel of
that path would stay, were the "any" column its times (on the ao and shadow
sets from 2^20 rays, below bounded closest in every round); as the code
stands an any-hit call runs the closest kernels, so the column shows what the
byte and the count cost beside the records.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402
from trace_bench import incoherent_rays  # noqa: E402

INF = float("inf")
PATHS = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}      # both forced: no size threshold
FORMS = ("trace", "closest", "any")


def camera_rays(cam, n, seed):
    """n primary rays of `cam` (Camera.getRay, stage3.zig:27-35) over the WHOLE
    image at any n: ray i looks through packed pixel i * pixels / n, jittered
    (trace_bench.py's camera set takes the first n / S pixels, which are sky
    below 2^20 rays)."""
    order = native.tile_pixels(cam.w, cam.h)
    pix = order[(np.arange(n, dtype=np.int64) * order.size) // n]
    rng = np.random.default_rng(seed)
    x = (pix % cam.w).astype(np.float32) + rng.random(n, dtype=np.float32)
    y = (pix // cam.w).astype(np.float32) + rng.random(n, dtype=np.float32)
    llc, right, up = (np.array(list(v), np.float32) for v in (cam.lower_left_corner, cam.right, cam.up))
    d = llc + x[:, None] * right + y[:, None] * up
    d /= np.sqrt((d * d).sum(1))[:, None]
    o = np.tile(np.array(list(cam.origin), np.float32), (n, 1))
    return np.ascontiguousarray(np.concatenate([o, d.astype(np.float32)], axis=1))


def surface_points(ctx, cam, n, diag):
    """(origins, reversed unit ray directions) for n rays: the cfg3 camera's
    hit points, each moved 1e-4 diagonals against its ray; rays that miss take
    the points of the hitting ones in turn."""
    rays = camera_rays(cam, n, 1)
    hits = np.zeros(n, native.HIT_DTYPE)
    ctx.trace_raw(n, rays.ctypes.data, hits.ctypes.data, False, 0)
    ok = np.nonzero(hits["triangle"] != native.MISS)[0]
    assert ok.size, "the camera sees the scene"
    src = ok[np.arange(n) % ok.size]
    src[ok] = ok
    o, d, t = rays[src, :3], rays[src, 3:], hits["t"][src]
    p = o + (t - np.float32(1e-4) * diag)[:, None] * d
    return p.astype(np.float32), (-d).astype(np.float32), float(ok.size) / n


def cosine_dirs(w, seed):
    """Unit directions, cosine-distributed about the unit vectors w."""
    rng = np.random.default_rng(seed)
    n = len(w)
    u1, u2 = rng.random(n), rng.random(n)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(w[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    b1 = np.cross(w, a)
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = np.cross(w, b1)
    d = (r * np.cos(phi))[:, None] * b1 + (r * np.sin(phi))[:, None] * b2 + np.sqrt(1 - u1)[:, None] * w
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench_cfg3.json"))
    a = ap.parse_args()
    if native.device_count() < 1:
        sys.exit("segment_bench: no HIP device (a time is measured on the GPU or not at all)")
    log_path = os.path.splitext(a.out)[0] + ".log"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(log_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    cfgd = dict(scenes.CONFIGS["cfg3"])
    soup = scenes.get_scene(cfgd["scene"])
    cam = camera_for(soup, cfgd["camera"], cfgd["width"], cfgd["height"])
    rs = RenderScene(soup, Config.load(os.path.join(ROOT, "config.json")).grid_resolution, device=0)
    ctx = rs.context
    xyz = soup.pos.reshape(-1, 3)
    lo, hi = xyz.min(0).astype(np.float32), xyz.max(0).astype(np.float32)
    diag = np.float32(np.linalg.norm(hi - lo))
    light = (lo + np.array([0.5, 0.8, 0.5], np.float32) * (hi - lo)).astype(np.float32)
    say(f"cfg3 scene, bbox diagonal {float(diag):.6g}, shadow target {light.tolist()}")

    rows, counts = [], []
    for lg in a.log2:
        n = 1 << lg
        p, back, seen = surface_points(ctx, cam, n, diag)
        to_light = light - p
        dist = np.sqrt((to_light * to_light).sum(1, dtype=np.float32), dtype=np.float32)
        ao = np.ascontiguousarray(np.concatenate([p, cosine_dirs(back.astype(np.float64), 3)], axis=1))
        sets = {"control": (incoherent_rays(lo, hi, n, 2), INF, None),
                "ao_0.05": (ao, float(np.float32(0.05) * diag), None),
                "ao_0.25": (ao, float(np.float32(0.25) * diag), None),
                "shadow": (np.ascontiguousarray(np.concatenate([p, to_light / dist[:, None]], axis=1).astype(np.float32)),
                           INF, np.ascontiguousarray(dist))}
        hits = {k: np.zeros(n, native.HIT_DTYPE) for k in ("trace", "lane", "park")}
        occ = {k: np.zeros(n, np.uint8) for k in ("lane", "park")}
        for sname, (rays, t_all, t_each) in sets.items():
            tp = None if t_each is None else t_each.ctypes.data

            def call(path, form, flags=0):
                f = PATHS[path] | flags
                if form == "trace":
                    return ctx.trace_raw(n, rays.ctypes.data, hits["trace"].ctypes.data, False, f)
                if form == "closest":
                    return ctx.segments_raw(n, rays.ctypes.data, tp, hits[path].ctypes.data, None, False, f, t_all)
                return ctx.segments_raw(n, rays.ctypes.data, tp, None, occ[path].ctypes.data, False,
                                        f | native.SEGMENT_ANY, t_all)
            for path in PATHS:
                for form in FORMS:
                    for _ in range(2):
                        call(path, form)
            hit = hits["lane"]["triangle"] != native.MISS
            free_hit = hits["trace"]["triangle"] != native.MISS
            checks = {"park_equals_lane": bool(np.array_equal(hits["lane"].view(np.uint32), hits["park"].view(np.uint32))),
                      "any_equals_closest": bool(np.array_equal(occ["lane"] != 0, hit) and np.array_equal(occ["park"] != 0, hit))}
            if sname == "control":
                checks["inf_equals_trace"] = bool(np.array_equal(hits["lane"].view(np.uint32), hits["trace"].view(np.uint32)))
            assert all(checks.values()), (sname, n, checks)
            calls = min(1000, max(5, (1 << 24) // n))
            med = {(pa, fo): [] for pa in PATHS for fo in FORMS}
            for _ in range(a.rounds):
                ms = {k: [] for k in med}
                for _ in range(calls):
                    for k in med:
                        ms[k].append(call(*k)["trace_kernel_ms"])
                for k in med:
                    med[k].append(float(np.median(ms[k])))
            row = {"set": sname, "rays": n, "calls_per_round": calls, "camera_hit_fraction": seen,
                   "occluded_fraction": float(hit.mean()), "unbounded_hit_fraction": float(free_hit.mean()), **checks,
                   "ms": {f"{pa}_{fo}": med[(pa, fo)] for pa in PATHS for fo in FORMS}}
            rows.append(row)
            say(f"{sname:8s} 2^{lg:<2d} " + "  ".join(
                f"{pa} {fo} {' / '.join(f'{x:.4f}' for x in med[(pa, fo)])}" for pa in PATHS for fo in FORMS) +
                f" ms  occluded {row['occluded_fraction']:.3f} (unbounded {row['unbounded_hit_fraction']:.3f})")
            if lg == 20:
                c = {"set": sname, "rays": n}
                for form in FORMS:
                    st = call("lane", form, native.FLAG_COUNT_STATS)
                    c[form] = {"cells_per_ray": st["cells_visited"] / n, "tests_per_ray": st["triangle_tests"] / n,
                               "hits": st["hits"]}
                counts.append(c)
                say(f"{sname:8s} 2^20 per ray: " + "  ".join(
                    f"{fo} {c[fo]['cells_per_ray']:.2f} cells {c[fo]['tests_per_ray']:.2f} tests" for fo in FORMS))

    def ms(sname, n, key):
        return next(r["ms"][key] for r in rows if r["set"] == sname and r["rays"] == n)
    big = [1 << lg for lg in a.log2 if lg >= 20]
    bounded = ("ao_0.05", "ao_0.25", "shadow")
    decisions = {}
    for pa in PATHS:     # an any-hit kernel stays only if it beats bounded closest wherever it is asked to
        decisions[f"any_{pa}_stays"] = bool(big) and all(
            x < y for s in bounded for n in big for x, y in zip(ms(s, n, f"{pa}_any"), ms(s, n, f"{pa}_closest")))
    decisions["park_wins_bounded"] = {str(1 << lg): {s: all(x < y for x, y in zip(ms(s, 1 << lg, "park_closest"),
                                                                                   ms(s, 1 << lg, "lane_closest")))
                                                     for s in bounded} for lg in a.log2}
    ctl = {}
    for lg in a.log2:    # control: the new call against the old one, beside the old one's own spread between rounds
        for pa in PATHS:
            t, c = ms("control", 1 << lg, f"{pa}_trace"), ms("control", 1 << lg, f"{pa}_closest")
            ctl[f"{pa}_2^{lg}"] = {"trace_ms": t, "closest_ms": c, "trace_spread_ms": max(t) - min(t),
                                   "worst_difference_ms": max(abs(x - y) for x, y in zip(c, t))}
    decisions["control"] = ctl
    say("decisions: " + json.dumps(decisions))
    with open(a.out, "w") as f:
        json.dump({"scene": "cfg3 contest stand-in, grid from config.json", "rounds": a.rounds,
                   "bbox_diagonal": float(diag), "rows": rows, "counts_2^20": counts, "decisions": decisions}, f, indent=1)
    log.close()
    rs.close()


if __name__ == "__main__":
    main()
