#!/usr/bin/env python3
"""Time of an adaptive film (zrt_context_refine) against the uniform film it
refines: one variant per process, so that a driver can alternate processes --
this tree's library and, through ZRT_LIB, another build's (the `accumulate`
variant needs nothing a build without zrt_context_refine lacks).  cfg3, the
contest stand-in at 1080p, max_bounce 4, the schedule 4, 4, 8, 16, 32, 64, 128
(256 samples), every call with the packed RGB8 of the frame so far on the host
(what a progressive caller shows), the last also with the row-major image:

  accumulate    Context.accumulate over the schedule;
  never         Context.refine with min_samples 65535: nothing is ever decided;
                per call the checkpoint launch (none in the first) and the
                present pass in place of the resolve's own output;
  decide        Context.refine with threshold -1: every call from the third on
                decides, scans, scatters and reads A back -- and freezes
                nothing, so the frame is still the uniform one;
  adaptive      Context.refine at --threshold: the count histogram, the samples
                traced, and the rate of the calls on a sparse list.

Host clock around synchronous calls; one warm-up frame, then --reps frames, each
printed.  The uniform variants' frame must be the oracle's
(tests/golden/frames.json); every variant prints its sha1.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zig_raytracing_contest_amd import camera_for, native, scenes  # noqa: E402

SCHEDULE = (4, 4, 8, 16, 32, 64, 128)
ap = argparse.ArgumentParser()
ap.add_argument("variant", choices=("accumulate", "never", "decide", "adaptive"))
ap.add_argument("--config", default="cfg3")
ap.add_argument("--threshold", type=float, default=0.125)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tag", default="this tree")
a = ap.parse_args()
if native.device_count() < 1:
    sys.exit("refine_bench: no HIP device (a time is measured on the GPU or not at all)")
cfg = scenes.CONFIGS[a.config]
soup = scenes.get_scene(cfg["scene"])
cam = camera_for(soup, cfg["camera"], cfg["width"], cfg["height"])
geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat)
keep = []
native.attach_materials(geo.scene, soup.tex_desc, soup.texels, keep)
ctx = native.Context(geo.scene)
mb = cfg["max_bounce"]
film = ctx.film(cam.w, cam.h)
img = np.zeros((cam.h, cam.w, 3), np.uint8)
with open(os.path.join(ROOT, "tests", "golden", "frames.json")) as fh:
    golden = json.load(fh).get(a.config)
uniform = a.variant != "adaptive"
assert not uniform or (golden and golden["spp"] == sum(SCHEDULE) and golden["max_bounce"] == mb)
thr, min_s = {"never": (0.125, 65535), "decide": (-1.0, 0), "adaptive": (a.threshold, 0)}.get(a.variant, (0.0, 0))


def frame():
    film.reset()
    calls = []
    for j, n in enumerate(SCHEDULE):
        last = j + 1 == len(SCHEDULE)
        t0 = time.perf_counter()
        if a.variant == "accumulate":
            r = ctx.accumulate(film, cam, n, mb, packed=True, image=img if last else None)
        else:
            r = ctx.refine(film, cam, n, mb, thr, min_s, packed=True, image=img if last else None, counts=last)
        r["ms"] = (time.perf_counter() - t0) * 1e3
        calls.append(r)
    return calls


frame()
P = film.n_owned
for _ in range(a.reps):
    t0 = time.perf_counter()
    calls = frame()
    ms = (time.perf_counter() - t0) * 1e3
    sha1 = hashlib.sha1(img.tobytes()).hexdigest()
    out = {"lib": a.tag, "variant": a.variant, "config": a.config, "frame_ms": round(ms, 3),
           "call_ms": [round(r["ms"], 2) for r in calls],
           "device_ms": [round(r["stats"]["render_ms"], 2) for r in calls],
           "call_mrays_s": [round(r["stats"]["segments"] / max(r["stats"]["render_ms"], 1e-9) / 1e3) for r in calls],
           "samples": sum(r["stats"]["samples"] for r in calls), "sha1": sha1[:12]}
    if uniform:
        assert sha1 == golden["rgb8_sha1"], (a.variant, sha1, golden["rgb8_sha1"])
        out["oracle_frame"] = True
    else:
        out["threshold"] = a.threshold
        out["active"] = [r["active"] for r in calls]
        out["of_uniform"] = round(out["samples"] / (P * sum(SCHEDULE)), 4)
        n, k = np.unique(calls[-1]["counts"], return_counts=True)
        out["counts"] = {int(x): int(y) for x, y in zip(n, k)}
        # the calls on a sparse list, and the same calls of a uniform film at the dense rate for comparison
        sparse = [r for r in calls if 0 < r["active"] < P]
        dense = [r for r in calls if r["active"] == P]
        rate = lambda rs: round(sum(r["stats"]["segments"] for r in rs) / max(sum(r["stats"]["render_ms"] for r in rs), 1e-9) / 1e3, 1)
        out["sparse_mrays_s"], out["dense_mrays_s"] = rate(sparse) if sparse else None, rate(dense) if dense else None
    print(json.dumps(out), flush=True)
film.close()
ctx.close()
