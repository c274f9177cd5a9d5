#!/usr/bin/env python3
"""Time of a film (zrt_context_accumulate) against the render it continues: one
variant per process, so that a driver can alternate processes -- this tree's
library and, through ZRT_LIB, another build's (the `render` variant needs
nothing a build without films lacks).  cfg3, the contest stand-in at 1080p,
256 samples, max_bounce 4, every variant with the packed RGB8 of the frame on
the host at the end:

  render        one Context.render of 256 samples;
  one_shot      one Context.accumulate of 256 samples into an empty film: the
                same launches, the film's resolve in place of wf_resolve_kernel
                (16 B more stored per pixel);
  progressive   64 calls of 4 samples, each with its RGB8 preview: the price of
                being progressive -- per call the launch ramps and tails, the
                frustum bounds (a call of 4 samples is below their threshold),
                no second pass set, and the output copy;
  quiet         64 calls of 4 samples, only the last asking for an output.

Host clock around synchronous calls; one warm-up frame, then --reps frames, each
printed.  The frame's sha1 is printed too: every variant gives the same image.
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

ap = argparse.ArgumentParser()
ap.add_argument("variant", choices=("render", "one_shot", "progressive", "quiet"))
ap.add_argument("--config", default="cfg3")
ap.add_argument("--spp", type=int, default=256)
ap.add_argument("--calls", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tag", default="this tree")
a = ap.parse_args()
if native.device_count() < 1:
    sys.exit("film_bench: no HIP device (a time is measured on the GPU or not at all)")
cfg = scenes.CONFIGS[a.config]
soup = scenes.get_scene(cfg["scene"])
cam = camera_for(soup, cfg["camera"], cfg["width"], cfg["height"])
geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat)
keep = []
native.attach_materials(geo.scene, soup.tex_desc, soup.texels, keep)
ctx = native.Context(geo.scene)
mb = cfg["max_bounce"]
film = ctx.film(cam.w, cam.h) if a.variant != "render" else None
calls = 1 if a.variant in ("render", "one_shot") else a.calls
assert a.spp % calls == 0


def frame():
    if film is None:
        return ctx.render(cam, a.spp, mb, packed=True)
    film.reset()
    for j in range(calls):
        r = ctx.accumulate(film, cam, a.spp // calls, mb, packed=a.variant != "quiet" or j + 1 == calls)
    return r


frame()
for _ in range(a.reps):
    t0 = time.perf_counter()
    r = frame()
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"lib": a.tag, "variant": a.variant, "config": a.config, "spp": a.spp, "calls": calls,
                      "frame_ms": round(ms, 3), "last_call_device_ms": round(r["stats"]["render_ms"], 3),
                      "sha1": hashlib.sha1(np.ascontiguousarray(r["packed"]).tobytes()).hexdigest()[:12]}), flush=True)
if film is not None:
    film.close()
ctx.close()
