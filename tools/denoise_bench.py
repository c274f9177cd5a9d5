#!/usr/bin/env python3
"""Device time of the denoiser (zrt_context_denoise) as the last stage of a
progressive preview, one process per run so that a driver can alternate
processes -- this tree's library and, through ZRT_LIB, another build's (the
plain-gather build: denoise.hip compiled -DZRT_DN_TILED=0).  cfg3, the contest
stand-in at 1080p, max_bounce 4.  A frame is three synchronous calls on one
context:

  accumulate   4 samples into a reset film, no output;
  features     the same 4 camera samples, base colour, normal and depth into
               device buffers (torch tensors);
  denoise      film=..., the three planes as guides, `--iterations` levels at
               the wrapper's default sigmas, RGB8 packed -- a device buffer,
               copied to the host inside the timed window.

Per call zrt_stats.render_ms (device events); the host clock around the three
calls and the copy.  One warm-up frame, then --reps frames, each printed.

The yardstick of the filter is its traffic floor, computed here from the
shapes: what the launches must read and write at least once -- per level the
three 16-byte records of every pixel in and one out; the gather's planes in
(16 B sum, 12 + 4 + 12 B guides, 4 B pixel index) and three records out; the
present's record and index in and 3 B out -- over the 8.0 TB/s HBM peak of the
roofline (a copy reaches about 6.3).  The 25 taps of a level
mostly hit L2 and the Infinity Cache, and at 1080p all four record arrays
(133 MB) fit the 256 MiB Infinity Cache, so a level need not reach HBM at all:
the ratio says how far the filter is from streaming its records once, not how
busy the HBM was.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zig_raytracing_contest_amd import camera_for, native, scenes  # noqa: E402

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg3")
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--iterations", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tag", default="this tree", help="names the library in the output (ZRT_LIB: another build)")
a = ap.parse_args()
if native.device_count() < 1:
    sys.exit("denoise_bench: no HIP device (a time is measured on the GPU or not at all)")
cfg = scenes.CONFIGS[a.config]
soup = scenes.get_scene(cfg["scene"])
cam = camera_for(soup, cfg["camera"], cfg["width"], cfg["height"])
geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat)
keep = []
native.attach_materials(geo.scene, soup.tex_desc, soup.texels, keep)
ctx = native.Context(geo.scene)
mb = cfg["max_bounce"]
film = ctx.film(cam.w, cam.h)
P = film.n_owned
dev = torch.device("cuda", 0)
planes = {"base_color": torch.zeros((P, 3), dtype=torch.float32, device=dev),
          "normal": torch.zeros((P, 3), dtype=torch.float32, device=dev),
          "depth": torch.zeros((P,), dtype=torch.float32, device=dev)}
rgb = torch.zeros((P, 3), dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
sig = native.DENOISE_SIGMAS

level_bytes = P * (3 * 16 + 16)
gather_bytes = P * (16 + 12 + 4 + 12 + 4 + 3 * 16)
present_bytes = P * (16 + 4 + 3)
floor_ms = {"level": level_bytes / HBM_PEAK * 1e3,
            "call": (a.iterations * level_bytes + gather_bytes + present_bytes) / HBM_PEAK * 1e3}


def frame():
    film.reset()
    t0 = time.perf_counter()
    acc = ctx.accumulate(film, cam, a.spp, mb)["stats"]
    feat = ctx.features_raw(cam, a.spp, {k: v.data_ptr() for k, v in planes.items()}, True)
    den = ctx.denoise_raw(cam.w, cam.h, None, film, planes["normal"].data_ptr(), planes["depth"].data_ptr(),
                          planes["base_color"].data_ptr(), None, rgb.data_ptr(), True, a.iterations, *sig)
    host = rgb.cpu().numpy()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, acc, feat, den, host


frame()
for _ in range(a.reps):
    ms, acc, feat, den, host = frame()
    out = {"variant": a.tag, "config": a.config, "pixels": P, "spp": a.spp, "iterations": a.iterations,
           "frame_ms_host_clock": round(ms, 3),
           "accumulate_device_ms": round(acc["render_ms"], 3), "features_device_ms": round(feat["render_ms"], 3),
           "denoise_device_ms": round(den["render_ms"], 3), "denoise_launches": den["trace_launches"],
           "floor_ms_per_level": round(floor_ms["level"], 4), "floor_ms_call": round(floor_ms["call"], 4),
           "denoise_over_floor": round(den["render_ms"] / floor_ms["call"], 2),
           "rgb_sha1": hashlib.sha1(host.tobytes()).hexdigest()[:12]}
    print(json.dumps(out), flush=True)
film.close()
ctx.close()
