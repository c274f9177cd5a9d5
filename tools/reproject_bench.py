#!/usr/bin/env python3
"""Device time of the reprojection (zrt_context_reproject) as a stage of a
progressive preview under a moving camera, one process per run.  cfg3, the
contest stand-in at 1080p, max_bounce 4.  The camera's origin moves by a fixed
step along its `right` every frame, so that every frame reprojects across a
camera change.  A frame is four synchronous calls on one context:

  accumulate   4 samples into a reset film, no output;
  features     the same 4 camera samples, base colour, normal and depth into
               device buffers (torch tensors);
  reproject    film=..., the normal guide and the lengths, the history colour
               and length buffers updated in place, against the previous
               frame's depth and normal planes and camera;
  denoise      the history colour, the three planes as guides, 5 levels at the
               wrapper's default sigmas, RGB8 packed -- a device buffer, copied
               to the host inside the timed window.

Per call zrt_stats.render_ms (device events); the host clock around the four
calls and the copy.  One warm-up frame, then --reps frames, each printed.

The yardstick of the call is its traffic floor, computed here from the shapes:
what the two launches must read and write at least once per pixel -- the gather
reads the previous colour, depth, normal and length planes (12 + 4 + 12 + 4 B)
and a pixel index (4 B) and writes two 16-byte records; the reprojection reads
the film's sum (16 B), the depth and normal planes (4 + 12 B), a pixel index
(4 B) and each record once (32 B), and writes the colour and the length
(12 + 4 B) -- over the 8.0 TB/s HBM peak of the roofline (a copy
reaches about 6.3).  At 1080p the records and planes (about 250 MB with the
film) are of the size of the 256 MiB Infinity Cache, and each record is read by
up to four pixels' taps, mostly from L2: the ratio says how far the call is
from streaming its bytes once, not how busy the HBM was.
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step", type=float, default=0.002, help="the camera's move per frame, in lengths of its `right` times w")
a = ap.parse_args()
if native.device_count() < 1:
    sys.exit("reproject_bench: no HIP device (a time is measured on the GPU or not at all)")
cfg = scenes.CONFIGS[a.config]
soup = scenes.get_scene(cfg["scene"])
cam0 = camera_for(soup, cfg["camera"], cfg["width"], cfg["height"])
geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat)
keep = []
native.attach_materials(geo.scene, soup.tex_desc, soup.texels, keep)
ctx = native.Context(geo.scene)
mb = cfg["max_bounce"]
film = ctx.film(cam0.w, cam0.h)
P = film.n_owned
hist = native.History(ctx, cam0.w, cam0.h)
rgb = torch.zeros((P, 3), dtype=torch.uint8, device=hist.color.device)
torch.cuda.synchronize()
sig = native.DENOISE_SIGMAS

gather_bytes = P * (12 + 4 + 12 + 4 + 4 + 2 * 16)
reproject_bytes = P * (16 + 4 + 12 + 4 + 2 * 16 + 12 + 4)
floor_ms = (gather_bytes + reproject_bytes) / HBM_PEAK * 1e3


def camera(j):
    """cam0 with its origin moved j steps along `right`."""
    c = native.Camera.from_buffer_copy(cam0)
    for k in range(3):
        c.origin[k] = cam0.origin[k] + j * a.step * cam0.w * cam0.right[k]
    return c


def frame(j):
    cam = camera(j)
    film.reset()
    t0 = time.perf_counter()
    acc = ctx.accumulate(film, cam, a.spp, mb)["stats"]
    # History.update's two calls, apart, for their stats
    cur, prev = hist._guides
    feat = ctx.features_raw(cam, a.spp, {k: v.data_ptr() for k, v in cur.items()}, True)
    first = hist.camera is None
    rep = ctx.reproject_raw(cam, cam if first else hist.camera, None, film, cur["depth"].data_ptr(),
                            cur["normal"].data_ptr(), hist.color.data_ptr(),
                            (cur if first else prev)["depth"].data_ptr(), (cur if first else prev)["normal"].data_ptr(),
                            None if first else hist.length.data_ptr(), hist.color.data_ptr(), hist.length.data_ptr(),
                            None, True, 1 if first else hist.max_history, hist.depth_tolerance, hist.normal_tolerance)
    hist.camera, hist._guides = cam, [prev, cur]
    den = ctx.denoise_raw(cam.w, cam.h, hist.color.data_ptr(), None, cur["normal"].data_ptr(), cur["depth"].data_ptr(),
                          cur["base_color"].data_ptr(), None, rgb.data_ptr(), True, 5, *sig)
    host = rgb.cpu().numpy()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, acc, feat, rep, den, host


frame(0)
seen = {"accumulate": [], "features": [], "reproject": [], "denoise": []}
for j in range(1, a.reps + 1):
    ms, acc, feat, rep, den, host = frame(j)
    for k, st in zip(seen, (acc, feat, rep, den)):
        seen[k].append(st["render_ms"])
    lens = hist.length.cpu().numpy()
    out = {"config": a.config, "pixels": P, "spp": a.spp, "frame": j, "frame_ms_host_clock": round(ms, 3),
           "accumulate_device_ms": round(acc["render_ms"], 3), "features_device_ms": round(feat["render_ms"], 3),
           "reproject_device_ms": round(rep["render_ms"], 3), "denoise_device_ms": round(den["render_ms"], 3),
           "reproject_launches": rep["trace_launches"], "pixels_with_history": round(rep["hits"] / P, 4),
           "mean_length": round(float(lens.mean()), 3), "floor_ms_call": round(floor_ms, 4),
           "reproject_over_floor": round(rep["render_ms"] / floor_ms, 2),
           "rgb_sha1": hashlib.sha1(host.tobytes()).hexdigest()[:12]}
    print(json.dumps(out), flush=True)
print(json.dumps({"device_ms_min_median_max": {k: [round(float(f(v)), 3) for f in (np.min, np.median, np.max)]
                                                for k, v in seen.items()},
                  "reproject_median_over_floor": round(float(np.median(seen["reproject"])) / floor_ms, 2)}), flush=True)
film.close()
ctx.close()
