#!/usr/bin/env python3
"""Device time of the SVGF stages (zrt_context_illumination, the two
zrt_context_reproject calls, zrt_context_svgf) of a progressive preview under
a moving camera, one process per run.  cfg3, the contest stand-in at 1080p,
max_bounce 4.  The camera's origin moves by a fixed step along its `right`
every frame.  A frame is SvgfHistory.update's calls made one by one on one
context, for their stats, then the two filters over the same history:

  accumulate    4 samples into a reset film, no output;
  features      the same 4 camera samples, base colour, normal and depth into
                device buffers (torch tensors);
  illumination  film=..., the new base colour: illumination and moments;
  reproject     the illumination, then the moments, each in place against the
                previous frame's guides, camera and lengths; the lengths into
                the spare plane;
  svgf          5 levels at the wrapper's default sigmas, RGB8 packed;
  denoise       zrt_context_denoise, 5 levels, default sigmas, over the same
                illumination history and guides, RGB8 packed: the yardstick in
                the same process (three records per tap against two).

Per call zrt_stats.render_ms (device events).  One warm-up frame, then --reps
frames, each printed.

The svgf call's traffic floor, computed here from the shapes as DESIGN.md 5.22
does for the denoiser: what its launches must read and write at least once per
pixel -- the gather reads colour, moments, length, normal, depth and a pixel
index (12 + 12 + 4 + 12 + 4 + 4 B) and writes three 16-byte records; the
variance estimate reads the three records and writes 4 B; a level reads two
records and writes one; the present reads a record, a pixel index and the
albedo (16 + 4 + 12 B) and writes 3 B -- over the 8.0 TB/s HBM peak of the
roofline.  The records of a 1080p frame (100 MB) fit the
256 MiB Infinity Cache: the ratio says how far the call is from streaming its
bytes once, not how busy the HBM was.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zig_raytracing_contest_amd import camera_for, native, scenes  # noqa: E402

HBM_PEAK = 8.0e12
LEVELS = 5

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg3")
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step", type=float, default=0.002, help="the camera's move per frame, in lengths of its `right` times w")
a = ap.parse_args()
if native.device_count() < 1:
    sys.exit("svgf_bench: no HIP device (a time is measured on the GPU or not at all)")
cfg = scenes.CONFIGS[a.config]
soup = scenes.get_scene(cfg["scene"])
cam0 = camera_for(soup, cfg["camera"], cfg["width"], cfg["height"])
geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat)
keep = []
native.attach_materials(geo.scene, soup.tex_desc, soup.texels, keep)
ctx = native.Context(geo.scene)
mb = cfg["max_bounce"]
w, h = cam0.w, cam0.h
film = ctx.film(w, h)
P = film.n_owned
hist = native.SvgfHistory(ctx, w, h)
rgb = torch.zeros((P, 3), dtype=torch.uint8, device=hist.color.device)
rgb_dn = torch.zeros((P, 3), dtype=torch.uint8, device=hist.color.device)
torch.cuda.synchronize()

svgf_bytes = P * ((48 + 48) + (48 + 4) + LEVELS * 48 + (32 + 3))
floor_ms = svgf_bytes / HBM_PEAK * 1e3


def camera(j):
    """cam0 with its origin moved j steps along `right`."""
    c = native.Camera.from_buffer_copy(cam0)
    for k in range(3):
        c.origin[k] = cam0.origin[k] + j * a.step * cam0.w * cam0.right[k]
    return c


def frame(j):
    cam = camera(j)
    film.reset()
    st = {"accumulate": ctx.accumulate(film, cam, a.spp, mb)["stats"]}
    # SvgfHistory.update's calls, apart, for their stats
    cur, prev = hist._guides
    st["features"] = ctx.features_raw(cam, a.spp, {k: v.data_ptr() for k, v in cur.items()}, True)
    illum, mom = hist._frame
    st["illumination"] = ctx.illumination_raw(w, h, None, film, cur["base_color"].data_ptr(), illum.data_ptr(),
                                              mom.data_ptr(), True)
    first = hist.camera is None
    old = cur if first else prev
    for name, now, past in (("reproject_illumination", illum, hist.color), ("reproject_moments", mom, hist.moments)):
        st[name] = ctx.reproject_raw(cam, cam if first else hist.camera, now.data_ptr(), None, cur["depth"].data_ptr(),
                                     cur["normal"].data_ptr(), past.data_ptr(), old["depth"].data_ptr(),
                                     old["normal"].data_ptr(), None if first else hist.length.data_ptr(),
                                     past.data_ptr(), hist._length_next.data_ptr(), None, True,
                                     1 if first else hist.max_history, hist.depth_tolerance, hist.normal_tolerance)
    hist.length, hist._length_next = hist._length_next, hist.length
    hist.camera, hist._guides = cam, [prev, cur]
    st["svgf"] = ctx.svgf_raw(w, h, hist.color.data_ptr(), hist.moments.data_ptr(), hist.length.data_ptr(),
                              cur["normal"].data_ptr(), cur["depth"].data_ptr(), cur["base_color"].data_ptr(), None,
                              rgb.data_ptr(), None, True, LEVELS, *native.SVGF_SIGMAS)
    st["denoise"] = ctx.denoise_raw(w, h, hist.color.data_ptr(), None, cur["normal"].data_ptr(), cur["depth"].data_ptr(),
                                    cur["base_color"].data_ptr(), None, rgb_dn.data_ptr(), True, LEVELS,
                                    *native.DENOISE_SIGMAS)
    return st, rgb.cpu().numpy()


frame(0)
seen = {}
for j in range(1, a.reps + 1):
    st, host = frame(j)
    for k, s in st.items():
        seen.setdefault(k, []).append(s["render_ms"])
    out = {"config": a.config, "pixels": P, "spp": a.spp, "frame": j}
    out.update({k + "_device_ms": round(s["render_ms"], 3) for k, s in st.items()})
    out.update({"svgf_launches": st["svgf"]["trace_launches"], "temporal_variance_pixels": round(st["svgf"]["hits"] / P, 4),
                "pixels_with_history": round(st["reproject_moments"]["hits"] / P, 4),
                "mean_length": round(float(hist.length.cpu().numpy().mean()), 3),
                "svgf_floor_ms": round(floor_ms, 4), "svgf_over_floor": round(st["svgf"]["render_ms"] / floor_ms, 2),
                "svgf_over_denoise": round(st["svgf"]["render_ms"] / st["denoise"]["render_ms"], 3),
                "rgb_sha1": hashlib.sha1(host.tobytes()).hexdigest()[:12]})
    print(json.dumps(out), flush=True)
med = {k: float(np.median(v)) for k, v in seen.items()}
print(json.dumps({"device_ms_min_median_max": {k: [round(float(f(v)), 3) for f in (np.min, np.median, np.max)]
                                                for k, v in seen.items()},
                  "svgf_median_over_floor": round(med["svgf"] / floor_ms, 2),
                  "svgf_median_over_denoise_median": round(med["svgf"] / med["denoise"], 3)}), flush=True)
film.close()
ctx.close()
