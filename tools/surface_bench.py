#!/usr/bin/env python3
"""Device time of surface queries (zrt_context_surface) against
zrt_context_trace on the same rays in the same process -- the yardstick: its
kernels are untouched by the surface call -- for 2^16, 2^20 and 2^22 rays with
device pointers, on a config's scene (--config cfg3: real and 1x1 textures;
cfg5) and two ray sets of tools/segment_bench.py:

  camera   the config camera's jittered primary rays over the whole image;
  ao       origins: those rays' hit points moved 1e-4 bbox diagonals back
           along the ray; unit directions, cosine-distributed about the
           reversed ray (incoherent).

Both calls take the park path (ZRT_TRACE_PARK) at every size.  Per (set,
size): two warm-up calls per variant with the results cross-checked (the
surface call's hit records are the trace call's, and a record is a miss
exactly where its hit record is), then `--rounds` rounds, each alternating the
two calls and the copy below and keeping the median of each call's
zrt_stats.trace_kernel_ms (the device time of the whole call for a
device batch).  A round times at least 2^24 rays or 5 calls per variant, at
most 1000.

The gather is the surface call minus the trace call.  Beside it: a
device-to-device copy (torch's copy_ of one contiguous buffer into another,
timed by device events in the same rounds) of HALF the bytes the gather has to
move, so that the copy's traffic, read plus write, is that byte count: per ray
the 16-byte hit record and the 24-byte ray in and the 64-byte record out, per
hit the 64-byte Data record and 16 B per channel of every texture of its
material larger than 1x1 (four texels; a 1x1 texel rides in the material
descriptor), counted from the call's own records.  The gather's time is
reported as a multiple of that copy's, and of those bytes over the HBM peak
(--hbm-tbs, 8.0 TB/s: MI355X's specification; about 6.3 TB/s is what a copy
reaches).  That second figure is a bound for the gather alone, not a share of
peak of the call.

(profiles/surface_bench_*_matpaths.* are from this tool while the library
still had a second gather that read the materials from an LDS copy, DESIGN
5.14: the same rounds with both gathers as variants.)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (first: libzrt then binds to torch's HIP runtime, as in bench.py)

from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402
from segment_bench import camera_rays, cosine_dirs, surface_points  # noqa: E402

PARK = native.TRACE_PARK


def gather_bytes(soup, surf_words):
    """(bytes the gather moves for these records, hits): see the module's docstring."""
    mat = surf_words[:, 3]
    hit = mat != native.MISS
    desc = np.asarray(soup.tex_desc).reshape(-1, 3, 7)
    big = desc[:, :, 1].astype(np.int64) * desc[:, :, 2] > 1                 # (nmat, 3)
    per_mat = (big * np.array([3, 3, 1]) * 16).sum(1)                         # four texels per channel
    n, h = len(mat), int(hit.sum())
    return int(n * (16 + 24 + 64) + h * 64 + per_mat[mat[hit]].sum()), h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", choices=sorted(scenes.CONFIGS))
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("surface_bench: no HIP device (a time is measured on the GPU or not at all)")
    out = a.out or os.path.join(ROOT, "profiles", f"surface_bench_{a.config}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    log = open(os.path.splitext(out)[0] + ".log", "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    cfgd = dict(scenes.CONFIGS[a.config])
    soup = scenes.get_scene(cfgd["scene"])
    cam = camera_for(soup, cfgd["camera"], cfgd["width"], cfgd["height"])
    rs = RenderScene(soup, Config.load(os.path.join(ROOT, "config.json")).grid_resolution, device=0)
    ctx = rs.context
    dev = torch.device("cuda", 0)
    xyz = soup.pos.reshape(-1, 3)
    diag = np.float32(np.linalg.norm(xyz.max(0).astype(np.float32) - xyz.min(0).astype(np.float32)))
    say(f"{a.config} scene ({cfgd['scene']}), {soup.num_triangles} triangles, {soup.num_materials} materials, "
        f"bbox diagonal {float(diag):.6g}, HBM peak taken as {a.hbm_tbs} TB/s")

    rows = []
    for lg in a.log2:
        n = 1 << lg
        p, back, seen = surface_points(ctx, cam, n, diag)
        sets = {"camera": camera_rays(cam, n, 1),
                "ao": np.ascontiguousarray(np.concatenate([p, cosine_dirs(back.astype(np.float64), 3)], axis=1))}
        for sname, host_rays in sets.items():
            rays = torch.from_numpy(host_rays).to(dev)
            hits_t = torch.empty((n, 4), dtype=torch.float32, device=dev)
            hits_s = torch.empty((n, 4), dtype=torch.float32, device=dev)
            surf = torch.empty((n, 16), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            variants = {"trace": lambda: ctx.trace_raw(n, rays.data_ptr(), hits_t.data_ptr(), True, PARK),
                        "surface": lambda: ctx.surface_raw(n, rays.data_ptr(), surf.data_ptr(), hits_s.data_ptr(), True,
                                                           PARK)}
            for f in variants.values():
                for _ in range(2):
                    f()
            words = surf.cpu().numpy().view(np.uint32)
            checks = {"hits_equal_trace": bool(torch.equal(hits_t.view(torch.int32), hits_s.view(torch.int32))),
                      "hit_iff_material": bool(np.array_equal(words[:, 3] != native.MISS,
                                                              hits_t[:, 3].view(torch.int32).cpu().numpy() != -1))}
            assert all(checks.values()), (sname, n, checks)
            nbytes, nhit = gather_bytes(soup, words)
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

            def copy_ms():
                ev[0].record()
                dst.copy_(src)
                ev[1].record()
                ev[1].synchronize()
                return ev[0].elapsed_time(ev[1])
            for _ in range(2):
                copy_ms()
            calls = min(1000, max(5, (1 << 24) // n))
            med = {k: [] for k in list(variants) + ["copy"]}
            for _ in range(a.rounds):
                ms = {k: [] for k in med}
                for _ in range(calls):
                    for k, f in variants.items():
                        ms[k].append(f()["trace_kernel_ms"])
                    ms["copy"].append(copy_ms())
                for k in med:
                    med[k].append(float(np.median(ms[k])))
            peak_ms = nbytes / (a.hbm_tbs * 1e12) * 1e3
            gather = [s - t for s, t in zip(med["surface"], med["trace"])]
            row = {"set": sname, "rays": n, "calls_per_round": calls, "hit_fraction": nhit / n, "gather_bytes": nbytes,
                   "copy_bytes": nbytes // 2, "bytes_over_hbm_peak_ms": peak_ms, **checks, "ms": med,
                   "gather_ms": gather, "gather_over_copy": [g / c for g, c in zip(gather, med["copy"])],
                   "gather_over_peak_bound": [g / peak_ms for g in gather]}
            rows.append(row)

            def fmt(v):
                return " / ".join(f"{x:.4f}" for x in v)
            say(f"{sname:6s} 2^{lg:<2d} hit {nhit / n:.3f}  trace {fmt(med['trace'])}  surface {fmt(med['surface'])}"
                f"  gather {fmt(gather)} ms  copy of {nbytes // 2} B {fmt(med['copy'])} ms"
                f"  gather / copy {fmt(row['gather_over_copy'])}  bytes / peak {peak_ms:.4f} ms"
                f"  gather / that {fmt(row['gather_over_peak_bound'])}")
            del rays, hits_t, hits_s, surf, src, dst

    with open(out, "w") as f:
        json.dump({"config": a.config, "scene": cfgd["scene"], "rounds": a.rounds, "hbm_peak_tbs": a.hbm_tbs,
                   "bbox_diagonal": float(diag), "rows": rows}, f, indent=1)
    log.close()
    rs.close()


if __name__ == "__main__":
    main()
