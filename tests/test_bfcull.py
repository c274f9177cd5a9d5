"""Host checks of the back-face cull masks (csrc/escape.h bfc_cull; the park
kernel's first cell, render.hip): tests/cpp/bfcull_check.cpp.

A cleared bit of a (cell, direction bin) mask says tri_ray's determinant test
rejects that ref for EVERY direction the device can put into the bin.  Checked
on random and adversarial triangles against the directions of every bin, with
the two controls that the check can fail (no error margin; no widening of the
cone), and by the sequential traceRay walk over baked scenes with and without
the masks.  The GPU images with the masks forced on are checked against the
oracle in test_bfcull_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = tmp_path_factory.mktemp("bfcull") / "libbfcull.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "zig_raytracing_contest_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "bfcull_check.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.bfc_fuzz.restype = None
    lib.bfc_fuzz.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p]
    lib.bfc_trace_check.restype = C.c_int
    return lib


KEYS = ("culled_pairs", "violations", "bits", "cleared", "dirs_outside", "dirs", "dirs_bin_moves", "nonfinite_cleared")
MARGIN, EPS = 2.0 ** -21, 1e-3      # escape.h kBfcMargin, kEscEps


def fuzz(lib, seed, ntri, per_bin, margin, eps):
    out = np.zeros(8, np.uint64)
    lib.bfc_fuzz(seed, ntri, per_bin, margin, eps, out.ctypes.data_as(C.c_void_p))
    return dict(zip(KEYS, (int(x) for x in out)))


def test_cleared_bit_implies_rejected_determinant(chk):
    """Slivers, edges of 1e-20 .. 1e20, zero area, axis-aligned and slightly
    tilted normals, planes through a test direction, NaN / inf edges; per
    escape bin its corners (exact and a few ulp off), interior, zero and tiny
    slopes, ties between axes, the reciprocal moved by up to 2 ulp."""
    r = fuzz(chk, 1, 1500, 400, MARGIN, EPS)
    print(r)
    assert r["violations"] == 0 and r["nonfinite_cleared"] == 0, r
    # not vacuous: the masks clear bits, many (triangle, direction) pairs
    # sit in cleared bins, and the perturbed reciprocal does move bins
    assert r["cleared"] > 0.2 * r["bits"] and r["culled_pairs"] > 10 ** 7 and r["dirs_bin_moves"] > 100, r


def test_the_margin_and_the_widening_are_both_needed(chk):
    """Controls: without the error margin, and without the cone's widening,
    the same check finds cleared bits whose determinant is not rejected."""
    no_margin = fuzz(chk, 2, 800, 200, 0.0, EPS)
    no_widen = fuzz(chk, 2, 800, 200, MARGIN, 0.0)
    print(no_margin, no_widen)
    assert no_margin["violations"] > 0, no_margin
    assert no_widen["violations"] > 0, no_widen
    assert fuzz(chk, 2, 800, 200, MARGIN, EPS)["violations"] == 0


@pytest.mark.parametrize("name,res", [("cornell", (32, 32, 32)), ("contest", (128, 128, 128)),
                                      ("sphere", (24, 16, 40))])
def test_masks_leave_trace_ray_bit_identical(chk, name, res):
    """Sequential traceRay over random rays and two generations of bounce
    rays (from the hit point, normalize(n_geo + unit vector)): every ref, the
    entry-face masks, those plus the cull mask in the first cell (what the
    park kernel does), and both masks in every cell -- identical (t, u, v,
    ref) bits.  The dropped share of the bounce rays' tests is printed: a
    property of the scene, not a pass condition."""
    soup = scenes.get_scene(name)
    geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution=res)
    g = geo.scene.grid
    bmin = np.array(g.bbox_min, np.float32)
    bmax = np.array(g.bbox_max, np.float32)
    r = np.array(g.resolution, np.uint32)
    cs = np.array(g.cell_size, np.float32)
    cells = np.ascontiguousarray(geo.cells().reshape(-1), np.uint32)
    pos = np.ascontiguousarray(geo.tri_pos().reshape(-1), np.float32)
    rng = np.random.default_rng(13)
    n, bounces = 2500, 2
    o = bmin + (bmax - bmin) * rng.random((n, 3), np.float32)
    o[: n // 2] = bmin - (bmax - bmin) * 0.5 + (bmax - bmin) * 2.0 * rng.random((n // 2, 3), np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:8] = np.eye(3, dtype=np.float32)[[0, 1, 2, 0, 1, 2, 0, 1]] * np.float32([1, 1, 1, -1, -1, -1, 1, -1])[:, None]
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), np.float32)
    un = rng.normal(size=(n * bounces, 3)).astype(np.float32)
    un /= np.linalg.norm(un, axis=1, keepdims=True)
    un = np.ascontiguousarray(un, np.float32)
    stats = np.zeros(9, np.uint64)
    f = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = chk.bfc_trace_check(f(bmin), f(bmax), f(r), f(cs), f(cells), f(pos), n, f(rays), f(un), bounces, f(stats))
    s = [int(x) for x in stats]
    first, later = s[0], s[1]
    print({"scene": name, "bounce_rays": s[8], "tests_first_cell": first, "tests_later_cells": later,
           "kept_face_masks": s[2] + s[3], "kept_first_cell_cull": s[4] + s[5], "kept_every_cell_cull": s[6] + s[7],
           "first_cell_dropped": round(1 - s[4] / max(first, 1), 3),
           "every_cell_dropped_vs_face_masks": round(1 - (s[6] + s[7]) / max(s[2] + s[3], 1), 3)})
    assert bad == 0
    assert s[8] > n // 20        # there were bounce rays
