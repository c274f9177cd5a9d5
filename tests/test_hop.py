"""Host checks of the park kernel's hop (render.hip PARK_HOP) and of the hop
bits in the cell records (context.hip cell32_hop_kernel):
tests/cpp/hop_check.cpp.

A cleared (inverted) hop bit f in a cell's mask words says: a ray leaving this
cell by a step across face f has no ref left to test in the cell it enters,
so it may walk through that cell without parking.  Checked here by the
sequential traceRay walk with and without hops (identical hit bits), on the
record words themselves (low bits unchanged, every other word reads "no hop",
the release statistic unchanged), with two controls that must change a ray,
and on tie rays for the kernel's own face rule.  The GPU images are checked
against the oracle in test_hop_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [("cornell", (32, 32, 32)), ("contest", (128, 128, 128)), ("sphere", (24, 16, 40))]
VARIANTS = ("no_hop", "hop", "hop_first_cell", "ctl_not_inverted", "ctl_wrong_face")


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = tmp_path_factory.mktemp("hop") / "libhop.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "zig_raytracing_contest_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hop_check.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for fn in (lib.hop_encoding_check, lib.hop_trace_check, lib.hop_tie_check):
        fn.restype = None
    return lib


_baked = {}


def _scene(name, res):
    if name not in _baked:
        soup = scenes.get_scene(name)
        geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution=res)
        g = geo.scene.grid
        _baked[name] = (geo, np.array(g.bbox_min, np.float32), np.array(g.bbox_max, np.float32),
                        np.array(g.resolution, np.uint32), np.array(g.cell_size, np.float32),
                        np.ascontiguousarray(geo.cells().reshape(-1), np.uint32),
                        np.ascontiguousarray(geo.tri_pos().reshape(-1), np.float32))
    return _baked[name][1:]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name,res", SCENES)
def test_hops_leave_trace_ray_bit_identical(chk, name, res):
    """Random rays (half from outside the box), the eight axis-parallel rays
    and two generations of bounce rays: (t, u, v, ref) identical with the hop,
    with and without hop bits in the first cell's word.  Not vacuous: on the
    contest stand-in and the Cornell box at least 10% of the parks are hopped
    (a scratch model measured 31% and 38%).  The controls -- the bits decoded
    non-inverted, the bit of the wrong face (axis + 1) -- must change a ray.
    The sphere is the field-word grid; its share is printed only."""
    bmin, bmax, r, cs, cells, pos = _scene(name, res)
    rng = np.random.default_rng(7)
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
    bad = np.zeros(5, np.uint64)
    stats = np.zeros(49, np.uint64)
    chk.hop_trace_check(_p(bmin), _p(bmax), _p(r), _p(cs), _p(cells), _p(pos), n, _p(rays), _p(un), bounces,
                        _p(bad), _p(stats))
    s = [int(x) for x in stats]
    parks, useless = s[0], s[1]
    rep = {"scene": name, "rays": s[48], "parks": parks, "useless_share": round(useless / max(parks, 1), 3),
           "useless_run_histogram_1_to_8plus": s[40:48]}
    for v, key in enumerate(VARIANTS):
        rep[key] = {"differing_rays": int(bad[v]), "parks": s[8 * v], "hops": s[8 * v + 2],
                    "parks_removed_share": round(s[8 * v + 2] / max(parks, 1), 3)}
    print(rep)
    assert s[48] > n and parks > 1000
    assert bad[1] == 0 and bad[2] == 0
    # a hop removes exactly one park
    assert s[8] + s[8 + 2] == parks and s[16] + s[16 + 2] == parks
    assert s[16 + 2] >= s[8 + 2]
    if name != "sphere":
        assert s[8 + 2] >= 0.10 * parks
        assert bad[3] > 0 and bad[4] > 0


@pytest.mark.parametrize("name,res", SCENES)
def test_record_words_keep_their_masks(chk, name, res):
    """Every (cell, face) word: its low n bits are the old mask; the words of
    empty cells and of cells of 27 refs or more have ones in every bit from 26
    up that is no mask bit and decode to no hop, as does an all-ones word; the
    six hop bits are the same in a cell's six words; the share of empty low
    masks over the occupied cells' faces -- the release statistic -- is what
    the old words gave."""
    bmin, bmax, r, cs, cells, pos = _scene(name, res)
    out = np.zeros(9, np.uint64)
    chk.hop_encoding_check(_p(bmin), _p(bmax), _p(r), _p(cs), _p(cells), _p(pos), _p(out))
    o = [int(x) for x in out]
    print({"scene": name, "low_bits_differ": o[0], "plain_words_wrong": o[1], "plain_words_hop": o[2],
           "faces": o[3], "zero_masks": o[4], "zero_masks_old": o[5], "release_frac": round(o[4] / max(o[3], 1), 4),
           "hops_offered": o[6], "cells_1_to_26": o[7], "hop_bits_differ_between_faces": o[8]})
    assert o[0] == 0 and o[1] == 0 and o[2] == 0 and o[8] == 0
    assert o[4] == o[5] and o[3] > 0
    assert o[6] > 0 and o[7] > 0


def test_release_fraction_is_the_documented_one(chk):
    """The release gate must not move: 0.291 on the contest stand-in at its
    bench grid (128^3), as documented."""
    bmin, bmax, r, cs, cells, pos = _scene(*SCENES[1])
    out = np.zeros(9, np.uint64)
    chk.hop_encoding_check(_p(bmin), _p(bmax), _p(r), _p(cs), _p(cells), _p(pos), _p(out))
    frac = int(out[4]) / int(out[3])
    print(round(frac, 4))
    assert abs(frac - 0.291) < 0.0006, frac


def test_face_rule_on_ties(chk):
    """Rays through cell edges and corners (exact diagonals from cell corners
    on power-of-two grids, zero components): the stepped packed word changes
    inside exactly the field of the axis DDA_STEP stepped, and the trip's test
    against the hop's field masks equals the hop bit of the face crossed, for
    field words and brick-major words."""
    out = np.zeros(5, np.uint64)
    chk.hop_tie_check(24, 1500, _p(out))
    steps, ties, outside, wrong, rays = (int(x) for x in out)
    print({"rays": rays, "steps": steps, "tie_steps": ties, "outside_field": outside, "wrong_bit": wrong})
    assert rays > 10000 and ties > 1000
    assert outside == 0 and wrong == 0
