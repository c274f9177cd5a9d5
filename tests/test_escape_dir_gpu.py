"""The park kernel with the direction-aware escape table (escape.h
esc_dir_occupied, context.hip context_escape): a region's bit is set when every
later cell is empty or holds only refs the ray's direction bin rejects by their
determinant.  With the table forced on, crossed with the park release, the cull
masks and the hop on and off, and with the plain table kept (ZRT_ESC_PLAIN):
RGB8, linear radiance and segments equal the CPU oracle's on the Cornell and
contest goldens at their golden sizes and on a hand-made scene -- a ground
quad, a lamp sphere, a wall that faces away from most bounce rays -- at
64 x 36 pixels, 16 spp, max_bounce 4 on 16^3 and 12 x 5 x 9 grids.  Batch
trace, segment and any-hit queries through the park kernel and the lane walk
agree bit for bit, surface-start, axis-parallel, zero-component and
unnormalised rays among them.  The sweep build's counters show that the
direction-aware table ends more lanes in fewer lane steps than the plain one."""
import dataclasses
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

HAND = {"hand16": (16, 16, 16), "hand_npot": (12, 5, 9)}
EXT = (16.0, 6.0, 12.0)


def hand_scene():
    """A ground quad facing up, a lamp sphere above it, a wall standing at the
    far side whose front faces away from the ground's bounce rays, and two
    small triangles pinning the bbox."""
    s = scenes.get_scene("cornell")
    X, Y, Z = EXT
    tris = []
    quad = lambda a, b, c, d: [a + b + c, a + c + d]
    h = 0.01 * Y
    tris += quad([0, h, 0], [0, h, Z], [X, h, Z], [X, h, 0])             # ground, normal +y
    tris += quad([0.1 * X, h, 0.9 * Z], [0.9 * X, h, 0.9 * Z], [0.9 * X, 0.6 * Y, 0.9 * Z], [0.1 * X, 0.6 * Y, 0.9 * Z])  # wall, normal +z
    tris += [[0, 0, 0, 0.02 * X, 0, 0, 0, 0, 0.02 * Z]]                  # bbox corners
    tris += [[X, Y, Z, 0.98 * X, Y, Z, X, Y, 0.98 * Z]]
    cx, cy, cz, r = 0.5 * X, 0.75 * Y, 0.4 * Z, 0.1 * Y                  # the lamp: a 6 x 8 sphere, outward
    nu, nv = 6, 8
    P = lambda i, j: [cx + r * math.sin(math.pi * i / nu) * math.cos(2 * math.pi * j / nv),
                      cy + r * math.cos(math.pi * i / nu),
                      cz + r * math.sin(math.pi * i / nu) * math.sin(2 * math.pi * j / nv)]
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1)
            if i > 0:
                tris.append(a + d + c)
            if i < nu - 1:
                tris.append(a + c + b)
    pos = np.array(tris, np.float32).reshape(-1, 9)
    n = len(pos)
    e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
    nr = np.cross(e1, e2)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    mat = (np.arange(n) % s.num_materials).astype(s.mat.dtype)      # (the Cornell box's, its emitter among them)
    cam = scenes.CameraDef("Hand", scenes.look_at((0.5 * X, 0.5 * Y, 0.02 * Z), (0.5 * X, 0.1 * Y, 0.7 * Z)),
                           math.radians(60.0), None)
    return dataclasses.replace(s, name="escape_dir_hand", pos=pos, nrm=np.tile(nr, (1, 3)).astype(np.float32),
                               uv=np.zeros((n, 6), np.float32), mat=mat, cameras=[cam])


NAMES = ["cornell", "contest"] + list(HAND)


# name -> (soup, resolution, camera, spp, max_bounce, the oracle's rgb, linear, segments)
@pytest.fixture(scope="module")
def frames(oracle_mod):
    out = {}
    for name in ("cornell", "contest"):
        g = np.load(os.path.join(GOLD, f"render_{name}.npz"), allow_pickle=False)
        soup = scenes.get_scene(name)
        cname = str(g["camera"]) or None
        c = soup.camera(cname)
        cam = camera_for(soup, cname, None if c.aspect else int(g["w"]), int(g["h"]))
        out[name] = (soup, (128, 128, 128), cam, int(g["spp"]), int(g["max_bounce"]), g["rgb"], g["linear"],
                     int(g["counters"][0]))
    soup = hand_scene()
    for name, res in HAND.items():
        cam = camera_for(soup, None, 64, 36)
        c = soup.camera(None)
        ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, 64, 36)
        rgb, lin, ctr = oracle_mod.OracleScene(soup, res).render(ocam, 16, 4, oracle_mod.RNG_PATH, 0, 16)
        out[name] = (soup, res, cam, 16, 4, rgb, lin, int(ctr[0]))
    return out


@pytest.fixture(scope="module")
def cases(frames):
    ctx = {}

    def get(name):
        if name not in ctx:
            ctx[name] = RenderScene(frames[name][0], frames[name][1])
        return (ctx[name],) + frames[name][2:]
    yield get
    for rs in ctx.values():
        rs.close()


def test_hand_scene_has_a_wall_that_faces_away():
    soup = hand_scene()
    for name, res in HAND.items():
        geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution=res)
        cells = geo.cells().reshape(-1, 2).astype(np.int64)
        occ = (cells[:, 1] > cells[:, 0]).reshape(res[2], res[1], res[0])
        assert occ[:, 0, :].all(), name                     # the ground: the whole lowest layer
        assert occ[:, 1:, :].mean() < 0.25, name
    e1, e2 = soup.pos[2, 3:6] - soup.pos[2, 0:3], soup.pos[2, 6:9] - soup.pos[2, 0:3]
    assert np.cross(e1, e2)[2] > 0                          # the wall's front looks along +z, the ground lies at -z


FLAGS = [(r, b, h) for r, b, h in itertools.product(
    (native.FLAG_RELEASE, native.FLAG_NO_RELEASE), (native.FLAG_BFCULL, native.FLAG_NO_BFCULL),
    (native.FLAG_HOP, native.FLAG_NO_HOP))]
FLAG_IDS = ["-".join(("rel" if r == native.FLAG_RELEASE else "norel", "cull" if b == native.FLAG_BFCULL else "nocull",
                      "hop" if h == native.FLAG_HOP else "nohop")) for r, b, h in FLAGS]


def _check(rs, cam, spp, mb, rgb, lin, segs, flags):
    img, res = rs.render(cam, num_samples=spp, max_bounce=mb, linear=True, flags=flags)
    pix = native.tile_pixels(cam.w, cam.h)
    assert np.array_equal(img.reshape(-1, 3), rgb)
    assert np.array_equal(res["linear"].view(np.uint32), lin[pix].view(np.uint32))
    assert res["stats"]["segments"] == segs


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_render_with_direction_table_bitexact_vs_oracle(cases, name, flags):
    _check(*cases(name), native.FLAG_ESCAPE | flags[0] | flags[1] | flags[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_render_with_plain_table_kept_bitexact_vs_oracle(frames, name, monkeypatch):
    """ZRT_ESC_PLAIN: the region table from plain occupancy, as before."""
    monkeypatch.setenv("ZRT_ESC_PLAIN", "1")
    rs = RenderScene(frames[name][0], frames[name][1])
    try:
        for f in (native.FLAG_RELEASE | native.FLAG_BFCULL | native.FLAG_HOP,
                  native.FLAG_NO_RELEASE | native.FLAG_NO_BFCULL | native.FLAG_NO_HOP):
            _check(rs, *frames[name][2:], native.FLAG_ESCAPE | f)
    finally:
        rs.close()


def _query_rays(soup, n, rng):
    """Rays from inside the scene's box: bounce rays from triangle surfaces
    (on the surface itself), axis-parallel, zero-component and unnormalised
    ones (|d|_1 > 4), the rest random unit directions."""
    tri = soup.pos.reshape(-1, 3, 3)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 2
    t = rng.integers(0, len(tri), k)
    b = rng.random((k, 2))
    b = np.where((b.sum(1) > 1)[:, None], 1 - b, b)
    e1, e2 = tri[t, 1] - tri[t, 0], tri[t, 2] - tri[t, 0]
    o[:k] = (tri[t, 0] + b[:, :1] * e1 + b[:, 1:] * e2).astype(np.float32)
    nr = np.cross(e1, e2)
    nr /= np.maximum(np.linalg.norm(nr, axis=1, keepdims=True), 1e-30)
    u = rng.normal(size=(k, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dd = nr + u
    d[:k] = dd / np.maximum(np.linalg.norm(dd, axis=1, keepdims=True), 1e-6)
    m = k + (n - k) // 4
    ax = rng.integers(0, 3, m - k)
    d[k:m] = 0.0
    d[np.arange(k, m), ax] = rng.choice([-1.0, 1.0], m - k)             # axis-parallel
    m2 = m + (n - k) // 4
    d[np.arange(m, m2), rng.integers(0, 3, m2 - m)] = 0.0               # a zero component
    d[m:m2] /= np.maximum(np.linalg.norm(d[m:m2], axis=1, keepdims=True), 1e-6)
    m3 = m2 + (n - k) // 4
    d[m2:m3] *= rng.uniform(3.0, 30.0, (m3 - m2, 1))                    # unnormalised
    return o, d.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["contest"] + list(HAND))
def test_queries_with_direction_table_identical(cases, name):
    """Batch trace, segment and any-hit queries through the park kernel with
    the table, the park kernel without it and the lane walk: the same bits."""
    rs = cases(name)[0]
    o, d = _query_rays(rs.soup, 8000, np.random.default_rng(12))
    on = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_ESCAPE)
    off = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_NO_ESCAPE)
    walk = rs.trace(o, d, flags=native.FLAG_LANE_WALK)
    hits = int((on["triangle"] != native.MISS).sum())
    assert len(o) // 10 < hits < len(o)
    for key in ("t", "u", "v", "triangle"):
        assert np.array_equal(on[key].view(np.uint32), off[key].view(np.uint32)), key
        assert np.array_equal(on[key].view(np.uint32), walk[key].view(np.uint32)), key
    # bounds around the hits: half of them short of the hit, half past it
    tm = np.where(np.isfinite(walk["t"]), walk["t"] * np.where(np.arange(len(o)) % 2 == 0, 0.7, 1.3), 5.0).astype(np.float32)
    for any_hit in (False, True):
        son = rs.segments(o, d, tm, any_hit=any_hit, flags=native.TRACE_PARK | native.FLAG_ESCAPE)
        soff = rs.segments(o, d, tm, any_hit=any_hit, flags=native.TRACE_PARK | native.FLAG_NO_ESCAPE)
        swalk = rs.segments(o, d, tm, any_hit=any_hit, flags=native.FLAG_LANE_WALK)
        for key in son:
            if isinstance(son[key], np.ndarray):
                a = son[key].view(np.uint32 if son[key].dtype.itemsize == 4 else np.uint8)
                assert np.array_equal(a, soff[key].view(a.dtype)), (any_hit, key)
                assert np.array_equal(a, swalk[key].view(a.dtype)), (any_hit, key)
        if any_hit:
            assert 0 < int(np.count_nonzero(son["occluded"])) < len(o)


_COUNTER_SCRIPT = r"""
import io, json, os, sys
sys.path.insert(0, os.environ["ZRT_ROOT"])
sys.path.insert(0, os.path.join(os.environ["ZRT_ROOT"], "tests"))
from zig_raytracing_contest_amd import RenderScene, camera_for, native
import test_escape_dir_gpu as T
soup = T.hand_scene()
cam = camera_for(soup, None, 64, 36)
for plain in (0, 1):
    if plain:
        os.environ["ZRT_ESC_PLAIN"] = "1"
    rs = RenderScene(soup, (16, 16, 16), device=0)
    print("table", plain, file=sys.stderr, flush=True)
    rs.render(cam, num_samples=16, max_bounce=4, flags=native.FLAG_ESCAPE | native.FLAG_ONE_SET)
    rs.close()
"""


@pytest.mark.gpu
def test_direction_table_ends_more_lanes_in_fewer_steps():
    """The sweep build's counters on the hand-made scene, one frame with the
    direction-aware table and one with the plain table: the same segments are
    traced, more lanes are ended by a set bit, fewer lane steps are walked."""
    lib = os.path.join(ROOT, "tools", "bin", "sweep", "libzrt.so")
    if not os.path.exists(lib):
        pytest.fail("tools/bin/sweep/libzrt.so not built (make)")
    env = dict(os.environ, ZRT_LIB=lib, ZRT_ROOT=ROOT, ZRT_PARK_PROFILE="1")
    env.pop("ZRT_ESC_PLAIN", None)
    p = subprocess.run([sys.executable, "-c", _COUNTER_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    tot, cur = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("table "):
            cur = int(line.split()[1])
            tot[cur] = {"escapes": 0, "lane_steps": 0}
        elif cur is not None and line.startswith('{"zrt_walk_steps"'):
            w = json.loads(line)["zrt_walk_steps"]
            tot[cur]["escapes"] += w["escapes"]
            tot[cur]["lane_steps"] += w["lane_steps"]
    print(tot)
    assert tot[0]["escapes"] > 0 and tot[1]["escapes"] > 0
    assert tot[0]["escapes"] > tot[1]["escapes"], tot
    assert tot[0]["lane_steps"] < tot[1]["lane_steps"], tot
