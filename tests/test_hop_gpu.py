"""The park kernel with the hop (render.hip PARK_HOP: a lane walking on from a
parked cell passes through the next cell when the parked cell's record says
nothing is left to test there) forced on and forced off, crossed with the
escape table, the park release and the cull masks each on and off: RGB8, linear
radiance and segments equal the CPU oracle's on the Cornell and contest golden
fixtures at their golden sizes and on a hand-made scene; and batch queries
(closest hit, bounded segments, any-hit) through the park kernel with and
without the hop against the lane walk."""
import dataclasses
import itertools
import math
import os

import numpy as np
import pytest

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOP_RES = (8, 8, 8)
# cells of the hand-made scene with exactly this many refs, each at an end of a
# row of cells that one long triangle runs through
HOP_CELLS = {(1, 2, 2): 26, (6, 2, 2): 33, (2, 1, 5): 27, (5, 5, 1): 32}


def hop_scene():
    """An 8^3-cell box [0, 8]^3: floor (y = 0) and back wall (z = 0); one long
    triangle along each axis inside one row of cells (x: cells 0..6 of row
    y = 2, z = 2; y: cells 1..6 of row x = 2, z = 5, as a coincident pair of
    opposite-facing triangles; z: cells 1..7 of row x = 5, y = 5, up to the
    grid's boundary, so a ray along +z leaves the grid on the step after a
    hop), which rays along the row in either direction meet again in every
    cell with nothing left to test; and clusters of small triangles that
    bring the cells of HOP_CELLS to exactly 26, 27, 32 and 33 refs."""
    s = scenes.get_scene("cornell")
    tris = []
    quad = lambda a, b, c, d: [a + b + c, a + c + d]
    tris += quad([0, 0, 0], [0, 0, 8], [8, 0, 8], [8, 0, 0])            # floor, normal +y
    tris += quad([0, 0, 0], [8, 0, 0], [8, 8, 0], [0, 8, 0])            # back wall, normal +z
    tris += [[8, 8, 8, 7.5, 8, 8, 8, 8, 7.5]]                            # bbox corner
    long_x = [0.2, 2.2, 2.2, 6.8, 2.2, 2.8, 0.2, 2.8, 2.5]
    long_y = [2.2, 1.2, 5.2, 2.8, 6.8, 5.2, 2.5, 1.2, 5.8]
    long_z = [5.2, 5.2, 1.2, 5.8, 5.2, 7.8, 5.5, 5.8, 1.2]
    tris += [long_x, long_y, long_y[0:3] + long_y[6:9] + long_y[3:6], long_z]
    rng = np.random.default_rng(11)

    def cluster(cell, n):
        out = []
        c = np.array(cell, np.float64) + 0.5
        for _ in range(n):
            p = c + rng.uniform(-0.25, 0.25, 3)
            out.append(list(np.concatenate([p, p + rng.uniform(-0.15, 0.15, 3), p + rng.uniform(-0.15, 0.15, 3)])))
        return out
    tris += cluster((1, 2, 2), 25) + cluster((6, 2, 2), 32) + cluster((2, 1, 5), 25) + cluster((5, 5, 1), 31)
    pos = np.array(tris, np.float32).reshape(-1, 9)
    n = len(pos)
    e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
    nr = np.cross(e1, e2)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    cam = scenes.CameraDef("Hop", scenes.look_at((4.0, 4.0, 14.0), (4.0, 4.0, 0.0)), math.radians(45.0), None)
    return dataclasses.replace(s, name="hop_hand", pos=pos, nrm=np.tile(nr, (1, 3)).astype(np.float32),
                               uv=np.zeros((n, 6), np.float32),
                               mat=(np.arange(n) % s.num_materials).astype(s.mat.dtype), cameras=[cam])


def test_hop_scene_has_the_cells_it_is_about():
    soup = hop_scene()
    geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution=HOP_RES)
    cells = geo.cells().reshape(-1, 2).astype(np.int64)
    counts = cells[:, 1] - cells[:, 0]
    at = lambda x, y, z: int(counts[(z * 8 + y) * 8 + x])
    for cell, want in HOP_CELLS.items():
        assert at(*cell) == want, (cell, at(*cell))
    # the long triangles' rows: at least four cells in a row hold them
    assert all(at(x, 2, 2) >= 1 for x in range(0, 7))
    assert all(at(2, y, 5) >= 2 for y in range(1, 7))
    assert all(at(5, 5, z) >= 1 for z in range(1, 8))


def _cases(oracle_mod):
    out = {}
    for name in ("cornell", "contest"):
        g = np.load(os.path.join(GOLD, f"render_{name}.npz"), allow_pickle=False)
        soup = scenes.get_scene(name)
        cname = str(g["camera"]) or None
        c = soup.camera(cname)
        cam = camera_for(soup, cname, None if c.aspect else int(g["w"]), int(g["h"]))
        out[name] = (soup, (128, 128, 128), cam, int(g["spp"]), int(g["max_bounce"]), g["rgb"], g["linear"],
                     int(g["counters"][0]))
    soup = hop_scene()
    cam = camera_for(soup, None, 64, 64)
    c = soup.camera(None)
    ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, 64, 64)
    osc = oracle_mod.OracleScene(soup, HOP_RES)
    for mb in (4, 1):
        rgb, lin, ctr = osc.render(ocam, 4, mb, oracle_mod.RNG_PATH, 0, 16)
        out[f"hand-mb{mb}"] = (soup, HOP_RES, cam, 4, mb, rgb, lin, int(ctr[0]))
    return out


@pytest.fixture(scope="module")
def cases(oracle_mod):
    c = _cases(oracle_mod)
    ctx = {}

    def get(name):
        key = name.split("-")[0]
        if key not in ctx:
            ctx[key] = RenderScene(c[name][0], c[name][1])
        return (ctx[key],) + c[name][2:]
    yield get
    for rs in ctx.values():
        rs.close()


FLAGS = list(itertools.product((native.FLAG_HOP, native.FLAG_NO_HOP), (native.FLAG_ESCAPE, native.FLAG_NO_ESCAPE),
                               (native.FLAG_RELEASE, native.FLAG_NO_RELEASE),
                               (native.FLAG_BFCULL, native.FLAG_NO_BFCULL)))
IDS = ["-".join(("hop" if h == native.FLAG_HOP else "nohop", "esc" if e == native.FLAG_ESCAPE else "noesc",
                 "rel" if r == native.FLAG_RELEASE else "norel", "cull" if b == native.FLAG_BFCULL else "nocull"))
       for h, e, r, b in FLAGS]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
@pytest.mark.parametrize("name", ["cornell", "contest", "hand-mb4", "hand-mb1"])
def test_render_with_hop_bitexact_vs_oracle(cases, name, flags):
    rs, cam, spp, mb, rgb, lin, segs = cases(name)
    img, res = rs.render(cam, num_samples=spp, max_bounce=mb, linear=True, flags=flags[0] | flags[1] | flags[2] | flags[3])
    pix = native.tile_pixels(cam.w, cam.h)
    assert np.array_equal(img.reshape(-1, 3), rgb)
    assert np.array_equal(res["linear"].view(np.uint32), lin[pix].view(np.uint32))
    assert res["stats"]["segments"] == segs


def _query_rays(soup, n=6000):
    """Rays from inside the scene's box: axis-parallel (along the long
    triangles' rows among them), exact diagonals from cell corners (ties of
    the crossing ts) and random ones."""
    lo = soup.pos.reshape(-1, 3).min(0)
    hi = soup.pos.reshape(-1, 3).max(0)
    rng = np.random.default_rng(5)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d[:900] = axes[np.arange(900) % 6]                                   # axis-parallel
    k = np.arange(900, 1800)
    cs = (hi - lo) / 8.0
    o[k] = (lo + cs * rng.integers(0, 9, (900, 3))).astype(np.float32)   # on cell corners of an 8^3 grid
    sg = rng.choice([-1.0, 1.0], (900, 3))
    d[k] = sg * np.where((k % 2 == 0)[:, None], 1.0, np.array([1.0, 2.0, 1.0]))
    d[k] /= np.linalg.norm(d[k], axis=1, keepdims=True)
    return o, d.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hand-mb4", "contest"])
def test_queries_with_hop_identical(cases, name):
    """zrt_context_trace and zrt_context_segments (closest and any-hit)
    through the park kernel with the hop and without it, and through the lane
    walk: the same answers, bit for bit."""
    rs = cases(name)[0]
    o, d = _query_rays(rs.soup)
    n = len(o)
    on = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_HOP)
    off = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_NO_HOP)
    walk = rs.trace(o, d, flags=native.FLAG_LANE_WALK)
    assert int((on["triangle"] != native.MISS).sum()) > n // 10
    for key in ("t", "u", "v", "triangle"):
        assert np.array_equal(on[key].view(np.uint32), off[key].view(np.uint32)), key
        assert np.array_equal(on[key].view(np.uint32), walk[key].view(np.uint32)), key
    # bounded segments: ends before, at and past the first hit
    t = np.where(np.isfinite(walk["t"]), walk["t"], np.float32(1.0)).astype(np.float32)
    tm = (t * np.float32([0.5, 1.0, 1.5, 4.0])[np.arange(n) % 4]).astype(np.float32)
    for any_hit in (False, True):
        son = rs.segments(o, d, tm, any_hit=any_hit, flags=native.TRACE_PARK | native.FLAG_HOP)
        soff = rs.segments(o, d, tm, any_hit=any_hit, flags=native.TRACE_PARK | native.FLAG_NO_HOP)
        swalk = rs.segments(o, d, tm, any_hit=any_hit, flags=native.FLAG_LANE_WALK)
        assert np.array_equal(son["occluded"], soff["occluded"]) and np.array_equal(son["occluded"], swalk["occluded"])
        assert 0 < int(son["occluded"].sum()) < n
        if not any_hit:
            for key in ("t", "u", "v", "triangle"):
                assert np.array_equal(son[key].view(np.uint32), soff[key].view(np.uint32)), key
                assert np.array_equal(son[key].view(np.uint32), swalk[key].view(np.uint32)), key
