"""The park kernel with the escape table keyed by sub-brick regions
(escape.h EscShape; wf_park_kernel<ESC = true>): with the table forced on and
forced off, the park release and the cull masks on and off, RGB8, linear
radiance and segments equal the CPU oracle's on the Cornell and contest
goldens at their golden sizes and on a hand-made skimming scene -- a ground
plane one cell thick with a few boxes on it, the camera low over the plane --
on a 16^3 grid (brick-major words), on non-power-of-two grids (field words,
clipped edge regions) and on grids whose smallest cells lie along x, y and z
(the region's long axis).  The same scenes with the brick-level table kept
(ZRT_ESC_BRICK, the fallback of a table that does not fit), and batch ray
queries through the park kernel against the lane walk."""
import dataclasses
import itertools
import math
import os

import numpy as np
import pytest

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (grid resolution, scene extent): the smallest cells along y, y, x, z
SKIM = {
    "skim16": ((16, 16, 16), (16.0, 6.0, 12.0)),
    "skim_npot": ((12, 10, 14), (16.0, 6.0, 12.0)),
    "skim_x": ((20, 6, 9), (16.0, 6.0, 12.0)),
    "skim_z": ((8, 8, 32), (16.0, 6.0, 12.0)),
}


def skim_scene(ext):
    """A floor just above y = 0 (every cell of the lowest layer, no other),
    four boxes standing on it, a small triangle pinning the bbox's far top
    corner, and a camera a little above the floor looking along it."""
    s = scenes.get_scene("cornell")
    X, Y, Z = ext
    tris = []
    quad = lambda a, b, c, d: [a + b + c, a + c + d]
    h = 0.01 * Y
    tris += quad([0, h, 0], [0, h, Z], [X, h, Z], [X, h, 0])             # floor, normal +y
    tris += [[0, 0, 0, 0.02 * X, 0, 0, 0, 0, 0.02 * Z]]                  # bbox corners
    tris += [[X, Y, Z, 0.98 * X, Y, Z, X, Y, 0.98 * Z]]
    for (bx, bz, w, hh) in ((0.3, 0.3, 0.08, 0.3), (0.6, 0.5, 0.05, 0.55), (0.45, 0.75, 0.1, 0.15), (0.8, 0.2, 0.04, 0.8)):
        x0, x1, z0, z1, y1 = bx * X, (bx + w) * X, bz * Z, (bz + w) * Z, hh * Y
        tris += quad([x0, h, z0], [x0, y1, z0], [x1, y1, z0], [x1, h, z0])
        tris += quad([x0, h, z1], [x1, h, z1], [x1, y1, z1], [x0, y1, z1])
        tris += quad([x0, h, z0], [x0, h, z1], [x0, y1, z1], [x0, y1, z0])
        tris += quad([x1, h, z0], [x1, y1, z0], [x1, y1, z1], [x1, h, z1])
        tris += quad([x0, y1, z0], [x0, y1, z1], [x1, y1, z1], [x1, y1, z0])
    pos = np.array(tris, np.float32).reshape(-1, 9)
    n = len(pos)
    e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
    nr = np.cross(e1, e2)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    cam = scenes.CameraDef("Skim", scenes.look_at((0.05 * X, 0.12 * Y, 0.05 * Z), (0.9 * X, 0.08 * Y, 0.8 * Z)),
                           math.radians(60.0), None)
    return dataclasses.replace(s, name="escape_skim", pos=pos, nrm=np.tile(nr, (1, 3)).astype(np.float32),
                               uv=np.zeros((n, 6), np.float32),
                               mat=(np.arange(n) % s.num_materials).astype(s.mat.dtype), cameras=[cam])


NAMES = ["cornell", "contest"] + list(SKIM)


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
    for name, (res, ext) in SKIM.items():
        soup = skim_scene(ext)
        cam = camera_for(soup, None, 40, 24)
        c = soup.camera(None)
        ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, 40, 24)
        rgb, lin, ctr = oracle_mod.OracleScene(soup, res).render(ocam, 4, 6, oracle_mod.RNG_PATH, 0, 16)
        out[name] = (soup, res, cam, 4, 6, rgb, lin, int(ctr[0]))
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


def test_skim_scene_is_a_plane_one_cell_thick():
    for name, (res, ext) in SKIM.items():
        soup = skim_scene(ext)
        geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution=res)
        cells = geo.cells().reshape(-1, 2).astype(np.int64)
        occ = (cells[:, 1] > cells[:, 0]).reshape(res[2], res[1], res[0])
        assert occ[:, 0, :].all(), name                     # the whole lowest layer
        assert occ[:, 1:, :].mean() < 0.08, name            # and little else: rays skim it
        cs = np.array(ext) / np.array(res)
        assert int(np.argmin(cs)) == {"skim16": 1, "skim_npot": 1, "skim_x": 0, "skim_z": 2}[name]


FLAGS = [(e, r, b) for e, r, b in itertools.product(
    (native.FLAG_ESCAPE, native.FLAG_NO_ESCAPE), (native.FLAG_RELEASE, native.FLAG_NO_RELEASE),
    (native.FLAG_BFCULL, native.FLAG_NO_BFCULL))]
FLAG_IDS = ["-".join(("esc" if e == native.FLAG_ESCAPE else "noesc", "rel" if r == native.FLAG_RELEASE else "norel",
                      "cull" if b == native.FLAG_BFCULL else "nocull")) for e, r, b in FLAGS]


def _check(rs, cam, spp, mb, rgb, lin, segs, flags):
    img, res = rs.render(cam, num_samples=spp, max_bounce=mb, linear=True, flags=flags)
    pix = native.tile_pixels(cam.w, cam.h)
    assert np.array_equal(img.reshape(-1, 3), rgb)
    assert np.array_equal(res["linear"].view(np.uint32), lin[pix].view(np.uint32))
    assert res["stats"]["segments"] == segs


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_render_with_region_table_bitexact_vs_oracle(cases, name, flags):
    _check(*cases(name), flags[0] | flags[1] | flags[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["contest", "skim16", "skim_npot"])
def test_render_with_brick_table_kept_bitexact_vs_oracle(frames, name, monkeypatch):
    """The fallback of a region table that does not fit: the context keeps
    the brick-level table and the same kernel asks it per brick."""
    monkeypatch.setenv("ZRT_ESC_BRICK", "1")
    rs = RenderScene(frames[name][0], frames[name][1])
    try:
        for rel in (native.FLAG_RELEASE, native.FLAG_NO_RELEASE):
            _check(rs, *frames[name][2:], native.FLAG_ESCAPE | rel)
    finally:
        rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["contest"] + list(SKIM))
def test_trace_with_region_table_identical(cases, name):
    """Batch queries: rays from inside the grid, a third of them nearly
    parallel to the ground plane, through the park kernel with the table, the
    park kernel without it and the lane walk: the same (t, u, v, ref)."""
    rs = cases(name)[0]
    soup = rs.soup
    lo = soup.pos.reshape(-1, 3).min(0)
    hi = soup.pos.reshape(-1, 3).max(0)
    rng = np.random.default_rng(11)
    n = 6000
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d[: n // 3, 1] *= 0.03                                              # skimming
    o[: n // 3, 1] = (lo[1] + (hi[1] - lo[1]) * (0.02 + 0.1 * rng.random(n // 3))).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    on = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_ESCAPE)
    off = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_NO_ESCAPE)
    walk = rs.trace(o, d, flags=native.FLAG_LANE_WALK)
    hits = int((on["triangle"] != native.MISS).sum())
    assert n // 10 < hits < n
    for key in ("t", "u", "v", "triangle"):
        assert np.array_equal(on[key].view(np.uint32), off[key].view(np.uint32)), key
        assert np.array_equal(on[key].view(np.uint32), walk[key].view(np.uint32)), key
