"""The park kernel with the back-face cull masks (escape.h bfc_cull) forced on
and forced off, with the escape table on and off and the park release on and
off: RGB8, linear radiance and segments equal the CPU oracle's on the Cornell
and contest golden fixtures at their golden sizes and on a hand-made scene
(one cell of exactly 32 refs and one of 33, a coincident pair of
opposite-facing triangles, a zero-area triangle, walls whose normals are
exactly an axis); and batch ray queries through the park kernel, where every
ray is a segment's first cell, axis-parallel rays included."""
import itertools
import os

import numpy as np
import pytest

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

from edge_scenes import HAND_RES, hand_scene

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

def test_hand_scene_has_the_cells_it_is_about():
    soup = hand_scene()
    geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution=HAND_RES)
    cells = geo.cells().reshape(-1, 2).astype(np.int64)
    counts = cells[:, 1] - cells[:, 0]
    at = lambda x, y, z: int(counts[(z * 8 + y) * 8 + x])
    assert at(2, 3, 2) == 32 and at(5, 3, 5) == 33


# (scene key, resolution): the frame and what the oracle gave for it
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
    soup = hand_scene()
    cam = camera_for(soup, None, 32, 32)
    c = soup.camera(None)
    ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, 32, 32)
    rgb, lin, ctr = oracle_mod.OracleScene(soup, HAND_RES).render(ocam, 4, 4, oracle_mod.RNG_PATH, 0, 16)
    out["hand"] = (soup, HAND_RES, cam, 4, 4, rgb, lin, int(ctr[0]))
    return out


@pytest.fixture(scope="module")
def cases(oracle_mod):
    c = _cases(oracle_mod)
    ctx = {}

    def get(name):
        if name not in ctx:
            ctx[name] = RenderScene(c[name][0], c[name][1])
        return (ctx[name],) + c[name][2:]
    yield get
    for rs in ctx.values():
        rs.close()


FLAGS = [(b, e, r) for b, e, r in itertools.product(
    (native.FLAG_BFCULL, native.FLAG_NO_BFCULL), (native.FLAG_ESCAPE, native.FLAG_NO_ESCAPE),
    (native.FLAG_RELEASE, native.FLAG_NO_RELEASE))]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=["-".join(("cull" if b == native.FLAG_BFCULL else "nocull",
                                                        "esc" if e == native.FLAG_ESCAPE else "noesc",
                                                        "rel" if r == native.FLAG_RELEASE else "norel"))
                                              for b, e, r in FLAGS])
@pytest.mark.parametrize("name", ["cornell", "contest", "hand"])
def test_render_with_cull_masks_bitexact_vs_oracle(cases, name, flags):
    rs, cam, spp, mb, rgb, lin, segs = cases(name)
    img, res = rs.render(cam, num_samples=spp, max_bounce=mb, linear=True, flags=flags[0] | flags[1] | flags[2])
    pix = native.tile_pixels(cam.w, cam.h)
    assert np.array_equal(img.reshape(-1, 3), rgb)
    assert np.array_equal(res["linear"].view(np.uint32), lin[pix].view(np.uint32))
    assert res["stats"]["segments"] == segs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hand", "contest"])
def test_trace_with_cull_masks_identical(cases, name):
    """Batch queries through the park kernel (every ray parks in its first
    cell with the cull mask): axis-parallel rays onto the axis-aligned walls,
    rays with zero and tiny components, random rays from inside the grid --
    the same hits with the masks, without them and through the lane walk."""
    rs = cases(name)[0]
    soup = rs.soup
    lo = soup.pos.reshape(-1, 3).min(0)
    hi = soup.pos.reshape(-1, 3).max(0)
    rng = np.random.default_rng(3)
    n = 6000
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d[:600] = axes[np.arange(600) % 6]                                   # axis-parallel
    k = np.arange(600, 1200)
    d[k, k % 3] = np.array([0.0, 1e-9, -1e-9, 1e-20, -1e-20, 3e-8])[k % 6]   # zero and tiny components
    d[600:1200] /= np.linalg.norm(d[600:1200], axis=1, keepdims=True)
    d = d.astype(np.float32)
    on = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_BFCULL)
    off = rs.trace(o, d, flags=native.TRACE_PARK | native.FLAG_NO_BFCULL)
    walk = rs.trace(o, d, flags=native.FLAG_LANE_WALK)
    assert int((on["triangle"] != native.MISS).sum()) > n // 10
    for key in ("t", "u", "v", "triangle"):
        assert np.array_equal(on[key].view(np.uint32), off[key].view(np.uint32)), key
        assert np.array_equal(on[key].view(np.uint32), walk[key].view(np.uint32)), key
