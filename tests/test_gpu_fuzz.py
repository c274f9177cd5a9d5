"""Seeded random scenes against the CPU oracle, bit for bit, in every kernel
mode (round 6).  The fixed edge cases (test_gpu_edges.py) and the benchmark
stand-ins pin the paths one at a time; this file draws scenes that mix them
(the generator: fuzz_scenes.py):

- triangle families: small random triangles, axis-aligned quads (shared
  coordinates: the DDA's ties, linalg.zig:478-496), slivers and degenerate
  ones (Moller-Trumbore's det near 0, linalg.zig:683-722), huge triangles
  spanning the box (refs in many cells: the SAT build, linalg.zig:516-563),
  exact duplicates (equal t: the first ref in cell order wins);
- materials: random RGBA textures of 1-17 texels a side, repeat or clamp
  wrap, uvs outside [0, 1], OPAQUE / MASK / BLEND alpha, emissive factors and
  textures (stage1.zig:381-496, stage3.zig:82-123);
- cameras outside and inside the grid's box, wide and narrow fields of view;
- grid resolutions from 1 to 64 cells per axis (and one above 1024: the wide
  walk), image sizes 1-40 pixels, 1-3 spp, max_bounce 0-5, and the seed.

Each scene renders through the counting build (image, linear radiance and
the traversal counters) and then through the timed kernels in every mode
(escape table forced on / off, frustum bounds, IEEE division, park release
forced on / off, back-face cull masks forced on / off, the lane walk for
every bounce).  The images are the oracle's whatever is drawn.
"""
import os

import numpy as np
import pytest

from zig_raytracing_contest_amd import RenderScene, camera_for, native

from fuzz_scenes import scene as _scene, triangles as _triangles

MODES = {"default": 0, "escape": native.FLAG_ESCAPE, "no_escape": native.FLAG_NO_ESCAPE,
         "frustum": native.FLAG_FRUSTUM, "mt_exact": native.FLAG_MT_EXACT,
         "release": native.FLAG_RELEASE, "no_release": native.FLAG_NO_RELEASE,
         "bfcull": native.FLAG_BFCULL, "no_bfcull": native.FLAG_NO_BFCULL, "lane_walk": native.FLAG_LANE_WALK}
F32 = np.float32


# ZRT_FUZZ_SEEDS=n widens the draw (round 6 ran 2,000 once: profiles/r06)
SEEDS = list(range(int(os.environ.get("ZRT_FUZZ_SEEDS", "160"))))
_KINDS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_scene_bitexact_vs_oracle(oracle_mod, seed):
    soup, res, w, h, spp, mb, rseed = _scene(seed)
    c = soup.camera(None)
    ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, w, h)
    rgb, lin, ctr = oracle_mod.OracleScene(soup, res).render(ocam, spp, mb, oracle_mod.RNG_PATH, rseed, 16)
    cam = camera_for(soup, None, w, h)
    pix = native.tile_pixels(cam.w, cam.h)
    rs = RenderScene(soup, res, device_build=bool(seed % 2))
    try:
        img, out = rs.render(cam, num_samples=spp, max_bounce=mb, seed=rseed, stats=True, linear=True)
        info = (seed, soup.num_triangles, res, w, h, spp, mb)
        assert np.array_equal(img.reshape(-1, 3), rgb), info
        assert np.array_equal(out["linear"].view(np.uint32), lin[pix].view(np.uint32)), info
        st = out["stats"]
        assert (st["segments"], st["cells_visited"], st["triangle_tests"], st["hits"]) == \
            tuple(int(x) for x in ctr[:4]), info
        for mode, flags in MODES.items():
            fast, fo = rs.render(cam, num_samples=spp, max_bounce=mb, seed=rseed, linear=True, flags=flags)
            _KINDS.setdefault(seed, set()).update(rs.context.profile()["kernels"])
            assert np.array_equal(fast.reshape(-1, 3), rgb), (mode,) + info
            assert np.array_equal(fo["linear"].view(np.uint32), lin[pix].view(np.uint32)), (mode,) + info
    finally:
        rs.close()


def test_fuzz_scenes_cover_the_families():
    """The draws reach what the file promises (checked on the host: no GPU
    call): cameras inside the box, wide grids, max_bounce 0, 1-pixel sides,
    masked materials and clamp-wrapped textures."""
    draws = [_scene(s) for s in SEEDS]
    assert any(r[0] > 1024 for _, r, *_ in draws)
    assert any(mb == 0 for *_, mb, _ in draws)
    assert any(min(w, h) == 1 for _, _, w, h, *_ in draws) or any(w * h < 40 for _, _, w, h, *_ in draws)
    assert any(m.alpha_mode == "MASK" and m.base_texture is not None for s, *_ in draws for m in s.materials)
    assert any(t.wrap_s_clamp or t.wrap_t_clamp for s, *_ in draws for t in s.textures)
    assert any(s.num_triangles >= 400 for s, *_ in draws)


MEDIUM = list(range(12))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", MEDIUM)
def test_fuzz_medium_scene_bitexact_vs_oracle(oracle_mod, seed):
    """Larger draws (128-320 pixels a side, 4-16 spp, 2,000-20,000
    triangles, 16-128 cells per axis): queues long enough for several park
    chunks per wave, the two pass sets and multi-pass splits
    (samples_per_pass); default, release forced on and the escape table forced
    on, each equal to the oracle's whole frame."""
    rng = np.random.default_rng(5000 + seed)
    soup, _, _, _, _, _, rseed = _scene(seed + 10000)
    n = int(rng.integers(2000, 20001))
    pos = _triangles(rng, n)
    v = pos.reshape(n, 3, 3)
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    soup.pos = pos
    soup.nrm = np.ascontiguousarray(np.repeat(fn, 3, axis=0).reshape(n, 9), F32)
    soup.uv = np.ascontiguousarray(rng.uniform(-2, 3, (n, 6)), F32)
    soup.mat = rng.integers(0, soup.num_materials, n).astype(np.uint32)
    res = tuple(int(x) for x in rng.integers(16, 129, 3))
    w, h = (int(x) for x in rng.integers(128, 321, 2))
    spp = int(rng.integers(4, 17))
    mb = int(rng.integers(1, 6))
    c = soup.camera(None)
    ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, w, h)
    rgb, lin, ctr = oracle_mod.OracleScene(soup, res).render(ocam, spp, mb, oracle_mod.RNG_PATH, rseed, 16)
    cam = camera_for(soup, None, w, h)
    pix = native.tile_pixels(cam.w, cam.h)
    rs = RenderScene(soup, res, device_build=bool(seed % 2))
    info = (seed, n, res, w, h, spp, mb)
    try:
        for flags, spp_pass in ((0, 0), (native.FLAG_RELEASE, 0), (native.FLAG_ESCAPE, 0), (0, max(1, spp // 3))):
            fast, fo = rs.render(cam, num_samples=spp, max_bounce=mb, seed=rseed, linear=True, flags=flags,
                                 samples_per_pass=spp_pass)
            assert np.array_equal(fast.reshape(-1, 3), rgb), (flags, spp_pass) + info
            assert np.array_equal(fo["linear"].view(np.uint32), lin[pix].view(np.uint32)), (flags, spp_pass) + info
            assert fo["stats"]["segments"] == int(ctr[0]), (flags, spp_pass) + info
    finally:
        rs.close()


@pytest.mark.gpu
def test_fuzz_reached_every_bounce_kernel():
    """(runs after the scenes above) the draws rendered bounces through both
    the park kernel and the lane walk (wide grids, the IEEE-division mode)."""
    if len(_KINDS) < len(SEEDS):
        pytest.skip("the fuzz scenes did not all run in this session")
    seen = set().union(*_KINDS.values())
    assert {"park", "bounce", "primary"} <= seen, seen
