"""The sample axis: few pixels or rays, very many samples, against the CPU
oracle, bit for bit (RGB8, the linear radiance as uint32 patterns, segments;
with the counting build also cells_visited, triangle_tests and hits).

num_samples goes to 65535 in zrt_context_render and zrt_context_radiance, and
radiance probes and lightmap texels are what the queries are for; the other
GPU tests stop at a few hundred samples on a handful of pixels.  At that shape
a wave's 64 primary items belong to one pixel (item = q * S + s), most of the
8 XCD regions of the queue are empty and one holds tens of thousands of items,
s0 + s_local reaches 65534 in later passes, wf_resolve_kernel walks thousands
of rounds per pixel, rad_fanout_kernel fans one ray out to 65535 records, and
the pass split and its lead get odd sample counts (a last pass of one sample
among them).

Two scenes on a (16, 16, 16) grid: Cornell, and the fuzz draw FUZZ_SEED, whose
materials include BLEND with a texture that has alpha and a clamp-wrapped
texture, so the transparency pass-through runs thousands of times per pixel.

Renders: 1x1, 2x1 and 3x3 (9 pixels: more than 8 regions) at spp 1, 15, 16,
17, 63, 64, 65, 4095, 4096 and 65535; 8x8 and 13x5 (65 pixels: a wave boundary
inside a pixel's samples) at 257, 4096 and 65535; max_bounce 4, and 0 and 1 at
1x1 x 65535; the default kernels, the lane walk, the IEEE-division kernels and
the counting build.  Pass splits of 3x3 x 65535; the smallest frame that takes
the two pass sets and their lead (13x10 x 65535 = 8,519,550 samples); the
last-pass-of-one corner at 64x33 x 4097.  Radiance: 1, 7, 9 and 65 rays of
test_query_fuzz_gpu.seed_rays at spp 1, 17, 4096 and 65535 (there 1 and 9 rays),
max_bounce 4 and 1, in five modes, and one batch whose stream keys wrap.

One oracle result per (scene, frame, spp, max_bounce), shared by every mode
and by the host-only tests, which assert from the oracle alone that every case
hits geometry and scatters, and that the textured scene's hits include the
BLEND material.
"""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import fuzz_scenes
import radiance_ref
import trace_ref
from test_query_fuzz_gpu import seed_rays

RES = (16, 16, 16)
FUZZ_SEED = 65           # chosen on the host: test_fuzz_scene_is_the_textured_one, test_tall_*_hit_and_scatter
SCENES = ("cornell", "fuzz")
THREADS = 16

SPPS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 65535)
SMALL_FRAMES = ((1, 1), (2, 1), (3, 3))
WAVE_FRAMES = ((8, 8), (13, 5))
WAVE_SPPS = (257, 4096, 65535)
# (w, h, spp, max_bounce)
RENDER_CASES = ([(w, h, spp, 4) for w, h in SMALL_FRAMES for spp in SPPS] +
                [(w, h, spp, 4) for w, h in WAVE_FRAMES for spp in WAVE_SPPS] +
                [(1, 1, 65535, 0), (1, 1, 65535, 1)])
RENDER_MODES = {"default": (0, False), "lane_walk": (native.FLAG_LANE_WALK, False),
                "mt_exact": (native.FLAG_MT_EXACT, False), "counting": (0, True)}
SPLITS = (4096, 32768, 65534, 65535)                 # samples_per_pass of 3x3 x 65535
TWO_SETS = (13, 10, 65535, 4)                        # 130 pixels: 129 is the least that makes 2^23 samples
LAST_ONE = (64, 33, 4097, 4)                         # 5 passes of 1024: the last of one sample, lead 0
BIG = 1 << 23                                        # kSetsMinSamples (render.hip)

RAD_N = (1, 7, 9, 65)
RAD_CASES = [(n, spp, mb) for n in RAD_N for spp in (1, 17, 4096, 65535) for mb in (4, 1)
             if spp < 65535 or n in (1, 9)]
RAD_MODES = {"default": 0, "park": native.TRACE_PARK, "per_sample": native.RADIANCE_PER_SAMPLE,
             "per_sample_park": native.RADIANCE_PER_SAMPLE | native.TRACE_PARK, "lane_walk": native.FLAG_LANE_WALK}
WRAP = (7, 4096, 4, 2 ** 32 - 3)                     # n, spp, max_bounce, index_base: keys 2^32 - 3 .. 3


def _is_blend_textured(soup, m):
    """A BLEND material whose transparency comes from its texture's alpha (scenes.bake_materials)."""
    return m.alpha_mode == "BLEND" and m.base_texture is not None and soup.textures[m.base_texture].has_alpha


def _is_clamp_wrapped(soup, m):
    return any(soup.textures[t].wrap_s_clamp or soup.textures[t].wrap_t_clamp
               for t in (m.base_texture, m.emissive_texture) if t is not None)


class Tall:
    """A scene of the file, its oracle and reference objects, and every
    oracle result asked for so far (computed once, left unchanged)."""

    def __init__(self, orc, name):
        self.orc, self.name = orc, name
        if name == "cornell":
            self.soup, self.seed = scenes.get_scene("cornell"), 1     # (with 7 the one sample of 1x1 x 1 misses)
        else:
            self.soup, _, _, _, _, _, self.seed = fuzz_scenes.scene(FUZZ_SEED)
        self.oracle = orc.OracleScene(self.soup, RES)
        self.rad = radiance_ref.RadianceRef(orc, self.soup, RES)
        self.o, self.d = seed_rays(self.soup, FUZZ_SEED)
        self._frames, self._rad, self._ray_ref = {}, {}, None

    def ocam(self, w, h):
        c = self.soup.camera(None)
        return self.orc.camera_from_matrix(c.matrix, c.yfov, None, w, h)

    def frame(self, w, h, spp, mb):
        """(rgb (w * h, 3), linear bits (w * h, 3) uint32, counters) in row-major pixel order."""
        key = (w, h, spp, mb)
        if key not in self._frames:
            rgb, lin, ctr = self.oracle.render(self.ocam(w, h), spp, mb, self.orc.RNG_PATH, self.seed, THREADS)
            bits = lin.view(np.uint32).copy()
            for a in (rgb, bits, ctr):
                a.setflags(write=False)
            self._frames[key] = (rgb, bits, ctr)
        return self._frames[key]

    def radiance(self, n, spp, mb, index_base=0):
        """(linear bits (n, 3) uint32, rgb, counters) of the first n rays."""
        key = (n, spp, mb, index_base)
        if key not in self._rad:
            lin, rgb, ctr = self.rad.radiance(self.o[:n], self.d[:n], spp, mb, seed=self.seed, index_base=index_base)
            bits = lin.view(np.uint32).copy()
            for a in (rgb, bits, ctr):
                a.setflags(write=False)
            self._rad[key] = (bits, rgb, ctr)
        return self._rad[key]

    @property
    def ray_ref(self):
        if self._ray_ref is None:
            self._ray_ref = trace_ref.RayRef(self.orc, self.soup, RES)
        return self._ray_ref

    def first_hit_material(self, o, d):
        _, ref, _, _ = self.ray_ref.trace(o, d)
        return None if ref == trace_ref.MISS else self.soup.materials[int(self.soup.mat[self.ray_ref.indices[ref]])]


_TALL = {}


@pytest.fixture(scope="module")
def tall(oracle_mod):
    def get(name):
        if name not in _TALL:
            _TALL[name] = Tall(oracle_mod, name)
        return _TALL[name]
    return get


# ------------------------------------------------- the oracle alone (CPU)
def test_fuzz_scene_is_the_textured_one():
    """From the soup alone: FUZZ_SEED's materials include BLEND with a texture
    that has alpha, and a clamp-wrapped texture, each on some triangle."""
    soup = fuzz_scenes.scene(FUZZ_SEED)[0]
    used = [soup.materials[i] for i in np.unique(soup.mat)]
    assert any(_is_blend_textured(soup, m) for m in used)
    assert any(_is_clamp_wrapped(soup, m) for m in used)
    assert soup.num_triangles >= 400


def _scatters(ctr, samples, mb):
    """A case proves something only if paths hit geometry and go on: hits, and
    more segments than samples (at max_bounce 1 a sample has one segment)."""
    assert int(ctr[3]) > 0, "no hit"
    if mb > 1:
        assert int(ctr[0]) > samples, "no path went on after its first segment"
    else:
        assert int(ctr[0]) == samples * mb


@pytest.mark.parametrize("name", SCENES)
def test_tall_renders_hit_and_scatter(name, tall):
    """Every render case, on each scene: hits, and segments > samples; at 65535
    spp also more segments with max_bounce 4 than with 3 (a path reaches
    bounce 4).  On the textured scene the pixel centres of the 8x8 frame see
    the BLEND material first."""
    t = tall(name)
    for w, h, spp, mb in RENDER_CASES + [TWO_SETS, LAST_ONE]:
        if mb == 0:
            assert int(t.frame(w, h, spp, mb)[2][0]) == 0 and not t.frame(w, h, spp, mb)[1].any()
            continue
        _scatters(t.frame(w, h, spp, mb)[2], w * h * spp, mb)
    _, _, c3 = t.oracle.render(t.ocam(1, 1), 65535, 3, t.orc.RNG_PATH, t.seed, THREADS)
    assert int(t.frame(1, 1, 65535, 4)[2][0]) > int(c3[0])
    if name == "fuzz":
        cam = t.ocam(8, 8)
        org, llc, right, up = (np.array(list(v), np.float64) for v in (cam.origin, cam.llc, cam.right, cam.up))
        mats = [t.first_hit_material(org, llc + right * (x + 0.5) + up * (y + 0.5))
                for y in range(8) for x in range(8)]
        assert any(m is not None and _is_blend_textured(t.soup, m) for m in mats)


@pytest.mark.parametrize("name", SCENES)
def test_tall_rays_hit_and_scatter(name, tall):
    t = tall(name)
    for n, spp, mb in RAD_CASES:
        _scatters(t.radiance(n, spp, mb)[2], n * spp, mb)
    n, spp, mb, base = WRAP
    _scatters(t.radiance(n, spp, mb, base)[2], n * spp, mb)
    assert not np.array_equal(t.radiance(n, spp, mb, base)[0], t.radiance(n, spp, mb)[0])   # other keys, other streams
    if name == "fuzz":
        for n in RAD_N[1:]:
            mats = [t.first_hit_material(t.o[i], t.d[i]) for i in range(n)]
            assert any(m is not None and _is_blend_textured(t.soup, m) for m in mats), n


# ------------------------------------------------------------------- the GPU
@pytest.fixture(scope="module")
def context(tall):
    made = {}

    def get(name):
        if name not in made:
            made[name] = RenderScene(tall(name).soup, RES, device=0, device_build=name == "fuzz")
        return made[name]
    yield get
    for rs in made.values():
        rs.close()


def _render(t, rs, w, h, spp, mb, flags=0, stats=False, spp_pass=0):
    """One render compared with the oracle's frame; returns the call's stats."""
    rgb, bits, ctr = t.frame(w, h, spp, mb)
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(cam.w, cam.h)
    img, out = rs.render(cam, num_samples=spp, max_bounce=mb, seed=t.seed, stats=stats, linear=True, flags=flags,
                         samples_per_pass=spp_pass)
    what = (t.name, w, h, spp, mb, hex(flags), stats, spp_pass)
    assert np.array_equal(img.reshape(-1, 3), rgb), what
    assert np.array_equal(out["linear"].view(np.uint32), bits[pix]), what
    st = out["stats"]
    assert st["segments"] == int(ctr[0]) and st["samples"] == w * h * spp, what
    if stats:
        assert (st["cells_visited"], st["triangle_tests"], st["hits"]) == tuple(int(x) for x in ctr[1:4]), what
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp,mb", RENDER_CASES)
@pytest.mark.parametrize("name", SCENES)
def test_tall_render_matches_the_oracle(name, w, h, spp, mb, tall, context):
    t, rs = tall(name), context(name)
    for flags, stats in RENDER_MODES.values():
        st = _render(t, rs, w, h, spp, mb, flags, stats)
        assert st["trace_launches"] == (1 if stats else max(mb, 1))      # one pass


@pytest.mark.gpu
@pytest.mark.parametrize("spp_pass", SPLITS)
@pytest.mark.parametrize("name", SCENES)
def test_pass_splits_at_65535_equal_one_pass(name, spp_pass, tall, context):
    """s0 up to 65534, a last pass of one sample (65534): the single-pass image."""
    t, rs = tall(name), context(name)
    passes = -(-65535 // spp_pass)
    for flags, stats in RENDER_MODES.values():
        st = _render(t, rs, 3, 3, 65535, 4, flags, stats, spp_pass)
        assert st["trace_launches"] == passes * (1 if stats else 4)
        assert rs.context.profile()["passes"] == passes


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_two_pass_sets_with_a_lead_at_the_smallest_frame(name, tall, context):
    t, rs = tall(name), context(name)
    w, h, spp, mb = TWO_SETS
    assert w * h * spp >= BIG > (w * h - 2) * spp
    st = _render(t, rs, w, h, spp, mb)
    assert st["trace_launches"] == 2 * 4
    assert rs.context.profile()["sets"] == 2
    st = _render(t, rs, w, h, spp, mb, native.FLAG_ONE_SET)
    assert st["trace_launches"] == 2 * 4 and rs.context.profile()["sets"] == 1
    st = _render(t, rs, w, h, spp, mb, spp_pass=1000)          # 66 passes on two sets, lead 200, last pass 535
    assert st["trace_launches"] == 66 * 4
    assert rs.context.profile()["passes"] == 66 and rs.context.profile()["sets"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_a_last_pass_of_one_sample_takes_no_lead(name, tall, context):
    t, rs = tall(name), context(name)
    w, h, spp, mb = LAST_ONE
    assert w * h * spp >= BIG and spp == 4 * 1024 + 1
    st = _render(t, rs, w, h, spp, mb, spp_pass=1024)
    assert st["trace_launches"] == 5 * 4 and rs.context.profile()["passes"] == 5
    st = _render(t, rs, w, h, spp, mb, spp_pass=spp)
    assert st["trace_launches"] == 4 and rs.context.profile()["passes"] == 1


def _radiance(t, rs, n, spp, mb, flags, index_base=0):
    bits, rgb, ctr = t.radiance(n, spp, mb, index_base)
    res = rs.radiance(t.o[:n], t.d[:n], spp, mb, seed=t.seed, index_base=index_base, flags=flags, rgb=True)
    what = (t.name, n, spp, mb, hex(flags), index_base)
    assert np.array_equal(res["radiance"].view(np.uint32), bits), what
    assert np.array_equal(res["rgb"], rgb), what
    assert res["stats"]["segments"] == int(ctr[0]) and res["stats"]["samples"] == n * spp, what


@pytest.mark.gpu
@pytest.mark.parametrize("n,spp,mb", RAD_CASES)
@pytest.mark.parametrize("name", SCENES)
def test_tall_radiance_matches_the_reference(name, n, spp, mb, tall, context):
    t, rs = tall(name), context(name)
    for flags in RAD_MODES.values():
        _radiance(t, rs, n, spp, mb, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_tall_radiance_with_wrapping_stream_keys(name, tall, context):
    t, rs = tall(name), context(name)
    n, spp, mb, base = WRAP
    for flags in RAD_MODES.values():
        _radiance(t, rs, n, spp, mb, flags, base)
