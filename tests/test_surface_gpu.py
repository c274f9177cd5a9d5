"""Surface queries on the GPU (zrt_context_surface, Context.surface) against
the per-ray reference (surface_ref.py: the trace reference's hit, then
stage3.zig:199-206 in numpy float32 and the oracle's Texture.sample), bit for
bit: all 16 words of every record as uint32 patterns; a miss is exactly
fifteen zero words and material = 0xFFFFFFFF.  Where a test asks for them, the
hit records are compared with the trace reference too.

The fuzz scenes (test_query_fuzz_gpu.py's seeds, rays and contexts: host-built
for even seeds, device-built for odd ones) bring real textures, clamp and
repeat wrap, uvs outside [0, 1], MASK and BLEND transparency and emissive
textures (counted in test_surface_host.py); the fixed query scenes
(test_trace_gpu.CASES) have 1x1 materials only, whose texels ride in the
material descriptor.  A case's reference is computed once and shared.
"""
import dataclasses

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import fuzz_scenes
import radiance_ref
import surface_ref
import test_query_fuzz_gpu as qf
import test_trace_gpu as ttg
import trace_ref
from surface_ref import MISS_WORDS, surface_bits
from test_surface_host import HAND_D, HAND_O, HAND_WANT, hand_soup

pytestmark = pytest.mark.gpu

MISS = native.MISS
FUZZ_MODES = {"lane": 0, "park": native.TRACE_PARK, "park_bfcull": native.TRACE_PARK | native.FLAG_BFCULL,
              "mt_exact": native.FLAG_MT_EXACT}
PATHS = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}


def _check(got, want, what):
    got = np.asarray(got)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rays differ, first {bad[0]}: got "
                           f"{[hex(int(x)) for x in got[bad[0]]]}, reference {[hex(int(x)) for x in want[bad[0]]]}")


def _check_result(res, words, bits, what):
    """A numpy result with hits=True against both references, and its misses' exact form."""
    got = surface_bits(res)
    _check(got, words, what)
    _check(trace_ref.hit_bits(res), bits, what + " hits")
    miss = res["triangle"] == MISS
    assert (got[miss] == MISS_WORDS).all() and (got[~miss, 3] != MISS).all(), what
    assert res["stats"]["segments"] == len(words) and res["stats"]["samples"] == 0, what


# ------------------------------------------------------------ the fuzz scenes
@pytest.fixture(scope="module")
def fuzz_case(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed]
    return get


@pytest.fixture(scope="module")
def fuzz_context(fuzz_case):
    """The seed's context; one at a time."""
    made = {}

    def get(seed):
        if seed not in made:
            for rs in made.values():
                rs.close()
            made.clear()
            cs = fuzz_case(seed)
            made[seed] = RenderScene(cs.soup, cs.res, device=0, device_build=cs.device_build)
        return made[seed]
    yield get
    for rs in made.values():
        rs.close()


@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_surfaces_match_the_reference(seed, fuzz_case, fuzz_context):
    cs, rs = fuzz_case(seed), fuzz_context(seed)
    words = surface_ref.cached_batch(cs)
    what = f"seed {seed}, {cs.soup.num_triangles} triangles, grid {cs.res}"
    for mode, flags in FUZZ_MODES.items():
        res = rs.surface(cs.o, cs.d, flags=flags, hits=True)
        _check_result(res, words, cs.bits, f"{what}, {mode}")
        if not cs.device_build:
            hit = res["triangle"] != MISS
            assert np.array_equal(res["source_triangle"][hit], cs.ref.indices[res["triangle"][hit]])
            assert (res["source_triangle"][~hit] == MISS).all()
    res = rs.surface(cs.o, cs.d, stats=True, hits=True)
    _check_result(res, words, cs.bits, f"{what}, counting")
    st = res["stats"]
    assert (st["segments"], st["cells_visited"], st["triangle_tests"], st["hits"]) == (qf.N_RAYS,) + cs.counts, what
    _check(surface_bits(rs.surface(cs.o, cs.d)), words, f"{what}, without hits")


# ----------------------------------------------------- the fixed query scenes
@pytest.fixture(scope="module")
def case(oracle_mod):
    def get(name):
        if name not in ttg._CASES:                 # test_trace_gpu's cases, computed once for both modules
            mk, res = ttg.CASES[name]
            soup = mk()
            ref = trace_ref.RayRef(oracle_mod, soup, res)
            o, d = ttg._case_rays(ref, soup, sorted(ttg.CASES).index(name) + 1)
            bits, counts = ref.trace_batch(o, d)
            bits.setflags(write=False)
            ttg._CASES[name] = ttg.Case(soup, res, ref, o, d, bits, counts)
        return ttg._CASES[name]
    return get


@pytest.fixture(scope="module")
def scene(case):
    """The context of (case, build), made once."""
    made = {}

    def get(name, build="host"):
        if (name, build) not in made:
            cs = case(name)
            made[(name, build)] = RenderScene(cs.soup, cs.res, device=0, device_build=build == "device")
        return made[(name, build)]
    yield get
    for rs in made.values():
        rs.close()


@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(ttg.CASES))
def test_fixed_scenes_match_the_reference(name, path, build, case, scene):
    cs, rs = case(name), scene(name, build)
    words = surface_ref.cached_batch(cs)
    res = rs.surface(cs.o, cs.d, flags=PATHS[path], hits=True)
    _check_result(res, words, cs.bits, f"{name} {path} {build}")
    assert (words[:, 3] == MISS).any() and (words[:, 3] != MISS).any(), "the case covers hits and misses"
    # one chunk: the trace call's launches (ttg.test_hits_match_the_reference) and the gather
    want = 5 if path == "park" and name in ttg.PARK_RUNS else 3 if path == "lane" else None
    if want is not None:
        assert res["stats"]["trace_launches"] == want


def test_hand_derived_surface_on_the_gpu():
    soup = hand_soup()
    for build in (False, True):
        rs = RenderScene(soup, (2, 2, 2), device=0, device_build=build)
        for flags in (0, native.TRACE_PARK, native.FLAG_MT_EXACT):
            res = rs.surface(np.float32([HAND_O, [0, 0, -2]]), np.float32([HAND_D, [0, 0, 1]]), flags=flags)
            got = surface_bits(res)
            assert [hex(int(x)) for x in got[0]] == [hex(int(x)) for x in HAND_WANT], (build, flags)
            assert np.array_equal(got[1], MISS_WORDS)
        rs.close()


# ------------------------------------------------- both sides of the LDS copy
N_MANY = 2048              # the rays pile up on the soup's large triangles: about 100 distinct ones are hit


@pytest.mark.parametrize("nmat,build", [(64, "host"), (65, "device")])
def test_many_materials_on_both_sides_of_the_lds_limit(nmat, build, oracle_mod):
    """Fuzz seed 10's soup (400 triangles, three textures, a BLEND material
    with a base and an emissive texture) with its four materials repeated to
    `nmat` under other factors, and every triangle's material redrawn: the
    shade kernels copy at most 64 materials to LDS, so 64 and 65 are the two
    sides of whatever a kernel does with that limit."""
    soup, res = fuzz_scenes.scene(10)[:2]
    rng = np.random.default_rng(6400 + nmat)
    mats = list(soup.materials)
    while len(mats) < nmat:
        m = mats[len(mats) % len(soup.materials)]
        mats.append(dataclasses.replace(m, base_color=tuple(float(x) for x in rng.random(4)),
                                        emissive=tuple(float(x) for x in rng.random(3) * (2.0 if any(m.emissive) else 0.0))))
    mat = rng.integers(0, nmat, soup.num_triangles).astype(np.uint32)
    mat[::7] = nmat - 1                                        # the last material is surely there
    many = scenes.SceneSoup(f"many{nmat}", soup.pos, soup.nrm, soup.uv, mat, mats, soup.textures,
                            soup.cameras).bake_materials()
    rays = [qf.seed_rays(many, s) for s in range(N_MANY // qf.N_RAYS)]
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    ref = trace_ref.RayRef(oracle_mod, many, res)
    bits, _ = ref.trace_batch(o, d)
    words = surface_ref.surface_batch(ref, many, o, d, bits)
    seen = set(int(x) for x in words[words[:, 3] != MISS, 3])
    assert len(seen) >= 32 and nmat - 1 in seen and max(seen) == nmat - 1, sorted(seen)
    rs = RenderScene(many, res, device=0, device_build=build == "device")
    for path, flags in PATHS.items():
        _check_result(rs.surface(o, d, flags=flags, hits=True), words, bits, f"{nmat} materials {path}")
    rs.close()


# ------------------------------------------------------------------ the calls
GUARD = 2


@pytest.mark.parametrize("with_hits", [False, True])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_and_the_records_beside_the_outputs(n, path, with_hits, case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    pick = np.random.default_rng(7).permutation(n) % ttg.N_RAYS
    rays = np.ascontiguousarray(np.concatenate([cs.o[pick], cs.d[pick]], axis=1))
    surf = np.full((n + 2 * GUARD, 16), 0xABABABAB, np.uint32)
    hits = np.full((n + 2 * GUARD, 4), 0xCDCDCDCD, np.uint32)
    st = rs.context.surface_raw(n, rays.ctypes.data, surf[GUARD:].ctypes.data,
                                hits[GUARD:].ctypes.data if with_hits else None, False, PATHS[path])
    assert (surf[:GUARD] == 0xABABABAB).all() and (surf[GUARD + n:] == 0xABABABAB).all(), "guard records"
    _check(surf[GUARD:GUARD + n], surface_ref.cached_batch(cs)[pick], f"n = {n} {path}")
    if with_hits:
        assert (hits[:GUARD] == 0xCDCDCDCD).all() and (hits[GUARD + n:] == 0xCDCDCDCD).all(), "guard hit records"
        _check(hits[GUARD:GUARD + n], cs.bits[pick], f"n = {n} {path} hits")
    else:
        assert (hits == 0xCDCDCDCD).all()
    assert st["segments"] == n and st["trace_launches"] == (5 if path == "park" else 3)


def test_a_batch_across_the_chunk_cut(case, scene):
    """2^20 + 77 rays: two chunks, the second of 77 rays; the park path's
    records are the lane walk's, and the rays around the cut are the
    reference's."""
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    words = surface_ref.cached_batch(cs)
    n, cut = (1 << 20) + 77, 1 << 20
    o, d = ttg._random_batch(cs, n, 11)
    hit, miss = np.nonzero(words[:, 3] != MISS)[0], np.nonzero(words[:, 3] == MISS)[0]
    pick = np.concatenate([hit[:3], miss[:2], hit[3:5], miss[2:4]])           # nine rays, both kinds on both sides
    pos = np.arange(cut - 4, cut + 5)
    o[pos], d[pos] = cs.o[pick], cs.d[pick]
    lane = rs.surface(o, d, flags=native.FLAG_LANE_WALK, hits=True)
    park = rs.surface(o, d, flags=native.TRACE_PARK, hits=True)
    assert (lane["stats"]["trace_launches"], park["stats"]["trace_launches"]) == (6, 10)
    lw = surface_bits(lane)
    assert np.array_equal(lw, surface_bits(park))
    assert np.array_equal(trace_ref.hit_bits(lane), trace_ref.hit_bits(park))
    _check(lw[pos], words[pick], "the rays around the cut")
    _check(trace_ref.hit_bits(lane)[pos], cs.bits[pick], "the hits around the cut")
    missed = lane["triangle"] == MISS
    assert missed.any() and (~missed).any() and (lw[missed] == MISS_WORDS).all() and (lw[~missed, 3] != MISS).all()


def test_one_context_serves_every_call_in_turn(case, scene, oracle_mod):
    """surface, render, trace, segments, radiance, surface on one context:
    the two surface results are equal and every other call matches its own
    reference."""
    cs = case("cornell_bm")
    cam = camera_for(cs.soup, None, 24, 24)
    fresh = RenderScene(cs.soup, cs.res, device=0)
    want_img, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    rad = radiance_ref.RadianceRef(oracle_mod, cs.soup, cs.res)
    want_lin, _, _ = rad.radiance(cs.o[:32], cs.d[:32], 2, 3, seed=5)
    words = surface_ref.cached_batch(cs)
    rs = scene("cornell_bm")
    for flags in (0, native.TRACE_PARK):
        first = rs.surface(cs.o, cs.d, flags=flags, hits=True)
        img, _ = rs.render(cam, num_samples=2, max_bounce=4)
        assert np.array_equal(img, want_img)
        _check(trace_ref.hit_bits(rs.trace(cs.o, cs.d, flags=flags)), cs.bits, "trace after surface")
        seg = rs.segments(cs.o, cs.d, np.inf, flags=flags)
        _check(trace_ref.hit_bits(seg), cs.bits, "segments after surface")
        got = rs.radiance(cs.o[:32], cs.d[:32], 2, 3, seed=5, flags=flags)
        assert np.array_equal(got["radiance"].view(np.uint32), want_lin.view(np.uint32))
        last = rs.surface(cs.o, cs.d, flags=flags, hits=True)
        _check_result(first, words, cs.bits, "the first surface call")
        assert np.array_equal(surface_bits(first), surface_bits(last))
        assert np.array_equal(trace_ref.hit_bits(first), trace_ref.hit_bits(last))


def test_empty_batch_touches_nothing(scene):
    ctx = scene("cornell_bm").context
    surf = np.full(32, 0xABABABAB, np.uint32)
    hits = np.full(8, 0xCDCDCDCD, np.uint32)
    rays = np.zeros(6, np.float32)
    for flags in (0, native.TRACE_PARK, native.FLAG_COUNT_STATS):
        st = ctx.surface_raw(0, rays.ctypes.data, surf.ctypes.data, hits.ctypes.data, False, flags)
        assert st["segments"] == 0 and st["hits"] == 0 and st["trace_launches"] == 0
    ctx.surface_raw(0, None, None, None, False, 0)
    assert (surf == 0xABABABAB).all() and (hits == 0xCDCDCDCD).all()
    z = np.zeros((0, 3), np.float32)
    res = ctx.surface(z, z, hits=True)
    assert res["position"].shape == (0, 3) and res["material"].shape == (0,) and res["triangle"].shape == (0,)


def test_bad_batches_raise_on_a_live_context(case, scene):
    cs, ctx = case("cornell_bm"), scene("cornell_bm").context
    rays = np.ascontiguousarray(np.concatenate([cs.o[0], cs.d[0]]))
    surf, hits = np.zeros(16, np.uint32), np.zeros(4, np.uint32)
    r, s, h = rays.ctypes.data, surf.ctypes.data, hits.ctypes.data
    for args in ((None, s, h, False, 0), (r, None, h, False, 0), (r, s, h, False, 0x4),
                 (r, s, h, False, native.FLAG_ONE_SET), (r, s, h, False, native.SEGMENT_ANY),
                 (r, s, h, False, native.RADIANCE_PER_SAMPLE), (r, s, h, False, 0x80000)):
        with pytest.raises(native.ZrtError) as e:
            ctx.surface_raw(1, *args)
        assert e.value.status == -1
    assert not surf.any() and not hits.any()
    ctx.surface_raw(1, r, s, h, False, 0)                      # the control: the valid batch runs
    assert np.array_equal(surf, surface_ref.cached_batch(cs)[0]) and np.array_equal(hits, cs.bits[0])


def _device(case, scene):
    if torch is None or not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    return case("cornell_bm"), scene("cornell_bm"), torch.device("cuda", 0)


def test_torch_tensors_are_filled_in_place(case, scene):
    cs, rs, dev = _device(case, scene)
    pick = np.random.default_rng(7).permutation(ttg.N_RAYS)[:200]
    words = surface_ref.cached_batch(cs)[pick]
    before = torch.arange(4096, dtype=torch.int32, device=dev)
    o, d = torch.from_numpy(cs.o[pick]).to(dev), torch.from_numpy(cs.d[pick]).to(dev)
    for mode, flags in (("lane", 0), ("park", native.TRACE_PARK), ("mt_exact", native.FLAG_MT_EXACT)):
        host = rs.surface(cs.o[pick], cs.d[pick], flags=flags, hits=True)
        for with_hits in (False, True):        # without: the hit records stay in the context
            res = rs.surface(o, d, flags=flags, hits=with_hits)
            after = torch.full((4096,), 5, dtype=torch.int32, device=dev)
            surf = res["surfaces"]
            assert surf.shape == (200, 16) and surf.dtype == torch.float32 and surf.device == dev
            got = surf.cpu().numpy().view(np.uint32)
            _check(got, surface_bits(host), f"torch {mode} vs the numpy path")
            _check(got, words, f"torch {mode} vs the reference")
            mat_i32 = surf[:, 3].view(torch.int32).cpu().numpy()          # as Context.surface documents
            assert np.array_equal(mat_i32.view(np.uint32), words[:, 3])
            assert ("hits" in res) == with_hits
            if with_hits:
                _check(res["hits"].cpu().numpy().view(np.uint32), cs.bits[pick], f"torch {mode} hits")
            assert torch.equal(before.cpu(), torch.arange(4096, dtype=torch.int32)) and bool((after == 5).all())
            assert res["stats"]["segments"] == 200


def test_a_misaligned_device_pointer_is_refused(case, scene):
    cs, rs, dev = _device(case, scene)
    o, d = torch.from_numpy(cs.o[:8]).to(dev), torch.from_numpy(cs.d[:8]).to(dev)
    rays = torch.cat([o, d], dim=1).contiguous()
    buf = torch.full((8 * 16 + 4,), -1.0, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    for off in (4, 8, 12):
        with pytest.raises(native.ZrtError) as e:
            rs.context.surface_raw(8, rays.data_ptr(), buf.data_ptr() + off, None, True, 0)
        assert e.value.status == -1
    assert bool((buf == -1.0).all())
    rs.context.surface_raw(8, rays.data_ptr(), buf.data_ptr(), None, True, 0)          # the control
    _check(buf[:128].cpu().numpy().view(np.uint32).reshape(8, 16), surface_ref.cached_batch(cs)[:8], "aligned")
    # device hit records need only their own 4-byte alignment
    hits = torch.zeros((8 * 4 + 1,), dtype=torch.float32, device=dev)
    rs.context.surface_raw(8, rays.data_ptr(), buf.data_ptr(), hits.data_ptr() + 4, True, 0)
    _check(hits[1:].cpu().numpy().view(np.uint32).reshape(8, 4), cs.bits[:8], "hit records at a 4-byte offset")
    _check(buf[:128].cpu().numpy().view(np.uint32).reshape(8, 16), surface_ref.cached_batch(cs)[:8], "beside them")
