"""Occlusion queries (zrt_context_occlusion) on the GPU, bit for bit --
`occluded`, the bits of `visibility` and the first hits -- against two
references:

  the CPU reference (occlusion_ref.py) on the fuzz seeds' rays;
  the device composition a caller would run without the call: Context.surface,
  numpy float32 directions from oracle.path_norm in the contract's order,
  Context.segments(any_hit=True) over exactly the traced samples, summed in
  numpy.  It needs no CPU walk, so it covers every ray and the large shapes.

Every compared call also has to report segments = rays + traced samples and
hits = the sum of `occluded`.
"""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import occlusion_ref
import test_occlusion_host as toh
import test_query_fuzz_gpu as qf
import trace_ref

pytestmark = pytest.mark.gpu

F = np.float32
ONE = 0x3F800000
MODES = {"default": 0, "lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK,
         "park_bfcull": native.TRACE_PARK | native.FLAG_BFCULL, "mt_exact": native.FLAG_MT_EXACT}
PATHS = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}
RADIUS_SEEDS = [4, 12, 18, 31]


@pytest.fixture(scope="module")
def case(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed]
    return get


@pytest.fixture(scope="module")
def context(case):
    """The seed's context; one at a time."""
    made = {}

    def get(seed):
        if seed not in made:
            for rs in made.values():
                rs.close()
            made.clear()
            cs = case(seed)
            made[seed] = RenderScene(cs.soup, cs.res, device=0, device_build=cs.device_build)
        return made[seed]
    yield get
    for rs in made.values():
        rs.close()


# ------------------------------------------------------------ the composition
_DRAWS = {}


def draws(orc, seed, key0, n, S):
    """(n, S, 3) float32: the first three floatNorm draws of the streams
    (seed, (key0 + i) mod 2^32, s); computed once per argument set."""
    k = (int(seed), int(key0), int(n), int(S))
    if k not in _DRAWS:
        out = np.zeros((n, S, 3), np.float32)
        fn, sd = orc.lib().orc_path_norm, int(seed) & 0xFFFFFFFFFFFFFFFF
        for i in range(n):
            key, row = (int(key0) + i) & 0xFFFFFFFF, out[i]
            for s in range(S):
                fn(sd, key, s, row[s], 3)
        out.setflags(write=False)
        _DRAWS[k] = out
    return _DRAWS[k]


def vnormalize(x):
    """occlusion_ref.normalize over the last axis of a float32 array."""
    with np.errstate(all="ignore"):
        n2 = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]
        inv = F(1.0) / np.sqrt(n2)
        return (x * inv[..., None]).astype(F)


def composition(orc, rs, o, d, S, radius, seed=0, key0=0, counting=False):
    """{"occluded", "visibility" (bits), "hits" (bits), "traced", "counts"}:
    what a caller composes from Context.surface and Context.segments."""
    n = len(o)
    surf = rs.surface(o, d, hits=True, stats=counting)
    hit = surf["material"] != native.MISS
    pos = np.ascontiguousarray(np.broadcast_to(surf["position"][hit][:, None, :], (int(hit.sum()), S, 3)))
    with np.errstate(all="ignore"):
        ds = vnormalize((surf["normal"][hit][:, None, :] + vnormalize(draws(orc, seed, key0, n, S)[hit])).astype(F))
    traced = np.isfinite(pos).all(-1) & np.isfinite(ds).all(-1) & (ds != 0).any(-1)
    rad = radius if np.ndim(radius) == 0 else \
        np.ascontiguousarray(np.broadcast_to(np.asarray(radius, F)[hit][:, None], traced.shape)[traced])
    seg = rs.segments(np.ascontiguousarray(pos[traced]), np.ascontiguousarray(ds[traced]), rad, any_hit=True,
                      stats=counting)
    items = np.zeros(traced.shape, bool)
    items[traced] = seg["occluded"]
    occ = np.zeros(n, np.uint32)
    occ[hit] = items.sum(1)
    counts = None
    if counting:
        counts = tuple(surf["stats"][k] + seg["stats"][k] for k in ("cells_visited", "triangle_tests"))
    return {"occluded": occ, "visibility": occlusion_ref.visibility(occ, S).view(np.uint32),
            "hits": trace_ref.hit_bits(surf), "traced": int(traced.sum()), "counts": counts}


def call(rs, o, d, S, radius, seed=0, key0=0, flags=0, device=False, stats=False):
    """Context.occlusion with host arrays or, `device`, torch tensors, as
    (occluded uint32, visibility bits, hit bits, stats)."""
    if device:
        dev = torch.device("cuda", 0)
        rad = radius if np.ndim(radius) == 0 else torch.from_numpy(np.ascontiguousarray(radius, F)).to(dev)
        res = rs.occlusion(torch.from_numpy(np.ascontiguousarray(o)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(d)).to(dev), S, rad, seed=seed, index_base=key0,
                           flags=flags, stats=stats, hits=True)
        return (res["occluded"].cpu().numpy().astype(np.uint32), res["visibility"].cpu().numpy().view(np.uint32),
                res["hits"].cpu().numpy().view(np.uint32), res["stats"])
    res = rs.occlusion(o, d, S, radius, seed=seed, index_base=key0, flags=flags, stats=stats, hits=True)
    return res["occluded"], res["visibility"].view(np.uint32), trace_ref.hit_bits(res), res["stats"]


def check(got, want_occ, want_vis, want_hits, traced, what):
    occ, vis, hits, st = got
    bad = np.nonzero((occ != want_occ) | (vis != want_vis) | (hits != want_hits).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rays differ, first {bad[0]}: got occluded {int(occ[bad[0]])} visibility "
                           f"{hex(int(vis[bad[0]]))} hit {[hex(int(x)) for x in hits[bad[0]]]}, reference "
                           f"{int(want_occ[bad[0]])} {hex(int(want_vis[bad[0]]))} "
                           f"{[hex(int(x)) for x in want_hits[bad[0]]]}")
    assert (st["segments"], st["hits"], st["samples"]) == (len(occ) + traced, int(want_occ.astype(np.int64).sum()), 0), \
        (what, st, traced)


def use_device(seed):
    """Host and device pointers alternate by seed pair."""
    return torch is not None and torch.cuda.is_available() and (seed // 2) % 2 == 1


# ------------------------------------------------------------------ the seeds
@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_occlusion_matches_both_references(seed, case, context, oracle_mod):
    cs, rs = case(seed), context(seed)
    smp = occlusion_ref.cached_samples(cs)
    radius = occlusion_ref.fuzz_radius(cs.soup)
    dev = use_device(seed)
    for S in (1, 3, 5):
        occ, vis, traced, counts = occlusion_ref.occlusion_batch(cs.ref, smp, radius, S, counts=True)
        comp = composition(oracle_mod, rs, cs.o, cs.d, S, radius, seed=cs.rseed, counting=True)
        what = f"seed {seed}, {cs.soup.num_triangles} triangles, grid {cs.res}, S {S}"
        assert np.array_equal(comp["occluded"], occ) and np.array_equal(comp["visibility"], vis), what + ": composition"
        assert np.array_equal(comp["hits"], cs.bits) and comp["traced"] == traced, what + ": composition"
        for mode, flags in MODES.items():
            check(call(rs, cs.o, cs.d, S, radius, seed=cs.rseed, flags=flags, device=dev), occ, vis, cs.bits, traced,
                  f"{what}, {mode}")
        got = call(rs, cs.o, cs.d, S, radius, seed=cs.rseed, device=dev, stats=True)
        check(got, occ, vis, cs.bits, traced, f"{what}, counting")
        st = got[3]
        want = (cs.counts[0] + counts[0], cs.counts[1] + counts[1])
        assert (st["cells_visited"], st["triangle_tests"]) == want == comp["counts"], (what, st, want, comp["counts"])


# -------------------------------------------------------------------- radii
@pytest.mark.parametrize("seed", RADIUS_SEEDS)
def test_radii_follow_the_t_max_rules(seed, case, context, oracle_mod):
    cs, rs = case(seed), context(seed)
    smp = occlusion_ref.cached_samples(cs)
    n = len(cs.o)
    diag = occlusion_ref.fuzz_radius(cs.soup)
    special = [F(np.inf), F(0), F(-1), F(-np.inf), F(np.nan)]
    per_ray = np.array([([diag] + special)[i % 6] for i in range(n)], F)
    for radius in special + [per_ray]:
        occ, vis, traced, _ = occlusion_ref.occlusion_batch(cs.ref, smp, radius, 3)
        name = "per ray" if np.ndim(radius) else float(radius)
        if np.ndim(radius) == 0 and not radius > 0:
            assert not occ.any() and (vis == ONE).all() and traced > 0      # never occluded, traced all the same
        comp = composition(oracle_mod, rs, cs.o, cs.d, 3, radius, seed=cs.rseed)
        assert np.array_equal(comp["occluded"], occ) and comp["traced"] == traced, (seed, name)
        for path, flags in PATHS.items():
            for dev in (False, use_device(2)):
                check(call(rs, cs.o, cs.d, 3, radius, seed=cs.rseed, flags=flags, device=dev), occ, vis, cs.bits, traced,
                      f"seed {seed}, radius {name}, {path}, device {dev}")
    assert occlusion_ref.occlusion_batch(cs.ref, smp, F(np.inf), 3)[0].any()


@pytest.mark.parametrize("seed", RADIUS_SEEDS)
def test_a_radius_equal_to_a_samples_t_is_not_a_hit_the_next_float_is(seed, case, context):
    """S = 1, so a ray's radius belongs to one sample: the reference's
    closest-mode t of that sample under +inf, and nextafter(t, +inf)."""
    cs, rs = case(seed), context(seed)
    smp = occlusion_ref.cached_samples(cs)
    n = len(cs.o)
    at = np.full(n, np.inf, F)
    for i, x in enumerate(smp):
        if x and x[0].occluded(cs.ref, np.inf):
            at[i] = x[0].closest(cs.ref, np.inf)[0][0]
    edge = np.isfinite(at)
    assert edge.sum() >= 8, f"seed {seed}: only {edge.sum()} first samples are occluded"
    traced = sum(1 for x in smp if x and x[0].traced)
    for radius, want in ((at, np.zeros(n, np.uint32)), (np.nextafter(at, F(np.inf)), edge.astype(np.uint32))):
        occ, vis, tr, _ = occlusion_ref.occlusion_batch(cs.ref, smp, radius, 1)
        assert np.array_equal(occ, want) and tr == traced
        for path, flags in PATHS.items():
            check(call(rs, cs.o, cs.d, 1, radius, seed=cs.rseed, flags=flags), occ, vis, cs.bits, traced,
                  f"seed {seed}, edge radii, {path}")


# ------------------------------------------------------------------- streams
@pytest.mark.parametrize("rseed", [3, 0x9E3779B97F4A7C15])
def test_index_base_and_the_key_wrap(rseed, case, context, oracle_mod):
    cs, rs = case(RADIUS_SEEDS[2]), context(RADIUS_SEEDS[2])
    pick = np.nonzero(cs.bits[:, 3] != native.MISS)[0][:8]
    assert len(pick) == 8
    o, d = cs.o[pick], cs.d[pick]
    radius = occlusion_ref.fuzz_radius(cs.soup)
    seen = []
    for base in (1000, 2 ** 32 - 3):
        smp = [occlusion_ref.ray_samples(cs.ref, cs.soup, o[i], d[i], cs.bits[pick[i]], rseed, (base + i) & 0xFFFFFFFF, 5)
               for i in range(8)]
        occ, vis, traced, _ = occlusion_ref.occlusion_batch(cs.ref, smp, radius, 5)
        comp = composition(oracle_mod, rs, o, d, 5, radius, seed=rseed, key0=base)
        assert np.array_equal(comp["occluded"], occ)
        for path, flags in PATHS.items():
            check(call(rs, o, d, 5, radius, seed=rseed, key0=base, flags=flags), occ, vis, cs.bits[pick], traced,
                  f"seed {hex(rseed)}, index_base {base}, {path}")
        seen.append(tuple(occ))
    # rays 3.. of the second base have keys 0..: the same streams as index_base = 0 gives rays 0..
    smp0 = [occlusion_ref.ray_samples(cs.ref, cs.soup, o[i], d[i], cs.bits[pick[i]], rseed, i - 3, 5) for i in range(3, 8)]
    assert tuple(occlusion_ref.occlusion_batch(cs.ref, smp0, radius, 5)[0]) == seen[1][3:]


# ------------------------------------------------ shapes, on the Cornell box
@pytest.fixture(scope="module")
def cornell():
    soup = scenes.get_scene("cornell")
    rs = RenderScene(soup, (16, 16, 16), device=0)
    yield soup, rs
    rs.close()


def box_rays(soup, n, seed, inside=0.75):
    """n rays from inside the soup's box (`inside` of them; the others from around it), unit directions."""
    rng = np.random.default_rng(seed)
    p = np.asarray(soup.pos, np.float64).reshape(-1, 3)
    lo, ext = p.min(0), p.max(0) - p.min(0)
    u = rng.random((n, 3))
    wide = rng.random(n) >= inside
    o = lo + np.where(wide[:, None], u * 1.6 - 0.3, 0.05 + 0.9 * u) * ext
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)


def guarded_call(rs, o, d, S, radius_all, flags, want_vis=True, want_occ=True, want_hits=True, seed=0):
    """occlusion_raw on host arrays between guard words; (occluded, visibility bits, hit bits, stats), None for an
    output that was not asked for."""
    n = len(o)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    vis = np.full(n + 2, 0xABABABAB, np.uint32)
    occ = np.full(n + 2, 0xCDCDCDCD, np.uint32)
    hit = np.full(4 * (n + 2), 0xEFEFEFEF, np.uint32)
    st = rs.context.occlusion_raw(n, rays.ctypes.data, None, vis[1:].ctypes.data if want_vis else None,
                                  occ[1:].ctypes.data if want_occ else None, hit[4:].ctypes.data if want_hits else None,
                                  False, S, radius_all, seed, 0, flags)
    assert vis[0] == vis[-1] == 0xABABABAB and occ[0] == occ[-1] == 0xCDCDCDCD, "guard words"
    assert (hit[:4] == 0xEFEFEFEF).all() and (hit[-4:] == 0xEFEFEFEF).all(), "guard words"
    if not want_vis:
        assert (vis == 0xABABABAB).all()
    if not want_occ:
        assert (occ == 0xCDCDCDCD).all()
    if not want_hits:
        assert (hit == 0xEFEFEFEF).all()
    return (occ[1:-1] if want_occ else None, vis[1:-1] if want_vis else None,
            hit[4:-4].reshape(n, 4) if want_hits else None, st)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_ray_and_sample_counts_between_guard_words(n, cornell, oracle_mod):
    soup, rs = cornell
    o, d = box_rays(soup, n, 100 + n)
    for S in (1, 2, 63, 64, 65):
        comp = composition(oracle_mod, rs, o, d, S, 0.25, seed=7)
        if n >= 63:
            assert 0 < comp["occluded"].sum() < comp["traced"]
        for path, flags in PATHS.items():
            check(guarded_call(rs, o, d, S, 0.25, flags, seed=7), comp["occluded"], comp["visibility"], comp["hits"],
                  comp["traced"], f"n = {n}, S = {S}, {path}")


def test_a_ray_whose_samples_straddle_the_sub_chunk_cut(cornell, oracle_mod):
    """4099 rays x 257 samples = 1,053,443 items: one cut at item 2^20, inside ray 4080."""
    soup, rs = cornell
    n, S = 4099, 257
    assert (1 << 20) // S == 4080 and (1 << 20) % S != 0 and n * S > 1 << 20
    o, d = box_rays(soup, n, 5)
    # straight down onto the floor, half a unit from two walls: the CPU reference counts 94 of its 257 samples
    # occluded within a radius of 1
    o[4080], d[4080] = (0.5, 2.5, -4.5), (0, -1, 0)
    comp = composition(oracle_mod, rs, o, d, S, 1.0, seed=9)
    assert comp["occluded"][4080] == 94, "the straddling ray is partly occluded"
    for path, flags in list(PATHS.items()) + [("unasked", 0)]:
        check(call(rs, o, d, S, 1.0, seed=9, flags=flags), comp["occluded"], comp["visibility"], comp["hits"],
              comp["traced"], f"4099 x 257, {path}")


def test_torch_tensors_in_place_across_the_ray_chunk_cut(cornell, oracle_mod):
    """2^20 + 77 rays at S = 1 on the device: two chunks of rays."""
    if torch is None or not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    soup, rs = cornell
    n = (1 << 20) + 77
    o, d = box_rays(soup, n, 6)
    comp = composition(oracle_mod, rs, o, d, 1, 0.25, seed=2)
    dev = torch.device("cuda", 0)
    before = torch.arange(4096, dtype=torch.int32, device=dev)
    for path, flags in PATHS.items():
        got = call(rs, o, d, 1, 0.25, seed=2, flags=flags, device=True)
        after = torch.full((4096,), 5, dtype=torch.int32, device=dev)
        check(got, comp["occluded"], comp["visibility"], comp["hits"], comp["traced"], f"2^20 + 77 rays, {path}")
        assert torch.equal(before.cpu(), torch.arange(4096, dtype=torch.int32)) and bool((after == 5).all())
    assert comp["occluded"][1 << 20:].any() and comp["occluded"][:1 << 20].any()


def test_a_host_batch_across_the_ray_chunk_cut(cornell, oracle_mod):
    """2^20 + 77 host rays at S = 1 with a radius per ray: two chunks, the radii
    staged behind a whole chunk's rays.  The rays around the cut against a call
    on those 205 alone with index_base advanced to them, bit for bit."""
    soup, rs = cornell
    n = (1 << 20) + 77
    idx = np.arange(n) % 128
    o, d = (np.ascontiguousarray(x[idx]) for x in box_rays(soup, 128, 6))
    radius = np.array([0.25, 1.0, np.inf, 0.0, np.nan, 0.5], F)[np.arange(n) % 6]
    traced = composition(oracle_mod, rs, o, d, 1, radius, seed=2)["traced"]
    lo = (1 << 20) - 128
    for path, flags in PATHS.items():
        occ, vis, hits, st = call(rs, o, d, 1, radius, seed=2, flags=flags)
        near = call(rs, o[lo:], d[lo:], 1, radius[lo:], seed=2, key0=lo, flags=flags)
        assert near[0][:128].any() and near[0][128:].any() and (near[0] == 0).any()
        check((occ[lo:], vis[lo:], hits[lo:], near[3]), near[0], near[1], near[2],
              near[3]["segments"] - 205, f"around the cut, {path}")
        print("occlusion segments", path, st["segments"], n + traced)
        assert (st["segments"], st["hits"]) == (n + traced, int(occ.astype(np.int64).sum())), path


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_launches_of_one_small_chunk(device, case, context, oracle_mod):
    """A seed's 128 rays at S = 3, one chunk and one sub-chunk:
    zrt_stats.trace_launches per mode, as the sequence in
    zrt_context_occlusion's comment gives them (recorded on the GPU at the
    commit before the query calls came to share their host code)."""
    if device and (torch is None or not torch.cuda.is_available()):
        pytest.skip("torch sees no device")
    seed = RADIUS_SEEDS[2]
    cs, rs = case(seed), context(seed)
    radius = occlusion_ref.fuzz_radius(cs.soup)
    occ, vis, traced, _ = occlusion_ref.occlusion_batch(cs.ref, occlusion_ref.cached_samples(cs), radius, 3)
    assert traced > 0
    want = {"lane": 2 + 1 + 2 + 1 + 1,      # first hits: the fast walk + the rest; gen; the list: the fast walk + the
                                            # rest; reduce (list); finish
            "park": 4 + 1 + 2 + 1,          # first hits: pack + park + out + the rest; gen; park + reduce (queue): every
                                            # sample is in the fast domain, the list is empty; finish
            "counting": 1 + 1 + 1 + 1 + 1}  # first hits: the counting walk; gen; the counting any-hit walk; reduce
                                            # (list); finish
    got = {}
    for mode, kw in (("lane", {"flags": native.FLAG_LANE_WALK}), ("park", {"flags": native.TRACE_PARK}),
                     ("counting", {"stats": True})):
        res = call(rs, cs.o, cs.d, 3, radius, seed=cs.rseed, device=device, **kw)
        check(res, occ, vis, cs.bits, traced, f"128 rays, {mode}")
        got[mode] = res[3]["trace_launches"]
    print("occlusion launches", "device" if device else "host", got)
    assert got == want


def test_output_subsets_leave_the_other_arrays_alone(cornell, oracle_mod):
    soup, rs = cornell
    o, d = box_rays(soup, 300, 8)
    comp = composition(oracle_mod, rs, o, d, 4, 0.25)
    for path, flags in PATHS.items():
        for want_vis, want_occ in ((True, False), (False, True), (True, True)):
            for want_hits in (False, True):
                occ, vis, hit, st = guarded_call(rs, o, d, 4, 0.25, flags, want_vis, want_occ, want_hits)
                what = (path, want_vis, want_occ, want_hits)
                assert occ is None or np.array_equal(occ, comp["occluded"]), what
                assert vis is None or np.array_equal(vis, comp["visibility"]), what
                assert hit is None or np.array_equal(hit, comp["hits"]), what
                assert (st["segments"], st["hits"]) == (300 + comp["traced"], int(comp["occluded"].sum())), what


def test_a_miss_is_exactly_one(cornell):
    """Every missed ray: occluded = 0, visibility = 1.0f, at the smallest S
    for which f32(S) * (f32(1) / f32(S)) is not 1."""
    S = np.arange(1, 65536, dtype=np.uint32).astype(F)
    S = int(S[np.nonzero(S * (F(1) / S) != 1)[0][0]])
    soup, rs = cornell
    o, d = box_rays(soup, 500, 3, inside=0.0)
    o, d = np.concatenate([o, o[:100] + 1000]), np.concatenate([d, d[:100]])
    for path, flags in PATHS.items():
        res = rs.occlusion(o, d, S, flags=flags, hits=True)
        miss = res["triangle"] == native.MISS
        assert miss.sum() >= 100 and (~miss).sum() >= 100
        assert not res["occluded"][miss].any() and (res["visibility"][miss].view(np.uint32) == ONE).all(), path
        open_ = ~miss & (res["occluded"] == 0)
        assert (res["visibility"][open_].view(np.uint32) == ONE).all()
        assert np.array_equal(res["visibility"], occlusion_ref.visibility(res["occluded"], S))


def test_samples_of_nan_infinite_and_huge_normals_are_not_traced(oracle_mod):
    """The corner of test_occlusion_host.py with the vertex normals of its four
    triangles NaN, inf, 3e38 and (the control) unit length."""
    soup = toh.corner_soup()
    nrm = np.array(soup.nrm, np.float32).reshape(4, 3, 3)
    nrm[0], nrm[1], nrm[2] = np.nan, np.inf, nrm[2] * F(3e38)
    soup = toh.dataclasses.replace(soup, nrm=nrm.reshape(4, 9))
    o = np.array([[2, -2, 5], [-2, 2, 5], [0, 0, 0.5], [0, 0, 3.5]], F)
    d = np.array([[0, 0, -1], [0, 0, -1], [1, 0, 0], [1, 0, 0]], F)
    S = 16
    rs = RenderScene(soup, (4, 4, 4), device=0)
    try:
        src = rs.trace(o, d)["source_triangle"]
        assert list(src) == [0, 1, 2, 3]
        comp = composition(oracle_mod, rs, o, d, S, np.inf, seed=1)
        assert comp["traced"] == S and comp["occluded"][3] > 0
        for mode, flags in MODES.items():
            got = call(rs, o, d, S, np.inf, seed=1, flags=flags)
            check(got, comp["occluded"], comp["visibility"], comp["hits"], S, f"odd normals, {mode}")
            assert not got[0][:3].any() and (got[1][:3] == ONE).all()
        got = call(rs, o, d, S, np.inf, seed=1, stats=True)
        comp = composition(oracle_mod, rs, o, d, S, np.inf, seed=1, counting=True)
        check(got, comp["occluded"], comp["visibility"], comp["hits"], S, "odd normals, counting")
        assert (got[3]["cells_visited"], got[3]["triangle_tests"]) == comp["counts"]
    finally:
        rs.close()


# ------------------------------------------------------------------------ other
def test_occlusion_renders_and_segments_share_a_context_cleanly(cornell, oracle_mod):
    soup, rs = cornell
    cam = camera_for(soup, None, 24, 24)
    fresh = RenderScene(soup, (16, 16, 16), device=0)
    want, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    o, d = box_rays(soup, 3000, 21)
    comp = composition(oracle_mod, rs, o, d, 4, 0.25)
    seg = trace_ref.hit_bits(rs.segments(o, d, 0.5))
    for path, flags in PATHS.items():
        img, _ = rs.render(cam, num_samples=2, max_bounce=4, flags=native.FLAG_KERNEL_TIMES)
        assert np.array_equal(img, want), f"render before a {path} occlusion call"
        prof = rs.context.profile()
        check(call(rs, o, d, 4, 0.25, flags=flags), comp["occluded"], comp["visibility"], comp["hits"], comp["traced"],
              path)
        assert rs.context.profile() == prof, "zrt_context_profile's record is the last render's"
        img, _ = rs.render(cam, num_samples=2, max_bounce=4)
        assert np.array_equal(img, want), f"render after a {path} occlusion call"
        assert np.array_equal(trace_ref.hit_bits(rs.segments(o, d, 0.5, flags=flags)), seg), path
        check(call(rs, o, d, 4, 0.25, flags=flags), comp["occluded"], comp["visibility"], comp["hits"], comp["traced"],
              f"{path} again")


def test_empty_and_bad_batches_on_a_live_context(cornell):
    ctx = cornell[1].context
    out = np.full(8, 0xABABABAB, np.uint32)
    rays = np.zeros(6, np.float32)
    r, p = rays.ctypes.data, out.ctypes.data
    for flags in (0, native.TRACE_PARK):
        st = ctx.occlusion_raw(0, r, None, p, p, None, False, 4, flags=flags)
        assert st["segments"] == 0 and st["hits"] == 0
    ctx.occlusion_raw(0, None, None, None, None, None, False, 4)
    z = np.zeros((0, 3), np.float32)
    res = ctx.occlusion(z, z, 4, hits=True)
    assert res["visibility"].shape == (0,) and res["occluded"].shape == (0,) and res["t"].shape == (0,)
    for args, kw in (((None, None, p, p, None, False, 4), {}), ((r, None, None, None, p, False, 4), {}),
                     ((r, None, p, p, None, False, 4), {"flags": native.SEGMENT_ANY}),
                     ((r, None, p, p, None, False, 4), {"flags": 0x4}),
                     ((r, None, p, p, None, False, 0), {}), ((r, None, p, p, None, False, 65536), {})):
        with pytest.raises(native.ZrtError) as e:
            ctx.occlusion_raw(1, *args, **kw)
        assert e.value.status == -1
    assert (out == 0xABABABAB).all()
    ctx.occlusion_raw(1, r, None, p, out[4:].ctypes.data, None, False, 65535)   # the control: the valid batch runs
