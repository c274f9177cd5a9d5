"""Transmittance queries (zrt_context_transmittance) on the GPU, against the
per-ray reference (transmit_ref.py), bit for bit: T and n of every ray, and the
segment / cell / test / crossing totals.

The rays are the fuzz seeds' (test_query_fuzz_gpu.seed_rays: MASK and BLEND
materials, 1x1 .. 17x17 alpha textures, chains of up to 16 crossings), each
seed on its own context (host build for even seeds, device build for odd ones),
through the lane path, the park path, the park path with the cull masks forced
on and the IEEE-division kernel, under caps 1, 3 and 16.  Bounds are built from
the reference's own chains.  On an opaque scene the call has to answer exactly
as an any-hit segment call does.
"""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native

import test_query_fuzz_gpu as qf
import test_trace_gpu as ttg
import trace_ref
import transmit_ref

pytestmark = pytest.mark.gpu

F = np.float32
CAP = transmit_ref.CAP
MODES = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK, "park_bfcull": native.TRACE_PARK | native.FLAG_BFCULL,
         "mt_exact": native.FLAG_MT_EXACT}
BOUND_SEEDS = [4, 12, 18, 31]
BIG = 18                       # the seed whose rays the size tests tile: a 16-crossing chain among them


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


def free_ref(cs, cap=CAP):
    """(T bits, n, totals) of the seed's rays, unbounded, under `cap`."""
    if not hasattr(cs, "_transmit_free"):
        cs._transmit_free = {}
    if cap not in cs._transmit_free:
        T, n, tot, _ = transmit_ref.transmit_batch(cs.ref, cs.soup, cs.o, cs.d, np.inf, cap,
                                                   chains=transmit_ref.cached_chains(cs))
        T.setflags(write=False)
        n.setflags(write=False)
        cs._transmit_free[cap] = (T, n, tot)
    return cs._transmit_free[cap]


def _check(res, T, n, what):
    got_T, got_n = np.asarray(res["transmittance"]).view(np.uint32), np.asarray(res["crossings"])
    bad = np.nonzero((got_T != T) | (got_n != n))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rays differ, first {bad[0]}: got T {hex(int(got_T[bad[0]]))} n "
                           f"{int(got_n[bad[0]])}, reference T {hex(int(T[bad[0]]))} n {int(n[bad[0]])}")


# how the park path's round loop ends (the library reads these per call): the
# default hands a small remainder to one lane launch after any round, here
# after the first; TAIL = 0 runs every (park, step) round; "fixed" runs
# max_crossings rounds without reading the survivor counts back
ENDINGS = {"tail": {}, "every_round": {"ZRT_TRANSMIT_TAIL": "0"}, "fixed": {"ZRT_TRANSMIT_ROUNDS": "fixed"}}


@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_transmittance_matches_the_reference(seed, case, context, monkeypatch):
    cs, rs = case(seed), context(seed)
    for cap in (1, 3, CAP):
        T, n, tot = free_ref(cs, cap)
        what = f"seed {seed}, {cs.soup.num_triangles} triangles, grid {cs.res}, cap {cap}"
        for mode, flags in MODES.items():
            for ending, env in ENDINGS.items() if mode.startswith("park") else [("", {})]:
                with monkeypatch.context() as mp:
                    for k, v in env.items():
                        mp.setenv(k, v)
                    res = rs.transmittance(cs.o, cs.d, max_crossings=cap, flags=flags, crossings=True)
                _check(res, T, n, f"{what}, {mode} {ending}")
                st = res["stats"]
                assert (st["segments"], st["hits"], st["samples"]) == (tot[0], tot[3], 0), (what, mode, ending, st, tot)
        res = rs.transmittance(cs.o, cs.d, max_crossings=cap, stats=True, crossings=True)
        _check(res, T, n, f"{what}, counting")
        st = res["stats"]
        assert (st["segments"], st["cells_visited"], st["triangle_tests"], st["hits"]) == tot, (what, st, tot)


def bounds_from_chains(chains):
    """A bound per ray from the reference's own unbounded chain: between two
    consecutive crossings, exactly a crossing's t, below the first crossing,
    NaN, 0 and -inf by turns; 1 for a ray that crosses nothing."""
    tm = np.ones(len(chains), F)
    for i, c in enumerate(chains):
        at = c.at
        if not at:
            continue
        k = (i // 8) % len(at)
        nxt = at[k + 1] if k + 1 < len(at) else 2 * at[k] + 1
        tm[i] = (F(0.5 * (at[k] + nxt)), F(0.5 * (at[0] + (at[1] if len(at) > 1 else 2 * at[0]))), F(0.5 * (at[k] + nxt)),
                 F(at[0]), F(0.5 * at[0]), F(np.nan), F(0), F(-np.inf))[i % 8]
    return tm


def bounded_ref(cs):
    """The bounds of bounds_from_chains and a scalar bound, with their references; computed once."""
    if not hasattr(cs, "_transmit_bounded"):
        free = transmit_ref.cached_chains(cs)
        tm = bounds_from_chains(free)
        T, n, tot, ch = transmit_ref.transmit_batch(cs.ref, cs.soup, cs.o, cs.d, tm, CAP)
        cut = sum(len(b.T_after) < len(f.T_after) for b, f in zip(ch, free))
        first = [c.at[0] for c in free if c.at]
        scalar = F(np.median(first))
        sT, sn, stot, _ = transmit_ref.transmit_batch(cs.ref, cs.soup, cs.o, cs.d, scalar, CAP)
        cs._transmit_bounded = (tm, T, n, tot, cut, scalar, sT, sn, stot)
    return cs._transmit_bounded


@pytest.mark.parametrize("seed", BOUND_SEEDS)
def test_bounds_cut_the_chains_as_the_reference_does(seed, case, context):
    cs, rs = case(seed), context(seed)
    tm, T, n, tot, cut, scalar, sT, sn, stot = bounded_ref(cs)
    assert cut >= 16, f"seed {seed}: the bounds cut only {cut} chains"
    special = ~np.isfinite(tm) | (tm <= 0)
    assert special.sum() >= 16 and (T[special] == F(1).view(np.uint32)).all() and not n[special].any()
    for mode, flags in MODES.items():
        res = rs.transmittance(cs.o, cs.d, tm, flags=flags, crossings=True)
        _check(res, T, n, f"seed {seed}, per-ray bounds, {mode}")
        assert (res["stats"]["segments"], res["stats"]["hits"]) == (tot[0], tot[3])
        res = rs.transmittance(cs.o, cs.d, float(scalar), flags=flags, crossings=True)
        _check(res, sT, sn, f"seed {seed}, t_max_all = {scalar}, {mode}")
        assert (res["stats"]["segments"], res["stats"]["hits"]) == (stot[0], stot[3])
    res = rs.transmittance(cs.o, cs.d, tm, stats=True, crossings=True)
    _check(res, T, n, f"seed {seed}, per-ray bounds, counting")
    st = res["stats"]
    assert (st["segments"], st["cells_visited"], st["triangle_tests"], st["hits"]) == tot


# ------------------------------------------------ cross-checks against segments
def test_on_an_opaque_scene_it_is_the_any_hit_segment_call(oracle_mod):
    mk, res = ttg.CASES["cornell_bm"]
    soup = mk()
    ref = trace_ref.RayRef(oracle_mod, soup, res)
    o, d = ttg._case_rays(ref, soup, 1)
    diag = F(np.linalg.norm((ref.bmax - ref.bmin).astype(F)))
    tm = (np.random.default_rng(5).random(len(o), dtype=F) * diag).astype(F)
    rs = RenderScene(soup, res, device=0)
    try:
        for bound in (np.inf, tm):
            occ = rs.segments(o, d, bound, any_hit=True)["occluded"]
            assert occ.sum() >= 16 and (~occ).sum() >= 16
            for mode, flags in MODES.items():
                r = rs.transmittance(o, d, bound, flags=flags, crossings=True)
                want = np.where(occ, F(0), F(1)).view(np.uint32)
                _check(r, want, occ.astype(np.uint32), f"cornell, {mode}")
    finally:
        rs.close()


def test_crossings_are_where_segments_reports_a_hit(case, context):
    cs, rs = case(12), context(12)
    tm = bounded_ref(cs)[0]
    for bound in (np.inf, tm):
        hit = rs.segments(cs.o, cs.d, bound)["occluded"]
        for mode, flags in MODES.items():
            r = rs.transmittance(cs.o, cs.d, bound, flags=flags, crossings=True)
            assert np.array_equal(r["crossings"] >= 1, hit), mode
            assert ((r["transmittance"] == 1) | hit).all(), mode


# ------------------------------------------------------------------ batch sizes
@pytest.mark.parametrize("mode", ["lane", "park"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_batch_sizes_and_the_words_beside_the_outputs(n, mode, case, context):
    cs, rs = case(BIG), context(BIG)
    T, cr, _ = free_ref(cs)
    pick = np.resize(np.random.default_rng(7).permutation(qf.N_RAYS), n)
    rays = np.ascontiguousarray(np.concatenate([cs.o[pick], cs.d[pick]], axis=1))
    out_T = np.full(n + 2, 0xABABABAB, np.uint32)
    out_n = np.full(n + 2, 0xCDCDCDCD, np.uint32)
    st = rs.context.transmittance_raw(n, rays.ctypes.data, None, out_T[1:].ctypes.data, out_n[1:].ctypes.data, False,
                                      MODES[mode])
    assert out_T[0] == out_T[-1] == 0xABABABAB and out_n[0] == out_n[-1] == 0xCDCDCDCD, "guard words"
    _check({"transmittance": out_T[1:-1], "crossings": out_n[1:-1]}, T[pick], cr[pick], f"n = {n} {mode}")
    assert st["hits"] == int(cr[pick].sum())
    # crossings = null: the same T, nothing else written
    out_T[:] = 0xABABABAB
    rs.context.transmittance_raw(n, rays.ctypes.data, None, out_T[1:].ctypes.data, None, False, MODES[mode])
    assert out_T[0] == out_T[-1] == 0xABABABAB and np.array_equal(out_T[1:-1], T[pick])


def test_the_unasked_park_threshold(case, context, monkeypatch):
    """2^16 + 192 rays, past a segment call's unasked park threshold: this call
    keeps the lane path there (it measured faster) and parks when asked."""
    cs, rs = case(BIG), context(BIG)
    T, cr, tot = free_ref(cs)
    n = (1 << 16) + 192
    idx = np.arange(n) % qf.N_RAYS
    o, d = cs.o[idx], cs.d[idx]
    res = {m: rs.transmittance(o, d, flags=f, crossings=True)
           for m, f in (("lane", native.FLAG_LANE_WALK), ("park", native.TRACE_PARK), ("unasked", 0))}
    for m, r in res.items():
        _check(r, T[idx], cr[idx], f"n = {n} {m}")
        assert r["stats"]["hits"] == int(cr[idx].astype(np.int64).sum()), m
        assert r["stats"]["segments"] == res["lane"]["stats"]["segments"], m
    launches = {m: r["stats"]["trace_launches"] for m, r in res.items()}
    # pack, one (park, step) round, the tail (fewer than 2^16 rays go on), the rest
    assert launches == {"lane": 2, "park": 5, "unasked": 2}, launches
    # every round: pack, a (park, step) pair per round, the rest; the rounds: the longest chain's segments among the
    # rays of the fast domain (the others' whole chains are the last launch's)
    monkeypatch.setenv("ZRT_TRANSMIT_TAIL", "0")
    r = rs.transmittance(o, d, flags=native.TRACE_PARK, crossings=True)
    _check(r, T[idx], cr[idx], f"n = {n} every round")
    segs = np.array([c.cut(CAP)[2] for c in transmit_ref.cached_chains(cs)])
    fast = np.abs((cs.d.astype(np.float64) ** 2).sum(1) - 1.0) <= 0.49
    assert int(cr.max()) == CAP and segs[fast].max() >= 8
    assert r["stats"]["trace_launches"] == 2 + 2 * int(segs[fast].max())


def test_torch_tensors_in_place_across_the_chunk_cut(case, context):
    """2^20 + 77 rays on the device: two chunks; with and without `crossings`."""
    if torch is None or not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    cs, rs = case(BIG), context(BIG)
    T, cr, _ = free_ref(cs)
    n = (1 << 20) + 77
    dev = torch.device("cuda", 0)
    idx = torch.arange(n, device=dev) % qf.N_RAYS
    o, d = torch.from_numpy(cs.o).to(dev)[idx].contiguous(), torch.from_numpy(cs.d).to(dev)[idx].contiguous()
    want_T = torch.from_numpy(T.view(np.int32).copy()).to(dev)[idx]
    want_n = torch.from_numpy(cr.astype(np.int32)).to(dev)[idx]
    before = torch.arange(4096, dtype=torch.int32, device=dev)
    # (park: several rounds over more than 2^16 survivors, then the tail; without `crossings` n lives in the context)
    for flags, crossings in ((native.TRACE_PARK, True), (native.TRACE_PARK, False), (0, True), (0, False)):
        res = rs.transmittance(o, d, flags=flags, crossings=crossings)
        after = torch.full((4096,), 5, dtype=torch.int32, device=dev)
        got = res["transmittance"]
        assert got.shape == (n,) and got.dtype == torch.float32 and got.device == dev
        assert torch.equal(got.view(torch.int32), want_T), (flags, crossings)
        if crossings:
            assert res["crossings"].dtype == torch.int32 and torch.equal(res["crossings"], want_n)
        else:
            assert "crossings" not in res
        assert torch.equal(before.cpu(), torch.arange(4096, dtype=torch.int32)) and bool((after == 5).all())
        assert res["stats"]["hits"] == int(want_n.sum().item())
    # a per-ray bound tensor and a float bound, 200 rays
    tm, bT, bn, _, _, scalar, sT, sn, _ = bounded_ref(cs)
    res = rs.transmittance(o[:128], d[:128], torch.from_numpy(tm.copy()).to(dev), crossings=True)
    _check({k: res[k].cpu().numpy() for k in ("transmittance", "crossings")}, bT, bn.astype(np.int32), "torch bounds")
    res = rs.transmittance(o[:128], d[:128], float(scalar), flags=native.TRACE_PARK, crossings=True)
    _check({k: res[k].cpu().numpy() for k in ("transmittance", "crossings")}, sT, sn.astype(np.int32), "torch scalar")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_launches_of_one_small_chunk(device, case, context):
    """The seed's 128 rays, one chunk: zrt_stats.trace_launches per mode, as the
    sequence in zrt_context_transmittance's comment gives them (recorded on the
    GPU at the commit before the query calls came to share their host code)."""
    if device and (torch is None or not torch.cuda.is_available()):
        pytest.skip("torch sees no device")
    cs, rs = case(BIG), context(BIG)
    T, cr, _ = free_ref(cs)
    o, d = cs.o, cs.d
    if device:
        o, d = torch.from_numpy(cs.o).to("cuda:0"), torch.from_numpy(cs.d).to("cuda:0")
    want = {"lane": 1 + 1,              # the fast walk + the rest
            "park": 1 + 2 + 1 + 1,      # pack + one (park, step) round + the tail (some chains go on, few) + the rest
            "counting": 1}              # the counting IEEE-division walk alone
    got = {}
    for mode, kw in (("lane", {"flags": native.FLAG_LANE_WALK}), ("park", {"flags": native.TRACE_PARK}),
                     ("counting", {"stats": True})):
        res = rs.transmittance(o, d, crossings=True, **kw)
        if device:
            res = {k: (v.cpu().numpy() if k != "stats" else v) for k, v in res.items()}
        _check(res, T, cr.astype(res["crossings"].dtype), f"128 rays, {mode}")
        got[mode] = res["stats"]["trace_launches"]
    print("transmittance launches", "device" if device else "host", got)
    assert got == want


def test_a_host_batch_across_the_chunk_cut(case, context):
    """2^20 + 77 host rays with a bound and `crossings` per ray: two chunks,
    the bounds staged behind a whole chunk's rays.  The rays around the cut
    against a call on those 205 alone, bit for bit."""
    cs, rs = case(BIG), context(BIG)
    tm, _, _, tot = bounded_ref(cs)[:4]
    n = (1 << 20) + 77
    idx = np.arange(n) % qf.N_RAYS
    o, d, bound = cs.o[idx], cs.d[idx], tm[idx]
    rest = n % qf.N_RAYS
    segments = (n // qf.N_RAYS) * tot[0] + transmit_ref.transmit_batch(cs.ref, cs.soup, cs.o[:rest], cs.d[:rest], tm[:rest],
                                                                        CAP)[2][0]
    lo = (1 << 20) - 128
    for mode, flags in (("lane", native.FLAG_LANE_WALK), ("park", native.TRACE_PARK)):
        res = rs.transmittance(o, d, bound, flags=flags, crossings=True)
        near = rs.transmittance(o[lo:], d[lo:], bound[lo:], flags=flags, crossings=True)
        assert near["crossings"].any() and (near["crossings"] == 0).any()
        _check({k: res[k][lo:] for k in ("transmittance", "crossings")}, near["transmittance"].view(np.uint32),
               near["crossings"], f"around the cut, {mode}")
        print("transmittance segments", mode, res["stats"]["segments"], segments)
        assert res["stats"]["segments"] == segments, mode


# ------------------------------------------------------------------------ other
def test_transmittance_renders_and_segments_share_a_context_cleanly(case, context):
    cs = case(BIG)
    T, cr, _ = free_ref(cs)
    cam = camera_for(cs.soup, None, 24, 24)
    fresh = RenderScene(cs.soup, cs.res, device=0, device_build=cs.device_build)
    want, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    rs = context(BIG)
    seg = trace_ref.hit_bits(rs.segments(cs.o, cs.d, 1.0))
    for mode, flags in MODES.items():                  # the same answers, a render and a segment call in between
        _check(rs.transmittance(cs.o, cs.d, flags=flags, crossings=True), T, cr, mode)
        img, _ = rs.render(cam, num_samples=2, max_bounce=4)
        assert np.array_equal(img, want), f"render after a {mode} transmittance call"
        assert np.array_equal(trace_ref.hit_bits(rs.segments(cs.o, cs.d, 1.0, flags=flags)), seg), mode
        _check(rs.transmittance(cs.o, cs.d, flags=flags, crossings=True), T, cr, f"{mode} again")


def test_empty_and_bad_batches_on_a_live_context(case, context):
    ctx = context(BIG).context
    T = np.full(8, 0xABABABAB, np.uint32)
    rays = np.zeros(6, np.float32)
    for flags in (0, native.TRACE_PARK):
        st = ctx.transmittance_raw(0, rays.ctypes.data, None, T.ctypes.data, None, False, flags)
        assert st["segments"] == 0 and st["hits"] == 0
    ctx.transmittance_raw(0, None, None, None, None, False, 0)
    assert (T == 0xABABABAB).all()
    z = np.zeros((0, 3), np.float32)
    res = ctx.transmittance(z, z, crossings=True)
    assert res["transmittance"].shape == (0,) and res["crossings"].shape == (0,)
    r, t = rays.ctypes.data, T.ctypes.data
    for args, kw in (((None, None, t, None, False, 0), {}), ((r, None, None, None, False, 0), {}),
                     ((r, None, t, None, False, native.SEGMENT_ANY), {}), ((r, None, t, None, False, 0x4), {}),
                     ((r, None, t, None, False, 0), {"max_crossings": 0}),
                     ((r, None, t, None, False, 0), {"max_crossings": 257})):
        with pytest.raises(native.ZrtError) as e:
            ctx.transmittance_raw(1, *args, **kw)
        assert e.value.status == -1
    assert (T == 0xABABABAB).all()
    ctx.transmittance_raw(1, r, None, t, None, False, 0, max_crossings=256)     # the control: the valid batch runs
