"""Sky-light queries on the GPU, bit for bit.

The call -- `irradiance`, `radiance`, `visibility` and the first hits, and
segments, samples and hits in every call -- against two references:

  the CPU reference (sky_light_ref.py) on the fuzz seeds' rays and on the
  hand-made scenes of test_sky_light_host.py;
  a device composition that needs no CPU walk: Context.surface, the draws from
  oracle.path_norm, the directions and the sky's colour in numpy float32 over
  whole arrays, Context.transmittance over exactly the traced items, and an
  ordered numpy sum over the samples.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import sky_light_ref as slr
import test_query_fuzz_gpu as qf
import test_sky_light_host as tsh
import trace_ref
from test_direct_gpu import MODES, PATHS, box_rays, use_device, vnormalize

pytestmark = pytest.mark.gpu

F = np.float32
M32 = 0xFFFFFFFF
SKY_C = np.array([0.5, 0.7, 1.0], F)


def have_torch():
    return torch is not None and torch.cuda.is_available()


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


def draws(orc, seed, keys, S):
    """(n, S, 3) float32: the first three floatNorm draws of the streams
    (seed, keys[i], s), each asked of the oracle once."""
    out = np.zeros((len(keys), S, 3), F)
    seed &= 2 ** 64 - 1
    for i, key in enumerate(keys):
        for s in range(S):
            k = (seed, int(key), s)
            if k not in _DRAWS:
                _DRAWS[k] = orc.path_norm(seed, int(key), s, 3)
            out[i, s] = _DRAWS[k]
    return out


def composition(rs, orc, o, d, S, seed=0, index_base=0, cap=16, unshadowed=False, counting=False):
    n = len(o)
    surf = rs.surface(o, d, hits=True, stats=counting)
    hit = surf["material"] != native.MISS
    pos = np.ascontiguousarray(surf["position"], F)
    keys = [(index_base + i) & M32 for i in range(n)]
    with np.errstate(all="ignore"):
        N = vnormalize(surf["normal"])
        shaded = hit & np.isfinite(pos).all(1) & np.isfinite(N).all(1)
        segs = cross = 0
        counts = (surf["stats"]["cells_visited"], surf["stats"]["triangle_tests"]) if counting else None
        D = vnormalize(N[:, None, :] + vnormalize(draws(orc, seed, keys, S)))
        TR = shaded[:, None] & np.isfinite(D).all(2) & (D != 0).any(2)
        t = F(0.5) * (D[..., 1] + F(1.0))
        L = (F(1.0) - t)[..., None] + SKY_C * t[..., None]
        assert L.dtype == F and D.dtype == F
        T = np.ones((n, S), F)
        if not unshadowed and TR.any():
            po = np.ascontiguousarray(np.broadcast_to(pos[:, None, :], (n, S, 3))[TR])
            tr = rs.transmittance(po, np.ascontiguousarray(D[TR]), np.full(len(po), np.inf, F), max_crossings=cap,
                                  stats=counting)
            T[TR] = tr["transmittance"]
            segs, cross = tr["stats"]["segments"], tr["stats"]["hits"]
            if counting:
                counts = (counts[0] + tr["stats"]["cells_visited"], counts[1] + tr["stats"]["triangle_tests"])
        A, V = np.zeros((n, 3), F), np.zeros(n, F)
        for s in range(S):
            A = np.where(TR[:, s][:, None], A + L[:, s] * T[:, s][:, None], A)
            V = np.where(TR[:, s], V + T[:, s], V)
        mean, V = A / F(S), V / F(S)
        E = mean * slr.PI
        R = np.where(shaded[:, None], surf["emissive"] + surf["base_color"] * mean, surf["emissive"])
        E, R, V = (np.where(hit.reshape((n,) + (1,) * (x.ndim - 1)), x, F(0)).astype(F) for x in (E, R, V))
    return {"irradiance": E.view(np.uint32), "radiance": R.view(np.uint32), "visibility": V.view(np.uint32),
            "hits": trace_ref.hit_bits(surf), "segments": int(segs), "samples": int(TR.sum()), "crossings": int(cross),
            "counts": counts, "traced": TR, "hit": hit, "shaded": shaded}


def call(rs, o, d, S, seed=0, index_base=0, cap=16, flags=0, device=False, stats=False, unshadowed=False):
    """Context.sky_light with host arrays or, `device`, torch tensors, as
    (irradiance bits, radiance bits, visibility bits, hit bits, stats)."""
    kw = dict(max_crossings=cap, seed=seed, index_base=index_base, flags=flags, unshadowed=unshadowed, hits=True,
              stats=stats)
    if device:
        dev = torch.device("cuda", 0)
        res = rs.context.sky_light(torch.from_numpy(np.ascontiguousarray(o)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(d)).to(dev), S, **kw)
        return (res["irradiance"].cpu().numpy().view(np.uint32), res["radiance"].cpu().numpy().view(np.uint32),
                res["visibility"].cpu().numpy().view(np.uint32), res["hits"].cpu().numpy().view(np.uint32), res["stats"])
    res = rs.context.sky_light(o, d, S, **kw)
    return (res["irradiance"].view(np.uint32), res["radiance"].view(np.uint32), res["visibility"].view(np.uint32),
            trace_ref.hit_bits(res), res["stats"])


def hexes(row):
    return [hex(int(x)) for x in np.atleast_1d(row)]


def check(got, want_E, want_R, want_V, want_hits, segments, samples, crossings, what):
    E, R, V, hits, st = got
    bad = np.nonzero((E != want_E).any(axis=1) | (R != want_R).any(axis=1) | (V != want_V) |
                     (hits != want_hits).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rays differ, first {bad[0]}: got E {hexes(E[bad[0]])} radiance "
                           f"{hexes(R[bad[0]])} visibility {hexes(V[bad[0]])} hit {hexes(hits[bad[0]])}, reference "
                           f"{hexes(want_E[bad[0]])} {hexes(want_R[bad[0]])} {hexes(want_V[bad[0]])} "
                           f"{hexes(want_hits[bad[0]])}")
    assert (st["segments"], st["samples"], st["hits"]) == (len(E) + segments, samples, crossings), (what, st)


def check_comp(got, comp, what):
    check(got, comp["irradiance"], comp["radiance"], comp["visibility"], comp["hits"], comp["segments"], comp["samples"],
          comp["crossings"], what)


# ------------------------------------------------------------------ the seeds
def check_case(rs, cs, rays, S, seed, dev, what):
    """The caps 16, 1 and 2 through MODES, the counting call and the
    unshadowed call through PATHS, against the CPU reference."""
    for cap in (16, 1, 2):
        E, R, V, tot = slr.sky_batch(cs.ref, cs.soup, rays, S, cap, counts=True)
        for mode, flags in (MODES if cap == 16 else {"unasked": 0}).items():
            check(call(rs, cs.o, cs.d, S, seed, cap=cap, flags=flags, device=dev), E, R, V, cs.bits, tot["segments"],
                  tot["samples"], tot["hits"], f"{what}, cap {cap}, {mode}")
        got = call(rs, cs.o, cs.d, S, seed, cap=cap, device=dev, stats=True)
        check(got, E, R, V, cs.bits, tot["segments"], tot["samples"], tot["hits"], f"{what}, cap {cap}, counting")
        want = (cs.counts[0] + tot["cells"], cs.counts[1] + tot["tests"])
        assert (got[4]["cells_visited"], got[4]["triangle_tests"]) == want, (what, cap, got[4], want)
    E, R, V, tot = slr.sky_batch(cs.ref, cs.soup, rays, S, unshadowed=True)
    for mode, flags in PATHS.items():
        for device in {False, dev}:
            check(call(rs, cs.o, cs.d, S, seed, flags=flags, device=device, unshadowed=True), E, R, V, cs.bits, 0,
                  tot["samples"], 0, f"{what}, unshadowed, {mode}")


@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_sky_light_matches_the_reference(seed, case, context, oracle_mod):
    cs, rs = case(seed), context(seed)
    rays = tsh.cached_rays(oracle_mod, cs)
    what = f"seed {seed}, {cs.soup.num_triangles} triangles, grid {cs.res}"
    check_case(rs, cs, rays, tsh.FUZZ_SPP, cs.seed, use_device(seed), what)


def test_hits_on_nan_infinite_and_huge_normals(case, oracle_mod):
    """direct_ref.PoisonedCase of seed 4: a hit on a NaN or infinite normal is
    not shaded -- no item, irradiance = visibility = +0, radiance = the
    emission; one on a 3e38 normal has N = 0, finite: shaded, its directions
    the draws themselves."""
    cs = tsh.poisoned_case(oracle_mod, case(tsh.POISON_SEED))
    rays = tsh.cached_rays(oracle_mod, cs)
    odd = np.array([r.words is not None and not r.shaded for r in rays])
    assert odd.sum() >= 5
    rs = RenderScene(cs.soup, cs.res, device=0, device_build=cs.device_build)
    try:
        E, R, V, tot = slr.sky_batch(cs.ref, cs.soup, rays, tsh.FUZZ_SPP)
        emis = rs.surface(cs.o, cs.d)["emissive"].view(np.uint32)
        for mode, flags in MODES.items():
            got = call(rs, cs.o, cs.d, tsh.FUZZ_SPP, cs.seed, flags=flags)
            check(got, E, R, V, cs.bits, tot["segments"], tot["samples"], tot["hits"], f"odd normals, {mode}")
            assert not got[0][odd].any() and not got[2][odd].any() and np.array_equal(got[1][odd], emis[odd]), mode
    finally:
        rs.close()


def test_the_hand_scenes(oracle_mod):
    S, seed = 16, 11
    cases = [(name, {}) for name in tsh.HAND_CASES] + [("open", dict(floor_normal=(0, 0, 0))),
                                                      ("open", dict(floor_normal=(0, -1, 0), up=False)),
                                                      ("one pane", dict(floor_normal=tsh.TILTED))]
    for name, kw in cases:
        ref, soup, o, d, bits, _ = tsh.hand_case(oracle_mod, name, S, seed, **kw)
        o = np.concatenate([o, o]).astype(F)                                 # ... and a ray that misses
        d = np.concatenate([d, np.array([[0, 1 if kw.get("up", True) else -1, 0]], F)])
        bits, _ = ref.trace_batch(o, d)
        assert bits[0, 3] != trace_ref.MISS and bits[1, 3] == trace_ref.MISS, name
        rays = slr.make_rays(oracle_mod, ref, soup, o, d, bits, S, seed=seed)
        rs = RenderScene(soup, tsh.HAND_RES, device=0)
        try:
            for cap in (16, 1):
                E, R, V, tot = slr.sky_batch(ref, soup, rays, S, cap)
                if not kw:
                    assert V.view(F)[0] == {"open": 1.0, "one pane": 0.75, "two panes": 0.5625 if cap == 16 else 0.75,
                                            "roof": 0.0}[name]
                for mode, flags in MODES.items():
                    for device in ([False, True] if have_torch() else [False]):
                        check(call(rs, o, d, S, seed, cap=cap, flags=flags, device=device), E, R, V, bits,
                              tot["segments"], tot["samples"], tot["hits"], f"hand scene {name} {kw}, cap {cap}, {mode}")
            E, R, V, tot = slr.sky_batch(ref, soup, rays, S, unshadowed=True)
            check(call(rs, o, d, S, seed, unshadowed=True), E, R, V, bits, 0, tot["samples"], 0, f"{name}, unshadowed")
        finally:
            rs.close()


# ------------------------------------------------ shapes, on the Cornell box
@pytest.fixture(scope="module")
def cornell():
    soup = scenes.get_scene("cornell")
    rs = RenderScene(soup, (16, 16, 16), device=0)
    yield soup, rs
    rs.close()


def guarded_call(rs, o, d, S, flags, want_E=True, want_R=True, want_V=True, want_hits=True, cap=16, seed=0, index_base=0):
    """sky_light_raw on host arrays between guard words; an unasked array
    stays at its guard pattern."""
    n = len(o)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    E = np.full(3 * (n + 2), 0xABABABAB, np.uint32)
    R = np.full(3 * (n + 2), 0xCDCDCDCD, np.uint32)
    V = np.full(n + 2, 0x12121212, np.uint32)
    hit = np.full(4 * (n + 2), 0xEFEFEFEF, np.uint32)
    st = rs.context.sky_light_raw(n, rays.ctypes.data, E[3:].ctypes.data if want_E else None,
                                  R[3:].ctypes.data if want_R else None, V[1:].ctypes.data if want_V else None,
                                  hit[4:].ctypes.data if want_hits else None, False, S, cap, seed, index_base, flags)
    for a, w, g in ((E, 3, 0xABABABAB), (R, 3, 0xCDCDCDCD), (V, 1, 0x12121212), (hit, 4, 0xEFEFEFEF)):
        assert (a[:w] == g).all() and (a[-w:] == g).all(), "guard words"
    assert want_E or (E == 0xABABABAB).all()
    assert want_R or (R == 0xCDCDCDCD).all()
    assert want_V or (V == 0x12121212).all()
    assert want_hits or (hit == 0xEFEFEFEF).all()
    return (E[3:-3].reshape(n, 3) if want_E else None, R[3:-3].reshape(n, 3) if want_R else None,
            V[1:-1] if want_V else None, hit[4:-4].reshape(n, 4) if want_hits else None, st)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_ray_and_sample_counts_between_guard_words(n, cornell, oracle_mod):
    """The wave width and the four-items-per-thread stride are what these
    sizes straddle.  One seed for all S: a stream's draws do not depend on S,
    so the oracle is asked once per (ray, sample)."""
    soup, rs = cornell
    o, d = box_rays(soup, n, 100 + n)
    for S in (65, 64, 63, 2, 1):
        comp = composition(rs, oracle_mod, o, d, S, seed=5)
        if n >= 63 and S >= 2:
            v = comp["visibility"].view(F)
            assert comp["samples"] == S * comp["shaded"].sum() > 0 and ((v > 0) & (v < 1)).any() and (v == 0).any()
        for path, flags in PATHS.items():
            check_comp(guarded_call(rs, o, d, S, flags, seed=5), comp, f"n = {n}, S = {S}, {path}")


@pytest.mark.parametrize("only_radiance", [False, True], ids=["all outputs", "radiance alone"])
def test_a_ray_whose_samples_straddle_the_sub_chunk_cut(only_radiance, cornell, oracle_mod):
    """17 rays x 65535 samples = 1,114,095 items: one cut at item 2^20, at
    sample 16 of ray 16.  Rays 15, 16 and the last against one-ray calls at
    index_base + i, which never cross a cut; ray 16 against the composition
    too.  With `radiance` alone A and V have no caller row to wait in."""
    soup, rs = cornell
    n, S = 17, 65535
    assert (1 << 20) // S == 16 and (1 << 20) % S == 16 and n * S > 1 << 20
    o, d = box_rays(soup, n, 5, inside=1.0)
    o[16], d[16] = o[7], d[7]                                      # a ray that sees about half its sky
    kw = dict(max_crossings=16, seed=9, index_base=70)
    if only_radiance:
        kw.update(irradiance=False, visibility=False)
    res = rs.context.sky_light(o, d, S, **kw)
    assert res["stats"]["samples"] > 15 * S
    names = ["radiance"] if only_radiance else ["irradiance", "radiance", "visibility"]
    for i in (15, 16, n - 1):
        one = rs.context.sky_light(o[i:i + 1], d[i:i + 1], S, **dict(kw, index_base=70 + i))
        for k in names:
            assert res[k][i].tobytes() == one[k][0].tobytes(), (i, k, res[k][i], one[k][0])
    comp = composition(rs, oracle_mod, o[16:17], d[16:17], S, seed=9, index_base=86)
    v = comp["visibility"].view(F)[0]
    assert comp["traced"][0, :16].all() and comp["traced"][0, 16:].all() and 0 < v < 1, v
    for k in names:
        assert res[k][16].tobytes() == comp[k][0].tobytes(), (k, res[k][16], comp[k].view(F)[0])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_batch_across_the_ray_chunk_cut(device, cornell):
    """2^20 + 77 rays x 1 sample: two chunks.  The first 128 rays, the 128
    before the cut and the 77 behind it against calls on those alone with
    index_base advanced to them, bit for bit; every shaded ray's sample is
    traced."""
    if device and not have_torch():
        pytest.skip("torch sees no device")
    soup, rs = cornell
    n = (1 << 20) + 77
    idx = np.arange(n) % 128
    o, d = (np.ascontiguousarray(x[idx]) for x in box_rays(soup, 128, 6))
    lo = (1 << 20) - 128
    hit = rs.trace(o[:128], d[:128])["triangle"] != native.MISS
    for path, flags in PATHS.items():
        E, R, V, hits, st = call(rs, o, d, 1, 4, 1000, flags=flags, device=device)
        tot = [0, 0, 0]
        for a, b in ((0, 128), (lo, 1 << 20), (1 << 20, n)):
            near = call(rs, o[a:b], d[a:b], 1, 4, 1000 + a, flags=flags, device=device)
            check((E[a:b], R[a:b], V[a:b], hits[a:b], near[4]), near[0], near[1], near[2], near[3],
                  near[4]["segments"] - (b - a), near[4]["samples"], near[4]["hits"], f"rays {a}..{b}, {path}")
            assert near[4]["samples"] == hit[idx[a:b]].sum() > 0 and (near[2].view(F) > 0).any()
        assert st["samples"] == hit[idx].sum() and st["segments"] >= n + st["samples"], (path, st)


def test_output_subsets_leave_the_other_arrays_alone(cornell, oracle_mod):
    soup, rs = cornell
    o, d = box_rays(soup, 300, 8)
    comp = composition(rs, oracle_mod, o, d, 5, seed=2)
    for path, flags in PATHS.items():
        for mask in range(1, 8):
            for want_hits in (False, True):
                want = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]
                E, R, V, hit, st = guarded_call(rs, o, d, 5, flags, *want, want_hits, seed=2)
                what = (path, want, want_hits)
                assert E is None or np.array_equal(E, comp["irradiance"]), what
                assert R is None or np.array_equal(R, comp["radiance"]), what
                assert V is None or np.array_equal(V, comp["visibility"]), what
                assert hit is None or np.array_equal(hit, comp["hits"]), what
                assert (st["segments"], st["samples"], st["hits"]) == (300 + comp["segments"], comp["samples"],
                                                                       comp["crossings"]), what
    if have_torch():                               # ... and on the device, where an unasked row is the context's own
        dev = torch.device("cuda", 0)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        for mask in range(1, 8):
            res = rs.context.sky_light(to, td, 5, seed=2, irradiance=bool(mask & 1), radiance=bool(mask & 2),
                                       visibility=bool(mask & 4))
            for bit, k in ((1, "irradiance"), (2, "radiance"), (4, "visibility")):
                assert (k in res) == bool(mask & bit)
                assert k not in res or np.array_equal(res[k].cpu().numpy().view(np.uint32), comp[k]), (mask, k)


def test_index_base_wraps_at_2_32_and_device_pointers(cornell, oracle_mod):
    soup, rs = cornell
    o, d = box_rays(soup, 700, 17)
    base = 2 ** 32 - 300
    comp = composition(rs, oracle_mod, o, d, 3, seed=2 ** 63 + 5, index_base=base)
    low = composition(rs, oracle_mod, o[300:], d[300:], 3, seed=2 ** 63 + 5, index_base=0)
    assert np.array_equal(comp["irradiance"][300:], low["irradiance"]) and comp["irradiance"].any()
    for path, flags in PATHS.items():
        check_comp(call(rs, o, d, 3, 2 ** 63 + 5, base, flags=flags), comp, f"wrapping keys, {path}")
        check_comp(call(rs, o, d, 3, 2 ** 63 + 5, base + 2 ** 32, flags=flags), comp, f"keys mod 2^32, {path}")
        if have_torch():
            check_comp(call(rs, o, d, 3, 2 ** 63 + 5, base, flags=flags, device=True), comp, f"device pointers, {path}")


def test_unshadowed_against_numpy_alone(cornell, oracle_mod):
    soup, rs = cornell
    o, d = box_rays(soup, 3000, 12)
    comp = composition(rs, oracle_mod, o, d, 4, seed=1, unshadowed=True)
    lit = composition(rs, oracle_mod, o, d, 4, seed=1)
    assert comp["segments"] == 0 and comp["samples"] == lit["samples"] == 4 * comp["shaded"].sum() > 0
    assert not np.array_equal(comp["irradiance"], lit["irradiance"])
    v = comp["visibility"].view(F)
    assert ((v == 1) == comp["shaded"]).all() and ((v == 0) == ~comp["shaded"]).all()
    for mode, flags in MODES.items():
        got = call(rs, o, d, 4, 1, flags=flags, unshadowed=True)
        check_comp(got, comp, f"unshadowed, {mode}")
        assert got[4]["samples"] == comp["samples"] and got[4]["segments"] == len(o)
        # no walk launch: a lane-walk call is the first hits' two launches, the gen and the reduce launch
        assert mode != "lane" or got[4]["trace_launches"] == 4, got[4]
        check_comp(call(rs, o, d, 4, 1, flags=flags), lit, f"shadowed, {mode}")


# ------------------------------------------------------------------------ other
def test_a_sequence_on_one_context(cornell, oracle_mod):
    """render, sky light, render, area lights, sky light: the frames, the
    results, trace_launches and the profile record are a fresh context's."""
    soup, rs = cornell
    cam = camera_for(soup, None, 24, 24)
    o, d = box_rays(soup, 3000, 21)
    comp = composition(rs, oracle_mod, o, d, 4, seed=6)
    fresh = RenderScene(soup, (16, 16, 16), device=0)
    want, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    launches = {}
    for path, flags in PATHS.items():
        fresh = RenderScene(soup, (16, 16, 16), device=0)
        got = call(fresh, o, d, 4, 6, flags=flags)
        check_comp(got, comp, f"fresh context, {path}")
        launches[path] = got[4]["trace_launches"]
        area = fresh.area_lights(o, d, 4, seed=6, flags=flags)["irradiance"].view(np.uint32).copy()
        fresh.close()
        img, _ = rs.render(cam, num_samples=2, max_bounce=4, flags=native.FLAG_KERNEL_TIMES)
        assert np.array_equal(img, want), f"render before a {path} call"
        prof = rs.context.profile()
        got = call(rs, o, d, 4, 6, flags=flags)
        check_comp(got, comp, path)
        assert got[4]["trace_launches"] == launches[path], (path, got[4], launches)
        assert rs.context.profile() == prof, "zrt_context_profile's record is the last render's"
        img, _ = rs.render(cam, num_samples=2, max_bounce=4, flags=native.FLAG_KERNEL_TIMES)
        assert np.array_equal(img, want), f"render after a {path} call"
        prof = rs.context.profile()
        assert np.array_equal(rs.area_lights(o, d, 4, seed=6, flags=flags)["irradiance"].view(np.uint32), area), path
        got = call(rs, o, d, 4, 6, flags=flags)
        check_comp(got, comp, f"{path} again")
        assert got[4]["trace_launches"] == launches[path], (path, got[4], launches)
        assert rs.context.profile() == prof, "zrt_context_profile's record is the last render's"
    print("sky light launches", launches)
    # first hits: the fast walk + the rest (lane) or pack + park + out + the rest (park); gen; chains: the fast walk +
    # the rest; reduce
    assert launches == {"lane": 2 + 1 + 2 + 1, "park": 4 + 1 + 2 + 1}


def test_empty_and_bad_batches_on_a_live_context(cornell):
    soup, rs = cornell
    ctx = rs.context
    out = np.full(16, 0xABABABAB, np.uint32)
    rays = np.zeros(6, np.float32)
    r, p = rays.ctypes.data, out.ctypes.data
    for flags in (0, native.TRACE_PARK, native.SKY_UNSHADOWED):
        st = ctx.sky_light_raw(0, r, p, p, p, None, False, 4, 16, 0, 0, flags)
        assert st["segments"] == 0 and st["hits"] == 0 and st["samples"] == 0
    ctx.sky_light_raw(0, None, None, None, None, None, False, 4)
    z = np.zeros((0, 3), np.float32)
    res = ctx.sky_light(z, z, 4, hits=True)
    assert res["irradiance"].shape == (0, 3) and res["radiance"].shape == (0, 3) and res["visibility"].shape == (0,) and \
        res["t"].shape == (0,)
    for args, kw in (((None, p, p, p, None, False, 4), {}),
                     ((r, None, None, None, p, False, 4), {}),
                     ((r, p, p, p, None, False, 0), {}), ((r, p, p, p, None, False, 65536), {}),
                     ((r, p, p, p, None, False, 4, 0), {}), ((r, p, p, p, None, False, 4, 257), {}),
                     ((r, p, p, p, None, False, 4, 16), {"flags": native.SEGMENT_ANY}),
                     ((r, p, p, p, None, False, 4, 16), {"flags": native.DIRECT_UNSHADOWED}),
                     ((r, p, p, p, None, False, 4, 16), {"flags": native.AREA_UNSHADOWED}),
                     ((r, p, p, p, None, False, 4, 16), {"flags": 0x4})):
        with pytest.raises(native.ZrtError) as e:
            ctx.sky_light_raw(1, *args, **kw)
        assert e.value.status == -1
    batch = native.SkyLightBatch(1, r, p, p, p, None, 2, 0, 4, 16, 0, 0)                 # on_device > 1
    assert native.lib().zrt_context_sky_light(ctx._h, C.byref(batch), None) == -1
    # the other calls refuse the new bit
    bit = native.SKY_UNSHADOWED
    one = [native.Light.point((0.5, 2.5, -2.5), (1, 1, 1))]
    L = native.lib()
    for refused in (lambda: ctx.direct_raw(1, r, one, p, p, None, False, 16, bit),
                    lambda: ctx.area_lights_raw(1, r, rs.emitters(), p, p, None, False, 4, 16, 0, 0, bit),
                    lambda: ctx.surface_raw(1, r, p, None, False, bit),
                    lambda: ctx.transmittance_raw(1, r, None, p, None, False, bit, 1.0, 16)):
        with pytest.raises(native.ZrtError) as e:
            refused()
        assert e.value.status == -1
    assert L.zrt_context_trace(ctx._h, C.byref(native.RayBatch(1, r, p, 0, bit)), None) == -1
    assert L.zrt_context_segments(ctx._h, C.byref(native.SegmentBatch(1, r, None, p, None, 0, bit, 1.0, 0)), None) == -1
    assert L.zrt_context_occlusion(ctx._h, C.byref(native.OcclusionBatch(1, r, None, p, None, None, 0, bit, 1.0, 4, 0, 0)),
                                   None) == -1
    assert L.zrt_context_radiance(ctx._h, C.byref(native.RadianceBatch(1, r, p, None, 0, bit, 1, 1, 0, 0)), None) == -1
    assert L.zrt_context_light_probes(ctx._h, C.byref(native.LightProbeBatch(1, r, p, None, None, None, None, 0, bit, 4,
                                                                             1, 1, 0, 0, 0)), None) == -1
    assert (out == 0xABABABAB).all()
    ctx.sky_light_raw(1, r, p, out[4:].ctypes.data, out[8:].ctypes.data, out[12:].ctypes.data, False, 4)   # the control
    wrote = np.r_[0:3, 4:7, 8, 12:16]
    assert (out[wrote] != 0xABABABAB).all() and (np.delete(out, wrote) == 0xABABABAB).all()
