"""Direct-light queries (zrt_context_direct) on the GPU, bit for bit --
`irradiance`, `radiance` and the first hits -- against two references:

  the CPU reference (direct_ref.py) on the fuzz seeds' rays and on the
  hand-derived scene of test_direct_host.py;
  the device composition a caller runs today: Context.surface, numpy float32
  light arithmetic in the contract's order, Context.transmittance over exactly
  the traced items, and an ordered numpy sum over the lights.  It needs no CPU
  walk, so it covers every ray and the large shapes.

Every compared call also has to report segments = rays + the chains' segments,
samples = the traced items and hits = the chains' crossings.
"""
import math

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import direct_ref
import test_direct_host as tdh
import test_query_fuzz_gpu as qf
import trace_ref

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"unasked": 0, "lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK,
         "park_bfcull": native.TRACE_PARK | native.FLAG_BFCULL, "mt_exact": native.FLAG_MT_EXACT}
PATHS = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}


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
def vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vnormalize(x):
    """direct_ref.normalize_rn over the last axis of a float32 array."""
    x = np.asarray(x, F)
    inv = F(1.0) / np.sqrt(vdot(x, x))
    return (x * inv[..., None]).astype(F)


def light_items(pos, N, shaded, lights):
    """(w (n, L, 3), b (n, L), f (n, L), traced (n, L)) of the contract, float32."""
    n, L = len(pos), len(lights)
    W, B = np.zeros((n, L, 3), F), np.zeros((n, L), F)
    Fm, TR = np.zeros((n, L), F), np.zeros((n, L), bool)
    for l, lt in enumerate(lights):
        if lt.type == native.LIGHT_DIRECTIONAL:
            dn = np.array([-F(x) for x in lt.direction], F)
            w = np.broadcast_to(vnormalize(dn), (n, 3))
            b = np.full(n, np.inf, F)
            c = vdot(N, w)
            f = c
        else:
            v = (np.array([F(x) for x in lt.position], F) - pos).astype(F)
            d2 = vdot(v, v)
            w = vnormalize(v)
            b = np.sqrt(d2)
            c = vdot(N, w)
            f = c / d2
        tr = shaded & (c > 0)
        if lt.type == native.LIGHT_SPOT:
            s = -vdot(vnormalize(np.array([F(x) for x in lt.direction], F)), w)
            k = s * F(lt.angle_scale) + F(lt.angle_offset)
            k = np.minimum(np.maximum(np.where(np.isnan(k), F(0), k), F(0)), F(1)).astype(F)
            f = f * (k * k)
            tr = tr & (k > 0)
        W[:, l], B[:, l], Fm[:, l], TR[:, l] = w, b, f, tr
    return W, B, Fm, TR


def composition(rs, o, d, lights, cap=16, unshadowed=False, counting=False):
    """{"irradiance", "radiance", "hits" (all bits), "segments", "samples",
    "crossings", "counts"}: what a caller composes today."""
    n, L = len(o), len(lights)
    surf = rs.surface(o, d, hits=True, stats=counting)
    hit = surf["material"] != native.MISS
    pos = np.ascontiguousarray(surf["position"], F)
    with np.errstate(all="ignore"):
        N = vnormalize(surf["normal"])
        shaded = hit & np.isfinite(pos).all(1) & np.isfinite(N).all(1)
        W, B, Fm, TR = light_items(pos, N, shaded, lights)
        T = np.ones((n, L), F)
        segs = cross = 0
        counts = (surf["stats"]["cells_visited"], surf["stats"]["triangle_tests"]) if counting else None
        if not unshadowed:
            po = np.ascontiguousarray(np.broadcast_to(pos[:, None, :], (n, L, 3))[TR])
            tr = rs.transmittance(po, np.ascontiguousarray(W[TR]), np.ascontiguousarray(B[TR]), max_crossings=cap,
                                  stats=counting)
            T[TR] = tr["transmittance"]
            segs, cross = tr["stats"]["segments"], tr["stats"]["hits"]
            if counting:
                counts = (counts[0] + tr["stats"]["cells_visited"], counts[1] + tr["stats"]["triangle_tests"])
        E = np.zeros((n, 3), F)
        for l, lt in enumerate(lights):
            g = (Fm[:, l] * T[:, l]).astype(F)
            add = (np.array([F(x) for x in lt.color], F)[None, :] * g[:, None]).astype(F)
            E = np.where(TR[:, l][:, None], (E + add).astype(F), E)
        R = np.zeros((n, 3), F)
        lit = (surf["emissive"] + (surf["base_color"] * E).astype(F) * direct_ref.INV_PI).astype(F)
        R[hit] = np.where(shaded[:, None], lit, surf["emissive"])[hit]
    return {"irradiance": E.view(np.uint32), "radiance": R.view(np.uint32), "hits": trace_ref.hit_bits(surf),
            "segments": int(segs), "samples": int(TR.sum()), "crossings": int(cross), "counts": counts,
            "shaded": shaded, "hit": hit}


def call(rs, o, d, lights, cap=16, flags=0, device=False, stats=False, unshadowed=False):
    """Context.direct with host arrays or, `device`, torch tensors, as
    (irradiance bits, radiance bits, hit bits, stats)."""
    if device:
        dev = torch.device("cuda", 0)
        res = rs.direct(torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev),
                        lights, max_crossings=cap, flags=flags, unshadowed=unshadowed, radiance=True, hits=True, stats=stats)
        return (res["irradiance"].cpu().numpy().view(np.uint32), res["radiance"].cpu().numpy().view(np.uint32),
                res["hits"].cpu().numpy().view(np.uint32), res["stats"])
    res = rs.direct(o, d, lights, max_crossings=cap, flags=flags, unshadowed=unshadowed, radiance=True, hits=True,
                    stats=stats)
    return res["irradiance"].view(np.uint32), res["radiance"].view(np.uint32), trace_ref.hit_bits(res), res["stats"]


def check(got, want_E, want_R, want_hits, segments, samples, crossings, what):
    E, R, hits, st = got
    bad = np.nonzero((E != want_E).any(axis=1) | (R != want_R).any(axis=1) | (hits != want_hits).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rays differ, first {bad[0]}: got E {[hex(int(x)) for x in E[bad[0]]]} "
                           f"radiance {[hex(int(x)) for x in R[bad[0]]]} hit {[hex(int(x)) for x in hits[bad[0]]]}, "
                           f"reference {[hex(int(x)) for x in want_E[bad[0]]]} {[hex(int(x)) for x in want_R[bad[0]]]} "
                           f"{[hex(int(x)) for x in want_hits[bad[0]]]}")
    assert (st["segments"], st["samples"], st["hits"]) == (len(E) + segments, samples, crossings), (what, st)


def check_comp(got, comp, what):
    check(got, comp["irradiance"], comp["radiance"], comp["hits"], comp["segments"], comp["samples"], comp["crossings"],
          what)


def use_device(seed):
    """Host and device pointers alternate by seed pair."""
    return torch is not None and torch.cuda.is_available() and (seed // 2) % 2 == 1


# ------------------------------------------------------------------ the seeds
@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_direct_matches_both_references(seed, case, context):
    cs, rs = case(seed), context(seed)
    lights, rays = direct_ref.cached_rays(cs)
    dev = use_device(seed)
    what = f"seed {seed}, {cs.soup.num_triangles} triangles, grid {cs.res}"
    for cap in (16, 1, 2):
        E, R, tot = direct_ref.direct_batch(cs.ref, cs.soup, rays, lights, cap, counts=True)
        comp = composition(rs, cs.o, cs.d, lights, cap, counting=True)
        assert np.array_equal(comp["irradiance"], E) and np.array_equal(comp["radiance"], R), f"{what}: composition"
        assert np.array_equal(comp["hits"], cs.bits), f"{what}: composition"
        assert (comp["segments"], comp["samples"], comp["crossings"]) == (tot["segments"], tot["samples"], tot["hits"])
        for mode, flags in (MODES if cap == 16 else {"unasked": 0}).items():
            check(call(rs, cs.o, cs.d, lights, cap, flags=flags, device=dev), E, R, cs.bits, tot["segments"],
                  tot["samples"], tot["hits"], f"{what}, cap {cap}, {mode}")
        got = call(rs, cs.o, cs.d, lights, cap, device=dev, stats=True)
        check(got, E, R, cs.bits, tot["segments"], tot["samples"], tot["hits"], f"{what}, cap {cap}, counting")
        want = (cs.counts[0] + tot["cells"], cs.counts[1] + tot["tests"])
        assert (got[3]["cells_visited"], got[3]["triangle_tests"]) == want == comp["counts"], (what, cap, got[3], want)
    E, R, tot = direct_ref.direct_batch(cs.ref, cs.soup, rays, lights, unshadowed=True)
    for mode, flags in PATHS.items():
        check(call(rs, cs.o, cs.d, lights, flags=flags, device=dev, unshadowed=True), E, R, cs.bits, 0, tot["samples"], 0,
              f"{what}, unshadowed, {mode}")


def test_the_hand_derived_scene(oracle_mod):
    soup = tdh.hand_soup()
    ref = trace_ref.RayRef(oracle_mod, soup, (4, 4, 4))
    o, d = tdh.hand_rays()
    bits, _ = ref.trace_batch(o, d)
    lights = tdh.hand_lights()
    rays = [direct_ref.Ray(ref, soup, o[i], d[i], bits[i], lights) for i in range(len(o))]
    rs = RenderScene(soup, (4, 4, 4), device=0)
    try:
        for cap in (16, 1):
            E, R, tot = direct_ref.direct_batch(ref, soup, rays, lights, cap)
            for mode, flags in MODES.items():
                check(call(rs, o, d, lights, cap, flags=flags), E, R, bits, tot["segments"], tot["samples"], tot["hits"],
                      f"hand scene, cap {cap}, {mode}")
        want, tol = tdh.hand_E64(lights)
        got = call(rs, o, d, lights)[0].view(F).astype(np.float64)
        assert (np.abs(got - want) <= tol).all()
    finally:
        rs.close()


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


def box_lights(soup, L, seed):
    """L lights in and around the soup's box: points, directionals and spots in turn."""
    rng = np.random.default_rng(seed)
    p = np.asarray(soup.pos, np.float64).reshape(-1, 3)
    lo, ext = p.min(0), p.max(0) - p.min(0)
    out = []
    for l in range(L):
        at = lo + (0.1 + 0.8 * rng.random(3)) * ext
        aim = rng.normal(size=3)
        col = 0.25 + rng.random(3) * 4
        if l % 3 == 0:
            out.append(native.Light.point(at, col))
        elif l % 3 == 1:
            out.append(native.Light.directional(aim * rng.choice([0.01, 1.0, 50.0]), col / 8))
        else:
            out.append(native.Light.spot(at, aim, col, math.radians(25), math.radians(60)))
    return out


def guarded_call(rs, o, d, lights, flags, want_E=True, want_R=True, want_hits=True, cap=16):
    """direct_raw on host arrays between guard words; (irradiance bits, radiance bits, hit bits, stats), None for an
    output that was not asked for."""
    n = len(o)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    E = np.full(3 * (n + 2), 0xABABABAB, np.uint32)
    R = np.full(3 * (n + 2), 0xCDCDCDCD, np.uint32)
    hit = np.full(4 * (n + 2), 0xEFEFEFEF, np.uint32)
    st = rs.context.direct_raw(n, rays.ctypes.data, lights, E[3:].ctypes.data if want_E else None,
                               R[3:].ctypes.data if want_R else None, hit[4:].ctypes.data if want_hits else None, False,
                               cap, flags)
    for a, w, g in ((E, 3, 0xABABABAB), (R, 3, 0xCDCDCDCD), (hit, 4, 0xEFEFEFEF)):
        assert (a[:w] == g).all() and (a[-w:] == g).all(), "guard words"
    assert want_E or (E == 0xABABABAB).all()
    assert want_R or (R == 0xCDCDCDCD).all()
    assert want_hits or (hit == 0xEFEFEFEF).all()
    return (E[3:-3].reshape(n, 3) if want_E else None, R[3:-3].reshape(n, 3) if want_R else None,
            hit[4:-4].reshape(n, 4) if want_hits else None, st)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_ray_and_light_counts_between_guard_words(n, cornell):
    soup, rs = cornell
    o, d = box_rays(soup, n, 100 + n)
    for L in (1, 2, 63, 64, 65):
        lights = box_lights(soup, L, 200 + L)
        comp = composition(rs, o, d, lights)
        if n >= 63 and L >= 2:
            assert 0 < comp["samples"] < n * L and comp["irradiance"].any()
        for path, flags in PATHS.items():
            check_comp(guarded_call(rs, o, d, lights, flags), comp, f"n = {n}, L = {L}, {path}")


def test_a_ray_whose_lights_straddle_the_sub_chunk_cut(cornell):
    """4099 rays x 257 lights = 1,053,443 items: one cut at item 2^20, inside
    ray 4080, whose lights 0..15 fall before it and 16..256 after it."""
    soup, rs = cornell
    n, L = 4099, 257
    assert (1 << 20) // L == 4080 and (1 << 20) % L == 16 and n * L > 1 << 20
    o, d = box_rays(soup, n, 5)
    o[4080], d[4080] = (0.5, 2.5, -4.5), (0, -1, 0)                 # straight down onto the floor
    lights = box_lights(soup, L, 11)
    comp = composition(rs, o, d, lights)
    s = rs.surface(o[4080:4081], d[4080:4081])
    TR = light_items(np.ascontiguousarray(s["position"], F), vnormalize(s["normal"]), s["material"] != native.MISS,
                     lights)[3]
    assert TR[0, :16].sum() >= 3 and TR[0, 16:].sum() >= 8, "the straddling ray has traced lights on both sides of the cut"
    assert comp["irradiance"][4080].view(F).min() > 0
    for path, flags in list(PATHS.items()) + [("unasked", 0)]:
        check_comp(call(rs, o, d, lights, flags=flags), comp, f"4099 x 257, {path}")


def test_torch_tensors_in_place_across_the_ray_chunk_cut(cornell):
    """2^20 + 77 rays x 1 light on the device: two chunks of rays."""
    if torch is None or not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    soup, rs = cornell
    n = (1 << 20) + 77
    o, d = box_rays(soup, n, 6)
    lights = box_lights(soup, 1, 3)
    comp = composition(rs, o, d, lights)
    dev = torch.device("cuda", 0)
    before = torch.arange(4096, dtype=torch.int32, device=dev)
    for path, flags in PATHS.items():
        got = call(rs, o, d, lights, flags=flags, device=True)
        after = torch.full((4096,), 5, dtype=torch.int32, device=dev)
        check_comp(got, comp, f"2^20 + 77 rays, {path}")
        assert torch.equal(before.cpu(), torch.arange(4096, dtype=torch.int32)) and bool((after == 5).all())
    assert comp["irradiance"][1 << 20:].any() and comp["irradiance"][:1 << 20].any()


def test_a_host_batch_across_the_ray_chunk_cut(cornell):
    """2^20 + 77 host rays x 1 light: two chunks, the light staged behind a
    whole chunk's rays.  The rays around the cut against a call on those 205
    alone, bit for bit; the totals from the 128 rays the batch tiles."""
    soup, rs = cornell
    n = (1 << 20) + 77
    o128, d128 = box_rays(soup, 128, 6)
    idx = np.arange(n) % 128
    o, d = np.ascontiguousarray(o128[idx]), np.ascontiguousarray(d128[idx])
    lights = box_lights(soup, 1, 3)
    tile, rest = composition(rs, o128, d128, lights), composition(rs, o128[:77], d128[:77], lights)
    want = {k: (n // 128) * tile[k] + rest[k] for k in ("segments", "samples", "crossings")}
    assert rest["samples"] > 0 and tile["irradiance"][64:].any()
    lo = (1 << 20) - 128
    for path, flags in PATHS.items():
        E, R, hits, st = call(rs, o, d, lights, flags=flags)
        near = call(rs, o[lo:], d[lo:], lights, flags=flags)
        check((E[lo:], R[lo:], hits[lo:], near[3]), near[0], near[1], near[2], near[3]["segments"] - 205,
              near[3]["samples"], near[3]["hits"], f"around the cut, {path}")
        print("direct segments", path, st["segments"], n + want["segments"])
        assert (st["segments"], st["samples"], st["hits"]) == (n + want["segments"], want["samples"], want["crossings"]), path


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_launches_of_one_small_chunk(device, case, context):
    """A seed's 128 rays x its 4 lights, one chunk and one sub-chunk:
    zrt_stats.trace_launches per mode, as the sequence in zrt_context_direct's
    comment gives them (recorded on the GPU at the commit before the query
    calls came to share their host code)."""
    if device and (torch is None or not torch.cuda.is_available()):
        pytest.skip("torch sees no device")
    cs, rs = case(18), context(18)
    lights, rays = direct_ref.cached_rays(cs)
    E, R, tot = direct_ref.direct_batch(cs.ref, cs.soup, rays, lights)
    assert len(lights) == 4 and tot["samples"] > 0
    want = {"lane": 2 + 1 + 2 + 1,                  # first hits: the fast walk + the rest; gen; chains: the fast walk +
                                                    # the rest; reduce
            "park": 4 + 1 + 2 + 1,                  # first hits: pack + park + out + the rest; gen; chains; reduce
            "counting": 1 + 1 + 1 + 1,              # first hits: the counting walk; gen; the counting chain walk; reduce
            "lane unshadowed": 2 + 1 + 1,           # first hits; gen; reduce: no chain is walked
            "park unshadowed": 4 + 1 + 1,
            "counting unshadowed": 1 + 1 + 1}
    got = {}
    for mode, kw in (("lane", {"flags": native.FLAG_LANE_WALK}), ("park", {"flags": native.TRACE_PARK}),
                     ("counting", {"stats": True})):
        res = call(rs, cs.o, cs.d, lights, device=device, **kw)
        check(res, E, R, cs.bits, tot["segments"], tot["samples"], tot["hits"], f"128 rays, {mode}")
        got[mode] = res[3]["trace_launches"]
        got[mode + " unshadowed"] = call(rs, cs.o, cs.d, lights, device=device, unshadowed=True, **kw)[3]["trace_launches"]
    print("direct launches", "device" if device else "host", got)
    assert got == want


def test_output_subsets_leave_the_other_arrays_alone(cornell):
    soup, rs = cornell
    o, d = box_rays(soup, 300, 8)
    lights = box_lights(soup, 5, 9)
    comp = composition(rs, o, d, lights)
    for path, flags in PATHS.items():
        for want_E, want_R in ((True, False), (False, True), (True, True)):
            for want_hits in (False, True):
                E, R, hit, st = guarded_call(rs, o, d, lights, flags, want_E, want_R, want_hits)
                what = (path, want_E, want_R, want_hits)
                assert E is None or np.array_equal(E, comp["irradiance"]), what
                assert R is None or np.array_equal(R, comp["radiance"]), what
                assert hit is None or np.array_equal(hit, comp["hits"]), what
                assert (st["segments"], st["samples"], st["hits"]) == (300 + comp["segments"], comp["samples"],
                                                                       comp["crossings"]), what


def test_unshadowed_against_numpy_alone(cornell):
    soup, rs = cornell
    o, d = box_rays(soup, 3000, 12)
    lights = box_lights(soup, 7, 13)
    comp = composition(rs, o, d, lights, unshadowed=True)
    lit = composition(rs, o, d, lights)
    assert comp["segments"] == 0 and comp["samples"] == lit["samples"] and not np.array_equal(comp["irradiance"], lit["irradiance"])
    for mode, flags in MODES.items():
        got = call(rs, o, d, lights, flags=flags, unshadowed=True)
        check_comp(got, comp, f"unshadowed, {mode}")
        # no walk launch: a lane-walk call is the first hits' two launches, the gen and the reduce launch
        assert mode != "lane" or got[3]["trace_launches"] == 4, got[3]


# ----------------------------------------------------------- odd inputs
def test_hits_on_nan_infinite_and_huge_normals(case, oracle_mod):
    """direct_ref.PoisonedCase of seed 4: a hit on a NaN or infinite normal is
    not shaded; one on a 3e38 normal has N = 0 and no light in front of it.
    None has a traced item, and the radiance of each is the emission."""
    cs = direct_ref.PoisonedCase(oracle_mod, case(tdh.POISON_SEED))
    lights = direct_ref.fuzz_lights(cs.soup)
    rays = [direct_ref.Ray(cs.ref, cs.soup, cs.o[i], cs.d[i], cs.bits[i], lights) for i in range(len(cs.o))]
    E, R, tot = direct_ref.direct_batch(cs.ref, cs.soup, rays, lights)
    odd = np.array([r.words is not None and int(cs.ref.indices[int(cs.bits[i, 3])]) in cs.poisoned
                    for i, r in enumerate(rays)])
    assert odd.sum() >= 3 and sum(not rays[i].shaded for i in np.nonzero(odd)[0]) >= 2
    assert all(not any(it.traced for it in rays[i].items) for i in np.nonzero(odd)[0])
    rs = RenderScene(cs.soup, cs.res, device=0, device_build=cs.device_build)
    try:
        emis = rs.surface(cs.o, cs.d)["emissive"].view(np.uint32)
        comp = composition(rs, cs.o, cs.d, lights)
        assert np.array_equal(comp["irradiance"], E) and np.array_equal(comp["radiance"], R)
        assert comp["samples"] == tot["samples"]
        for mode, flags in MODES.items():
            got = call(rs, cs.o, cs.d, lights, flags=flags)
            check(got, E, R, cs.bits, tot["segments"], tot["samples"], tot["hits"], f"odd normals, {mode}")
            assert not got[0][odd].any() and np.array_equal(got[1][odd], emis[odd]), mode
        got = call(rs, cs.o, cs.d, lights, stats=True)
        ccomp = composition(rs, cs.o, cs.d, lights, counting=True)
        assert (got[3]["cells_visited"], got[3]["triangle_tests"]) == ccomp["counts"]
    finally:
        rs.close()


def test_non_finite_light_fields_are_taken_as_given(cornell):
    soup, rs = cornell
    o, d = box_rays(soup, 2000, 14)
    nan, inf = float("nan"), float("inf")
    odd = [native.Light.point((nan, 0, 0), (1, 1, 1)), native.Light.point((inf, 0, 0), (1, 1, 1)),
           native.Light.point((-inf, inf, 0), (1, 1, 1)), native.Light.point((3e38, 3e38, 0), (1, 1, 1)),
           native.Light.directional((0, 0, 0), (1, 1, 1)), native.Light.directional((inf, 0, 0), (1, 1, 1)),
           native.Light.directional((nan, 1, 0), (1, 1, 1)),
           native.Light.spot((0.5, 2.5, -2.5), (0, 0, 0), (1, 1, 1), 0.3, 0.6),
           native.Light.spot((inf, 2.5, -2.5), (0, -1, 0), (1, 1, 1), 0.3, 0.6)]
    comp = composition(rs, o, d, odd)
    assert comp["samples"] == 0 and not comp["irradiance"].any() and comp["hit"].sum() > 1000
    for path, flags in PATHS.items():
        check_comp(call(rs, o, d, odd, flags=flags), comp, f"odd lights, {path}")
    # among ordinary lights they add nothing; a NaN colour or spot number on a traced item is stored as it comes
    good = box_lights(soup, 3, 15)
    mixed = [odd[0], good[0], odd[4], good[1], odd[7], good[2]]
    a, b = composition(rs, o, d, mixed), composition(rs, o, d, good)
    assert np.array_equal(a["irradiance"], b["irradiance"]) and a["samples"] == b["samples"] > 0
    nan_col = native.Light.point((0.5, 2.5, -2.5), (nan, 1, inf))
    nan_spot = native.Light.spot((0.5, 2.5, -2.5), (0, -1, 0), (1, 1, 1), 0.3, 0.6)
    nan_spot.angle_scale = nan
    c = composition(rs, o, d, good + [nan_col, nan_spot])
    assert np.isnan(c["irradiance"].view(F)[:, 0]).any() and np.isinf(c["irradiance"].view(F)[:, 2]).any()
    for path, flags in PATHS.items():
        check_comp(call(rs, o, d, mixed, flags=flags), a, f"mixed lights, {path}")
        check_comp(call(rs, o, d, good + [nan_col, nan_spot], flags=flags), c, f"NaN colour, {path}")


# ------------------------------------------------------------------------ other
def test_direct_renders_and_transmittance_share_a_context_cleanly(cornell):
    soup, rs = cornell
    cam = camera_for(soup, None, 24, 24)
    fresh = RenderScene(soup, (16, 16, 16), device=0)
    want, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    o, d = box_rays(soup, 3000, 21)
    lights = box_lights(soup, 4, 22)
    comp = composition(rs, o, d, lights)
    tm = rs.transmittance(o, d, 0.5)["transmittance"].view(np.uint32)
    for path, flags in PATHS.items():
        img, _ = rs.render(cam, num_samples=2, max_bounce=4, flags=native.FLAG_KERNEL_TIMES)
        assert np.array_equal(img, want), f"render before a {path} direct call"
        prof = rs.context.profile()
        check_comp(call(rs, o, d, lights, flags=flags), comp, path)
        assert rs.context.profile() == prof, "zrt_context_profile's record is the last render's"
        img, _ = rs.render(cam, num_samples=2, max_bounce=4)
        assert np.array_equal(img, want), f"render after a {path} direct call"
        assert np.array_equal(rs.transmittance(o, d, 0.5, flags=flags)["transmittance"].view(np.uint32), tm), path
        check_comp(call(rs, o, d, lights, flags=flags), comp, f"{path} again")


def test_empty_and_bad_batches_on_a_live_context(cornell):
    ctx = cornell[1].context
    out = np.full(16, 0xABABABAB, np.uint32)
    rays = np.zeros(6, np.float32)
    r, p = rays.ctypes.data, out.ctypes.data
    one = [native.Light.point((0.5, 2.5, -2.5), (1, 1, 1))]
    bad = [native.Light.point((0.5, 2.5, -2.5), (1, 1, 1))]
    bad[0].type = 7
    for flags in (0, native.TRACE_PARK, native.DIRECT_UNSHADOWED):
        st = ctx.direct_raw(0, r, one, p, p, None, False, 16, flags)
        assert st["segments"] == 0 and st["hits"] == 0 and st["samples"] == 0
    ctx.direct_raw(0, None, one, None, None, None, False)
    z = np.zeros((0, 3), np.float32)
    res = ctx.direct(z, z, one, radiance=True, hits=True)
    assert res["irradiance"].shape == (0, 3) and res["radiance"].shape == (0, 3) and res["t"].shape == (0,)
    for args, kw in (((None, one, p, p, None, False), {}), ((r, [], p, p, None, False), {}),
                     ((r, one, None, None, p, False), {}), ((r, bad, p, p, None, False), {}),
                     ((r, one, p, p, None, False, 0), {}), ((r, one, p, p, None, False, 257), {}),
                     ((r, one, p, p, None, False, 16), {"flags": native.SEGMENT_ANY}),
                     ((r, one, p, p, None, False, 16), {"flags": 0x4})):
        with pytest.raises(native.ZrtError) as e:
            ctx.direct_raw(1, *args, **kw)
        assert e.value.status == -1
    assert (out == 0xABABABAB).all()
    ctx.direct_raw(1, r, one, p, out[4:].ctypes.data, out[8:].ctypes.data, False)   # the control: the valid batch runs
