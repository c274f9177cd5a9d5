"""Area-light queries on the GPU, bit for bit.

The set (zrt_emitters_read's records, C and Q) against area_light_ref.EmitterSet
on seeded soups past one scan block and past one scan level, on materials whose
emissive textures hold NaN, negative and infinite texels, and on the fuzz seeds.

The call -- `irradiance`, `radiance` and the first hits, and segments, samples
and hits in every call -- against two references:

  the CPU reference (area_light_ref.py) on the fuzz seeds' rays and on the
  hand-derived scene of test_area_lights_host.py;
  a device composition that needs no CPU walk: Context.surface, the item
  arithmetic in numpy float32 over whole arrays (the stream's words and the
  64 x 64 -> high 64 product on uint64 arrays), Context.transmittance over
  exactly the traced items, and an ordered numpy sum over the samples.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import area_light_ref as alr
import test_area_lights_host as tah
import test_query_fuzz_gpu as qf
import trace_ref
from direct_ref import INV_PI
from test_direct_gpu import MODES, PATHS, box_rays, use_device, vdot, vnormalize

pytestmark = pytest.mark.gpu

F = np.float32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
GOLDEN = U64(0x9E3779B97F4A7C15)


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


# -------------------------------------------------------------------- the set
def check_set(em, want, what):
    rec, pre = em.read()
    n, q, _ = em.info()
    assert (n, q) == (want.count, want.Q), (what, n, q, want.count, want.Q)
    assert rec.tobytes() == want.records.tobytes(), f"{what}: records differ"
    assert np.array_equal(pre, want.C), f"{what}: C differs"


def set_soup():
    """test_area_lights_host.hand_soup with five materials more: 3 a 1x1 emitter,
    4 a 37x5 emissive texture with a NaN, a negative and many small texels (its
    maximum 3), 5 a 37x5 one with an inf texel (w is infinite: no emitter), 6 a
    1x1 of NaN, a negative and -0 (m = 0: no emitter), 7 a 37x5 one that is all
    NaN or negative."""
    soup = tah.hand_soup()
    rng = np.random.default_rng(77)
    texels = list(soup.texels)
    desc = np.zeros((8, 3, 7), np.int32)
    desc[:3] = soup.tex_desc

    def push(vals):
        off = len(texels)
        texels.extend(float(v) for v in vals)
        return off

    def big(special):
        t = rng.random(37 * 5 * 3).astype(F)
        for at, v in special:
            t[at] = v
        return t

    emis = {3: ([0.5, 2.0, 1.0], 1, 1),
            4: (big([(0, np.nan), (7, -5.0), (554, 3.0), (300, -np.inf)]), 37, 5),
            5: (big([(100, np.inf), (3, np.nan)]), 37, 5),
            6: ([np.nan, -2.0, -0.0], 1, 1),
            7: (np.where(rng.random(555) < 0.5, np.nan, -1.0), 37, 5)}
    for m, (vals, w, h) in emis.items():
        desc[m, 0] = (push([0.5, 0.5, 0.5]), 1, 1, 0, 0, 0, 0)
        desc[m, 1] = (push(vals), w, h) + ((0, 0, 0, 0) if w == 1 else (-2 ** 31, 2 ** 31 - 1, 0, h - 1))
        desc[m, 2] = (push([1.0]), 1, 1, 0, 0, 0, 0)
    return dataclasses.replace(soup, materials=[scenes.Material()] * 8, tex_desc=desc, texels=np.asarray(texels, F))


@pytest.fixture(scope="module")
def set_scene():
    soup = set_soup()
    rs = RenderScene(soup, (4, 4, 4), device=0)
    yield soup, rs
    rs.close()


def random_soup(n, seed, emitting):
    """n triangles, `emitting` of them (about) on the emitting materials 2, 3
    and 4, the others on 0, 1, 5, 6 and 7; some degenerate, some huge."""
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(n, 9)) * rng.choice([0.01, 1.0, 30.0], (n, 1))).astype(F)
    pos[rng.random(n) < 0.02, 3:] = 0                                  # zero area
    uv = rng.random((n, 6)).astype(F)
    em = rng.random(n) < emitting
    mat = np.where(em, rng.choice([2, 3, 4], n), rng.choice([0, 1, 5, 6, 7], n)).astype(np.uint32)
    return pos, uv, mat


@pytest.mark.parametrize("n", [1, 64, 65, 1025, 70001])
def test_the_set_matches_the_reference(n, set_scene):
    """1: one emitter or none; 64, 65: a wave's edge; 1025: five scan blocks;
    70,001: 274 blocks, so the block sums take a second level of two blocks."""
    soup, rs = set_scene
    mm = alr.material_max(soup.tex_desc, soup.texels)
    assert list(mm) == [0, 0, 4, 2, 3, np.inf, 0, 0]
    for k, frac in enumerate((0.0, 0.3, 1.0)):
        pos, uv, mat = random_soup(n, 1000 * n + k, frac)
        want = alr.EmitterSet(pos, uv, mat, soup.tex_desc, soup.texels)
        assert (want.count == 0) if frac == 0 else (want.count > 0.5 * n * frac - 1), (n, frac, want.count)
        em = native.Emitters(rs.context, pos, uv, mat)
        check_set(em, want, f"{n} triangles, {frac}")
        assert em.info()[2] == n
        em.close()
    # null texcoords are zeros
    pos, uv, mat = random_soup(n, 5, 0.5)
    em = native.Emitters(rs.context, pos, None, mat)
    check_set(em, alr.EmitterSet(pos, None, mat, soup.tex_desc, soup.texels), f"{n} triangles, no texcoords")
    em.close()


def test_the_empty_set_and_bad_arguments(set_scene):
    soup, rs = set_scene
    em = native.Emitters(rs.context, np.zeros((0, 9), F), None, np.zeros(0, np.uint32))
    assert em.info() == (0, 0, 0) and len(em.read()[0]) == 0
    em.close()
    L = native.lib()
    pos, mat, out = np.zeros(9, F), np.array([8], np.uint32), C.c_void_p(0x1234)
    assert L.zrt_emitters_create(rs.context._h, pos.ctypes.data, None, mat.ctypes.data, 1, C.byref(out)) == -1   # 8 materials
    assert L.zrt_emitters_create(rs.context._h, None, None, mat.ctypes.data, 1, C.byref(out)) == -1
    assert L.zrt_emitters_create(rs.context._h, pos.ctypes.data, None, None, 1, C.byref(out)) == -1
    assert L.zrt_emitters_create(rs.context._h, pos.ctypes.data, None, mat.ctypes.data, 1, None) == -1
    assert out.value == 0x1234


@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_sets_match_the_reference(seed, case, context):
    cs, rs = case(seed), context(seed)
    check_set(rs.emitters(), tah.fuzz_set(cs), f"seed {seed}")


# ------------------------------------------------------------ the composition
def mix64(z):
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def stream_words(seed, keys, S):
    """(3, n, S) uint64: the first three words of the streams (seed, keys[i], s)."""
    with np.errstate(over="ignore"):
        pix = (keys.astype(U64)[:, None] << U64(16)) | np.arange(S, dtype=U64)[None, :]
        s = mix64(pix ^ mix64(np.array([seed & (2 ** 64 - 1)], U64) + GOLDEN))
        out = []
        for _ in range(3):
            s = s + GOLDEN
            out.append(mix64(s))
    return np.stack(out)


def mulhi(x, q):
    """The high 64 bits of x * q, uint64 arrays."""
    q = U64(q)
    with np.errstate(over="ignore"):
        al, ah, bl, bh = x & M32, x >> U64(32), q & M32, q >> U64(32)
        p0, p1, p2, p3 = al * bl, al * bh, ah * bl, ah * bh
        carry = ((p0 >> U64(32)) + (p1 & M32) + (p2 & M32)) >> U64(32)
        return p3 + (p1 >> U64(32)) + (p2 >> U64(32)) + carry


def texel_1x1(es, mat, slot, chans):
    """The texels of materials whose `slot` texture is 1x1 (a finite texture
    coordinate samples a 1x1 texture to its texel exactly: lerp(x, x, t) = x)."""
    d = es.tex_desc[:, slot]
    assert (d[np.unique(mat), 1:3] == 1).all(), "the composition samples 1x1 textures only"
    return es.texels[d[mat, 0][..., None] + np.arange(chans)]


def sampled(orc, es, mat, slot, chans, s, t):
    """... and of any texture, one oracle call per item (small batches)."""
    out = np.zeros(mat.shape + (chans,), F)
    for idx in np.ndindex(mat.shape):
        out[idx] = alr._tex(orc, es, int(mat[idx]), slot, s[idx], t[idx])
    return out


def items(es, pos, N, shaded, S, seed, keys, orc=None):
    """(w (n, S, 3), b (n, S), con (n, S, 3), traced (n, S)) of the contract, float32."""
    n = len(pos)
    x0, x1, x2 = stream_words(seed, keys, S)
    k = np.searchsorted(es.C, mulhi(x0, es.Q), side="right") - 1
    r = es.records[k]
    with np.errstate(all="ignore"):
        bu, bv = (x1 >> U64(40)).astype(F) * alr.INV24, (x2 >> U64(40)).astype(F) * alr.INV24
        fold = (bu + bv) > 1
        bu, bv = np.where(fold, F(1) - bu, bu), np.where(fold, F(1) - bv, bv)
        v0, e1, e2, tc = r["v0"], r["e1"], r["e2"], r["texcoords"]
        y = (v0 + e1 * bu[..., None]) + e2 * bv[..., None]
        w0 = (F(1) - bu) - bv
        s, t = [(tc[..., j] * w0 + tc[..., 2 + j] * bu) + tc[..., 4 + j] * bv for j in range(2)]
        if orc is None:
            Le, alpha = texel_1x1(es, r["material"], 1, 3), texel_1x1(es, r["material"], 2, 1)[..., 0]
        else:
            Le, alpha = sampled(orc, es, r["material"], 1, 3, s, t), sampled(orc, es, r["material"], 2, 1, s, t)[..., 0]
        v = (y - pos[:, None, :]).astype(F)
        d2 = vdot(v, v)
        w = vnormalize(v)
        c = vdot(np.broadcast_to(N[:, None, :], (n, S, 3)), w)
        ne = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                       e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
        cl = -vdot(vnormalize(ne), w)
        traced = shaded[:, None] & (c > 0) & (cl > 0)
        g = ((c * cl) / d2) * ((F(es.Q) / r["q"].astype(F)) * r["a"])
        con = (Le * alpha[..., None]) * g[..., None]
        b = np.sqrt(d2) * alr.SHORT
    return w, b.astype(F), con.astype(F), traced


def composition(rs, es, o, d, S, seed=0, index_base=0, cap=16, unshadowed=False, counting=False, orc=None):
    n = len(o)
    surf = rs.surface(o, d, hits=True, stats=counting)
    hit = surf["material"] != native.MISS
    pos = np.ascontiguousarray(surf["position"], F)
    keys = ((index_base + np.arange(n, dtype=np.uint64)) & M32).astype(np.uint32)
    with np.errstate(all="ignore"):
        N = vnormalize(surf["normal"])
        shaded = hit & np.isfinite(pos).all(1) & np.isfinite(N).all(1)
        segs = cross = 0
        counts = (surf["stats"]["cells_visited"], surf["stats"]["triangle_tests"]) if counting else None
        E = np.zeros((n, 3), F)
        TR = np.zeros((n, S), bool)
        if es.count:
            W, B, con, TR = items(es, pos, N, shaded, S, seed, keys, orc)
            T = np.ones((n, S), F)
            if not unshadowed and TR.any():
                po = np.ascontiguousarray(np.broadcast_to(pos[:, None, :], (n, S, 3))[TR])
                tr = rs.transmittance(po, np.ascontiguousarray(W[TR]), np.ascontiguousarray(B[TR]), max_crossings=cap,
                                      stats=counting)
                T[TR] = tr["transmittance"]
                segs, cross = tr["stats"]["segments"], tr["stats"]["hits"]
                if counting:
                    counts = (counts[0] + tr["stats"]["cells_visited"], counts[1] + tr["stats"]["triangle_tests"])
            for s in range(S):
                E = np.where(TR[:, s][:, None], (E + (con[:, s] * T[:, s][:, None]).astype(F)).astype(F), E)
        E = np.where(hit[:, None], (E / F(S)).astype(F), F(0))
        R = np.zeros((n, 3), F)
        lit = (surf["emissive"] + (surf["base_color"] * E).astype(F) * INV_PI).astype(F)
        R[hit] = np.where(shaded[:, None], lit, surf["emissive"])[hit]
    return {"irradiance": E.view(np.uint32), "radiance": R.view(np.uint32), "hits": trace_ref.hit_bits(surf),
            "segments": int(segs), "samples": int(TR.sum()), "crossings": int(cross), "counts": counts, "traced": TR,
            "hit": hit}


def call(rs, em, o, d, S, seed=0, index_base=0, cap=16, flags=0, device=False, stats=False, unshadowed=False):
    """Context.area_lights with host arrays or, `device`, torch tensors, as
    (irradiance bits, radiance bits, hit bits, stats)."""
    kw = dict(max_crossings=cap, seed=seed, index_base=index_base, flags=flags, unshadowed=unshadowed, radiance=True,
              hits=True, stats=stats)
    if device:
        dev = torch.device("cuda", 0)
        res = rs.context.area_lights(torch.from_numpy(np.ascontiguousarray(o)).to(dev),
                                     torch.from_numpy(np.ascontiguousarray(d)).to(dev), em, S, **kw)
        return (res["irradiance"].cpu().numpy().view(np.uint32), res["radiance"].cpu().numpy().view(np.uint32),
                res["hits"].cpu().numpy().view(np.uint32), res["stats"])
    res = rs.context.area_lights(o, d, em, S, **kw)
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


# ------------------------------------------------------------------ the seeds
@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_area_lights_match_both_references(seed, case, context, oracle_mod):
    cs, rs = case(seed), context(seed)
    es, rays = tah.fuzz_set(cs), tah.cached_rays(oracle_mod, cs)
    em = rs.emitters()
    S, dev = tah.FUZZ_SPP, use_device(seed)
    what = f"seed {seed}, {cs.soup.num_triangles} triangles, {es.count} emitters, grid {cs.res}"
    for cap in (16, 1, 2):
        E, R, tot = alr.area_batch(cs.ref, cs.soup, rays, S, cap, counts=True)
        comp = composition(rs, es, cs.o, cs.d, S, seed=cs.seed, cap=cap, counting=True, orc=oracle_mod)
        assert np.array_equal(comp["irradiance"], E) and np.array_equal(comp["radiance"], R), f"{what}: composition"
        assert np.array_equal(comp["hits"], cs.bits), f"{what}: composition"
        assert (comp["segments"], comp["samples"], comp["crossings"]) == (tot["segments"], tot["samples"], tot["hits"])
        for mode, flags in (MODES if cap == 16 else {"unasked": 0}).items():
            check(call(rs, em, cs.o, cs.d, S, cs.seed, cap=cap, flags=flags, device=dev), E, R, cs.bits, tot["segments"],
                  tot["samples"], tot["hits"], f"{what}, cap {cap}, {mode}")
        got = call(rs, em, cs.o, cs.d, S, cs.seed, cap=cap, device=dev, stats=True)
        check(got, E, R, cs.bits, tot["segments"], tot["samples"], tot["hits"], f"{what}, cap {cap}, counting")
        want = (cs.counts[0] + tot["cells"], cs.counts[1] + tot["tests"])
        assert (got[3]["cells_visited"], got[3]["triangle_tests"]) == want == comp["counts"], (what, cap, got[3], want)
    E, R, tot = alr.area_batch(cs.ref, cs.soup, rays, S, unshadowed=True)
    for mode, flags in PATHS.items():
        check(call(rs, em, cs.o, cs.d, S, cs.seed, flags=flags, device=dev, unshadowed=True), E, R, cs.bits, 0,
              tot["samples"], 0, f"{what}, unshadowed, {mode}")


def test_the_hand_derived_scene(oracle_mod):
    soup = tah.hand_soup()
    ref = trace_ref.RayRef(oracle_mod, soup, (4, 4, 4))
    o = np.array([[x, 0.0, 4.0] for x in tah.HAND_X], F)
    d = np.tile(np.array([0, 0, -1], F), (len(o), 1))
    bits, _ = ref.trace_batch(o, d)
    rs = RenderScene(soup, (4, 4, 4), device=0)
    try:
        for name, which in (("lamp", tah.LAMP), ("back", tah.BACK), ("plane", tah.PLANE), ("none", slice(0, 6)),
                            ("all", slice(0, 12))):
            es = tah.hand_set(soup, which)
            em = native.Emitters(rs.context, soup.pos.reshape(-1, 9)[which], None, soup.mat[which])
            check_set(em, es, name)
            rays = alr.make_rays(oracle_mod, ref, soup, es, o, d, bits, 8, seed=7)
            for cap in (16, 1):
                E, R, tot = alr.area_batch(ref, soup, rays, 8, cap)
                assert name not in ("back", "plane", "none") or (tot["samples"] == 0 and not E.any())
                for mode, flags in MODES.items():
                    check(call(rs, em, o, d, 8, 7, cap=cap, flags=flags), E, R, bits, tot["segments"], tot["samples"],
                          tot["hits"], f"hand scene, {name}, cap {cap}, {mode}")
            em.close()
    finally:
        rs.close()


# ------------------------------------------------ shapes, on the Cornell box
@pytest.fixture(scope="module")
def cornell():
    soup = scenes.get_scene("cornell")
    rs = RenderScene(soup, (16, 16, 16), device=0)
    es = alr.EmitterSet.of_soup(soup)
    check_set(rs.emitters(), es, "cornell")
    assert es.count == 2
    yield soup, rs, es
    rs.close()


def sized_set(soup, rs, count):
    """A set of `count` emitters on the Cornell box's materials: its own two
    for 2, else the first `count` triangles of a fan of slivers under the
    ceiling, all on the lamp's material."""
    if count == 2:
        return rs.emitters(), alr.EmitterSet.of_soup(soup)
    lamp = int(alr.EmitterSet.of_soup(soup).records["material"][0])
    p = np.asarray(soup.pos, np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c = (lo + hi) / 2
    c[1] = hi[1] - 0.05 * (hi[1] - lo[1])
    rad = 0.3 * min(hi[0] - lo[0], hi[2] - lo[2])
    pos = []
    for k in range(count):
        a0, a1 = 2 * np.pi * k / 65, 2 * np.pi * (k + 1) / 65
        pos.append(list(c) + [c[0] + rad * np.cos(a0), c[1], c[2] + rad * np.sin(a0)] +
                   [c[0] + rad * np.cos(a1), c[1], c[2] + rad * np.sin(a1)])         # facing down (-y)
    pos = np.asarray(pos, F).reshape(-1, 9)
    mat = np.full(count, lamp, np.uint32)
    return (native.Emitters(rs.context, pos, None, mat),
            alr.EmitterSet(pos, None, mat, soup.tex_desc, soup.texels))


def guarded_call(rs, em, o, d, S, flags, want_E=True, want_R=True, want_hits=True, cap=16, seed=0, index_base=0):
    """area_lights_raw on host arrays between guard words."""
    n = len(o)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    E = np.full(3 * (n + 2), 0xABABABAB, np.uint32)
    R = np.full(3 * (n + 2), 0xCDCDCDCD, np.uint32)
    hit = np.full(4 * (n + 2), 0xEFEFEFEF, np.uint32)
    st = rs.context.area_lights_raw(n, rays.ctypes.data, em, E[3:].ctypes.data if want_E else None,
                                    R[3:].ctypes.data if want_R else None, hit[4:].ctypes.data if want_hits else None,
                                    False, S, cap, seed, index_base, flags)
    for a, w, g in ((E, 3, 0xABABABAB), (R, 3, 0xCDCDCDCD), (hit, 4, 0xEFEFEFEF)):
        assert (a[:w] == g).all() and (a[-w:] == g).all(), "guard words"
    assert want_E or (E == 0xABABABAB).all()
    assert want_R or (R == 0xCDCDCDCD).all()
    assert want_hits or (hit == 0xEFEFEFEF).all()
    return (E[3:-3].reshape(n, 3) if want_E else None, R[3:-3].reshape(n, 3) if want_R else None,
            hit[4:-4].reshape(n, 4) if want_hits else None, st)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_ray_and_sample_counts_between_guard_words(n, cornell):
    soup, rs, es = cornell
    o, d = box_rays(soup, n, 100 + n)
    for S in (1, 2, 63, 64, 65):
        comp = composition(rs, es, o, d, S, seed=S)
        if n >= 63 and S >= 2:
            assert 0 < comp["samples"] < n * S and comp["irradiance"].any()
        for path, flags in PATHS.items():
            check_comp(guarded_call(rs, rs.emitters(), o, d, S, flags, seed=S), comp, f"n = {n}, S = {S}, {path}")


@pytest.mark.parametrize("count", [0, 1, 2, 65])
def test_sets_of_several_sizes(count, cornell):
    soup, rs, _ = cornell
    em, es = sized_set(soup, rs, count)
    check_set(em, es, f"{count} emitters")
    assert es.count == count
    o, d = box_rays(soup, 2049, 31)
    for S in (1, 5):
        comp = composition(rs, es, o, d, S, seed=3)
        assert (comp["samples"] > 0) == (count > 0)
        if count == 65:
            assert len(np.unique(np.searchsorted(es.C, mulhi(stream_words(3, np.arange(2049, dtype=np.uint32), S)[0], es.Q),
                                                 side="right") - 1)) == 65
        for path, flags in PATHS.items():
            check_comp(guarded_call(rs, em, o, d, S, flags, seed=3), comp, f"{count} emitters, S = {S}, {path}")
    if count != 2:
        em.close()


def test_a_ray_whose_samples_straddle_the_sub_chunk_cut(cornell):
    """4099 rays x 257 samples = 1,053,443 items: one cut at item 2^20, inside
    ray 4080, whose samples 0..15 fall before it and 16..256 after it."""
    soup, rs, es = cornell
    n, S = 4099, 257
    assert (1 << 20) // S == 4080 and (1 << 20) % S == 16 and n * S > 1 << 20
    o, d = box_rays(soup, n, 5)
    o[4080], d[4080] = (0.5, 2.5, -4.5), (0, 1, 0)                  # straight up onto the ceiling: the box's lamp is wound
                                                                    # like its floor and faces the ceiling above it
    comp = composition(rs, es, o, d, S, seed=9)
    TR = comp["traced"][4080]
    assert TR[:16].sum() >= 3 and TR[16:].sum() >= 8, "the straddling ray has traced samples on both sides of the cut"
    assert comp["irradiance"][4080].view(F).min() > 0
    for path, flags in list(PATHS.items()) + [("unasked", 0)]:
        check_comp(call(rs, rs.emitters(), o, d, S, 9, flags=flags), comp, f"4099 x 257, {path}")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_batch_across_the_ray_chunk_cut(device, cornell):
    """2^20 + 77 rays x 1 sample: two chunks; a host batch's contribution row
    lies 16-byte aligned behind a whole chunk's rays.  The rays around the cut
    against a call on those 205 alone with index_base advanced to them, bit for
    bit; the totals from the composition."""
    if device and (torch is None or not torch.cuda.is_available()):
        pytest.skip("torch sees no device")
    soup, rs, es = cornell
    n = (1 << 20) + 77
    idx = np.arange(n) % 128
    o, d = (np.ascontiguousarray(x[idx]) for x in box_rays(soup, 128, 6))
    comp = composition(rs, es, o, d, 1, seed=4, index_base=1000)
    lo = (1 << 20) - 128
    assert comp["traced"][lo:1 << 20].any() and comp["traced"][1 << 20:].any()
    for path, flags in PATHS.items():
        E, R, hits, st = call(rs, rs.emitters(), o, d, 1, 4, 1000, flags=flags, device=device)
        near = call(rs, rs.emitters(), o[lo:], d[lo:], 1, 4, 1000 + lo, flags=flags, device=device)
        check((E[lo:], R[lo:], hits[lo:], near[3]), near[0], near[1], near[2], near[3]["segments"] - 205,
              near[3]["samples"], near[3]["hits"], f"around the cut, {path}")
        print("area lights segments", path, st["segments"], n + comp["segments"])
        assert (st["segments"], st["samples"], st["hits"]) == (n + comp["segments"], comp["samples"], comp["crossings"]), path


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_launches_of_one_small_chunk(device, cornell):
    """128 rays x 2 samples in the Cornell box, one chunk and one sub-chunk:
    zrt_stats.trace_launches per mode, as the sequence in light_items' comment
    gives them (recorded on the GPU at the commit before the query calls came
    to share their host code)."""
    if device and (torch is None or not torch.cuda.is_available()):
        pytest.skip("torch sees no device")
    soup, rs, es = cornell
    o, d = box_rays(soup, 128, 6)
    comp = composition(rs, es, o, d, 2, seed=4)
    assert comp["samples"] > 0
    em = rs.emitters()
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
        res = call(rs, em, o, d, 2, 4, device=device, **kw)
        check_comp(res, comp, f"128 rays, {mode}")
        got[mode] = res[3]["trace_launches"]
        got[mode + " unshadowed"] = call(rs, em, o, d, 2, 4, device=device, unshadowed=True, **kw)[3]["trace_launches"]
    print("area lights launches", "device" if device else "host", got)
    assert got == want


def test_output_subsets_leave_the_other_arrays_alone(cornell):
    soup, rs, es = cornell
    o, d = box_rays(soup, 300, 8)
    comp = composition(rs, es, o, d, 5, seed=2)
    for path, flags in PATHS.items():
        for want_E, want_R in ((True, False), (False, True), (True, True)):
            for want_hits in (False, True):
                E, R, hit, st = guarded_call(rs, rs.emitters(), o, d, 5, flags, want_E, want_R, want_hits, seed=2)
                what = (path, want_E, want_R, want_hits)
                assert E is None or np.array_equal(E, comp["irradiance"]), what
                assert R is None or np.array_equal(R, comp["radiance"]), what
                assert hit is None or np.array_equal(hit, comp["hits"]), what
                assert (st["segments"], st["samples"], st["hits"]) == (300 + comp["segments"], comp["samples"],
                                                                       comp["crossings"]), what


def test_index_base_wraps_at_2_32_and_device_pointers(cornell):
    soup, rs, es = cornell
    o, d = box_rays(soup, 700, 17)
    base = 2 ** 32 - 300
    comp = composition(rs, es, o, d, 3, seed=2 ** 63 + 5, index_base=base)
    low = composition(rs, es, o[300:], d[300:], 3, seed=2 ** 63 + 5, index_base=0)
    assert np.array_equal(comp["irradiance"][300:], low["irradiance"]) and comp["irradiance"].any()
    for path, flags in PATHS.items():
        check_comp(call(rs, rs.emitters(), o, d, 3, 2 ** 63 + 5, base, flags=flags), comp, f"wrapping keys, {path}")
        check_comp(call(rs, rs.emitters(), o, d, 3, 2 ** 63 + 5, base + 2 ** 32, flags=flags), comp, f"keys mod 2^32, {path}")
        if torch is not None and torch.cuda.is_available():
            check_comp(call(rs, rs.emitters(), o, d, 3, 2 ** 63 + 5, base, flags=flags, device=True), comp,
                       f"device pointers, {path}")


def test_unshadowed_against_numpy_alone(cornell):
    """On the fan of 65 slivers that faces the floor: the box's own lamp faces
    the ceiling a hundredth above it and nothing ever stands between the two."""
    soup, rs, _ = cornell
    em, es = sized_set(soup, rs, 65)
    o, d = box_rays(soup, 3000, 12)
    comp = composition(rs, es, o, d, 4, seed=1, unshadowed=True)
    lit = composition(rs, es, o, d, 4, seed=1)
    assert comp["segments"] == 0 and comp["samples"] == lit["samples"] and \
        not np.array_equal(comp["irradiance"], lit["irradiance"])
    for mode, flags in MODES.items():
        got = call(rs, em, o, d, 4, 1, flags=flags, unshadowed=True)
        check_comp(got, comp, f"unshadowed, {mode}")
        # no walk launch: a lane-walk call is the first hits' two launches, the gen and the reduce launch
        assert mode != "lane" or got[3]["trace_launches"] == 4, got[3]
        check_comp(call(rs, em, o, d, 4, 1, flags=flags), lit, f"shadowed, {mode}")
    em.close()


# ------------------------------------------------------------------------ other
def test_a_sequence_on_one_context(cornell):
    """render, area lights, render, direct, area lights: the frames and the
    profile record are a fresh context's; the set outlives the renders."""
    soup, rs, es = cornell
    cam = camera_for(soup, None, 24, 24)
    fresh = RenderScene(soup, (16, 16, 16), device=0)
    want, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    o, d = box_rays(soup, 3000, 21)
    comp = composition(rs, es, o, d, 4, seed=6)
    lights = [native.Light.point((0.5, 2.5, -2.5), (3, 2, 1))]
    dr = rs.direct(o, d, lights)["irradiance"].view(np.uint32).copy()
    em = rs.emitters()
    for path, flags in PATHS.items():
        img, _ = rs.render(cam, num_samples=2, max_bounce=4, flags=native.FLAG_KERNEL_TIMES)
        assert np.array_equal(img, want), f"render before a {path} call"
        prof = rs.context.profile()
        check_comp(call(rs, em, o, d, 4, 6, flags=flags), comp, path)
        assert rs.context.profile() == prof, "zrt_context_profile's record is the last render's"
        img, _ = rs.render(cam, num_samples=2, max_bounce=4)
        assert np.array_equal(img, want), f"render after a {path} call"
        assert np.array_equal(rs.direct(o, d, lights, flags=flags)["irradiance"].view(np.uint32), dr), path
        check_comp(call(rs, em, o, d, 4, 6, flags=flags), comp, f"{path} again")
        check_set(em, es, "the set after renders and queries")


def test_empty_and_bad_batches_on_a_live_context(cornell):
    soup, rs, _ = cornell
    ctx, em = rs.context, rs.emitters()
    out = np.full(16, 0xABABABAB, np.uint32)
    rays = np.zeros(6, np.float32)
    r, p = rays.ctypes.data, out.ctypes.data
    for flags in (0, native.TRACE_PARK, native.AREA_UNSHADOWED):
        st = ctx.area_lights_raw(0, r, em, p, p, None, False, 4, 16, 0, 0, flags)
        assert st["segments"] == 0 and st["hits"] == 0 and st["samples"] == 0
    ctx.area_lights_raw(0, None, None, None, None, None, False, 4)
    z = np.zeros((0, 3), np.float32)
    res = ctx.area_lights(z, z, em, 4, radiance=True, hits=True)
    assert res["irradiance"].shape == (0, 3) and res["radiance"].shape == (0, 3) and res["t"].shape == (0,)
    other = RenderScene(tah.hand_soup(), (4, 4, 4), device=0)
    foreign = native.Emitters(other.context, soup.pos.reshape(-1, 9)[:2], None, np.zeros(2, np.uint32))
    try:
        for args, kw in (((None, em, p, p, None, False, 4), {}), ((r, None, p, p, None, False, 4), {}),
                         ((r, foreign, p, p, None, False, 4), {}),                       # a set made on another context
                         ((r, em, None, None, p, False, 4), {}),
                         ((r, em, p, p, None, False, 0), {}), ((r, em, p, p, None, False, 65536), {}),
                         ((r, em, p, p, None, False, 4, 0), {}), ((r, em, p, p, None, False, 4, 257), {}),
                         ((r, em, p, p, None, False, 4, 16), {"flags": native.SEGMENT_ANY}),
                         ((r, em, p, p, None, False, 4, 16), {"flags": native.DIRECT_UNSHADOWED}),
                         ((r, em, p, p, None, False, 4, 16), {"flags": 0x4})):
            with pytest.raises(native.ZrtError) as e:
                ctx.area_lights_raw(1, *args, **kw)
            assert e.value.status == -1
        # the other calls keep refusing the new bit
        bit = native.AREA_UNSHADOWED
        one = [native.Light.point((0.5, 2.5, -2.5), (1, 1, 1))]
        L = native.lib()
        for refused in (lambda: ctx.direct_raw(1, r, one, p, p, None, False, 16, bit),
                        lambda: ctx.surface_raw(1, r, p, None, False, bit),
                        lambda: ctx.transmittance_raw(1, r, None, p, None, False, bit, 1.0, 16)):
            with pytest.raises(native.ZrtError) as e:
                refused()
            assert e.value.status == -1
        assert L.zrt_context_trace(ctx._h, C.byref(native.RayBatch(1, r, p, 0, bit)), None) == -1
        assert L.zrt_context_radiance(ctx._h, C.byref(native.RadianceBatch(1, r, p, None, 0, bit, 1, 1, 0, 0)), None) == -1
        assert (out == 0xABABABAB).all()
        ctx.area_lights_raw(1, r, em, p, out[4:].ctypes.data, out[8:].ctypes.data, False, 4)   # the control: the valid batch runs
    finally:
        foreign.close()
        other.close()
