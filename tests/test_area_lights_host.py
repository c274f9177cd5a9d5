"""Area-light queries (zrt_emitters_*, zrt_context_area_lights), the part that
runs without a GPU: the C ABI's declarations and exports, the layouts of the
80-byte record and the batch, the argument errors that come back before any
device work, and the reference (area_light_ref.py) -- its properties on a
hand-derived scene, its agreement with the path tracer on a closed box, and
what the fuzz seeds reach.

The hand-derived scene (materials: 0 opaque, 1 glass of alpha 1/4, 2 the lamp,
emission (4, 2, 1), opaque; every texture 1x1):

    floor    z = 0 over [-4, 4]^2, facing up, material 0
    glass    z = 1 over x in [0, 4], facing down, material 1
    blocker  z = 1 over x in [-4, -3/2], facing down, material 0
    lamp     z = 2 over [-1/4, 1/4]^2, facing DOWN, material 2
    back     z = 5/2 over [-1/4, 1/4]^2, facing UP, material 2: seen from behind
    plane    z = 0 over x in [5, 6], facing up, material 2: in the floor's plane

Rays start at z = 4 and point straight down; they pass every upper quad from
behind (Moller-Trumbore culls back faces) and meet the floor at t = 4 with
position (x, y, 0) and N = (0, 0, 1).  A segment from (x, y, 0) to a point of
the lamp crosses z = 1 at (x, y) / 2 + up to 1/8: over nothing for x = -1,
over the glass for x = 1 (T = 3/4), over the blocker for x = -7/2 (T = 0).
"""
import ctypes as C
import dataclasses
import math
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

import area_light_ref as alr
import radiance_ref
import test_query_fuzz_gpu as qf
import trace_ref

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
F = np.float32


def _fields(hdr, name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*(\[\d+\])?\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]


def test_header_declares_the_five_symbols_and_native_binds_them():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    L = native.lib()
    for sym in ("zrt_emitters_create", "zrt_emitters_info", "zrt_emitters_read", "zrt_emitters_destroy",
                "zrt_context_area_lights"):
        assert re.search(r"\b(int|void)\s+%s\s*\(" % sym, hdr), sym
        assert sym in native.EXPORTS and hasattr(L, sym), sym
    assert re.search(r"\bint\s+zrt_context_area_lights\s*\(\s*zrt_context\s*\*\s*\w*\s*,"
                     r"\s*const\s+zrt_area_light_batch\s*\*", hdr)
    assert re.search(r"#define\s+ZRT_AREA_UNSHADOWED\s+0x800000u", hdr) and native.AREA_UNSHADOWED == 0x800000
    assert "area-light queries (ABI 2, added)" in hdr and "0x1.ff8p-1f" in hdr and "0x1p24f" in hdr
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and L.zrt_abi_version() == 2
    # a bit of its own among every flag the header defines
    others = [int(v, 16) for n, v in re.findall(r"#define\s+(ZRT_\w+)\s+(0x[0-9A-Fa-f]+)u", hdr)
              if n != "ZRT_AREA_UNSHADOWED"]
    assert len(others) >= 20 and not any(v & 0x800000 for v in others)
    for name in ("area_lights_raw", "area_lights"):
        assert callable(getattr(native.Context, name))
    assert callable(native.Emitters.read) and callable(native.Emitters.info)
    from zig_raytracing_contest_amd import RenderScene
    assert callable(RenderScene.area_lights) and callable(RenderScene.emitters)


def test_record_and_batch_layouts():
    """Against the header's own comments: 80 B each."""
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\}\s*zrt_emitter;\s*/\*\s*80 B\s*\*/", hdr)
    assert re.search(r"\}\s*zrt_area_light_batch;\s*/\*\s*80 B\s*\*/", hdr)
    dt, ab = native.EMITTER_DTYPE, native.AreaLightBatch
    assert dt.itemsize == 80
    assert [dt.fields[n][1] for n in dt.names] == [0, 12, 16, 28, 32, 44, 48, 72, 76]
    assert _fields(hdr, "zrt_emitter") == list(dt.names)
    assert C.sizeof(ab) == 80
    assert [getattr(ab, n).offset for n, _ in ab._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 72]
    assert _fields(hdr, "zrt_area_light_batch") == [n for n, _ in ab._fields_]


def test_area_lights_rejects_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included),
    and the outputs stay as they were."""
    L = native.lib()
    assert L.zrt_context_area_lights(None, None, None) == -1
    rays = np.zeros(6, np.float32)
    irr = np.full(3, 0xABABABAB, np.uint32)
    rad = np.full(3, 0xCDCDCDCD, np.uint32)
    hit = np.full(4, 0xEFEFEFEF, np.uint32)
    fake = np.zeros(16, np.uint64)                  # stands for a set: never read behind a null context
    r, e, q, h, s = rays.ctypes.data, irr.ctypes.data, rad.ctypes.data, hit.ctypes.data, fake.ctypes.data
    AB = native.AreaLightBatch
    for batch in (AB(0, None, None, None, None, None, 0, 0, 4, 16, 0, 0),
                  AB(1, r, s, e, q, h, 0, 0, 4, 16, 0, 0),                              # a valid batch
                  AB(1, None, s, e, q, h, 0, 0, 4, 16, 0, 0),                           # null rays
                  AB(1, r, None, e, q, h, 0, 0, 4, 16, 0, 0),                           # null emitters
                  AB(1, r, s, None, None, h, 0, 0, 4, 16, 0, 0),                        # no output at all
                  AB(1, r, s, e, q, h, 0, 0, 0, 16, 0, 0),                              # num_samples 0
                  AB(1, r, s, e, q, h, 0, 0, 65536, 16, 0, 0),                          # ... above 65535
                  AB(1, r, s, e, q, h, 0, 0, 4, 0, 0, 0),                               # max_crossings 0
                  AB(1, r, s, e, q, h, 0, 0, 4, 257, 0, 0),                             # ... above 256
                  AB(1, r, s, e, q, h, 2, 0, 4, 16, 0, 0),                              # on_device > 1
                  AB(1, r, s, e, q, None, 0, native.FLAG_ONE_SET, 4, 16, 0, 0),         # a render-only flag
                  AB(1, r, s, e, q, None, 0, native.SEGMENT_ANY, 4, 16, 0, 0),          # another call's flags
                  AB(1, r, s, e, q, None, 0, native.DIRECT_UNSHADOWED, 4, 16, 0, 0),
                  AB(1, r, s, e, q, None, 0, native.SVGF_ROW_MAJOR, 4, 16, 0, 0),
                  AB(1, r, s, e, q, None, 0, native.AREA_UNSHADOWED, 4, 16, 0, 0)):     # (valid: its own flag)
        assert L.zrt_context_area_lights(None, C.byref(batch), None) == -1
    assert (irr == 0xABABABAB).all() and (rad == 0xCDCDCDCD).all() and (hit == 0xEFEFEFEF).all()
    # the set's own entry points
    out = C.c_void_p(0x1234)
    pos, mat = np.zeros(9, np.float32), np.zeros(1, np.uint32)
    assert L.zrt_emitters_create(None, pos.ctypes.data, None, mat.ctypes.data, 1, C.byref(out)) == -1
    assert out.value == 0x1234
    assert L.zrt_emitters_info(None, None, None, None) == -1 and L.zrt_emitters_read(None, None, None) == -1
    L.zrt_emitters_destroy(None)


def test_the_other_calls_refuse_the_new_bit():
    """Through a null context, as above, outputs untouched; on a live context
    test_area_lights_gpu.py asks again."""
    L = native.lib()
    bit = native.AREA_UNSHADOWED
    rays, out = np.zeros(6, np.float32), np.full(16, 0xABABABAB, np.uint32)
    r, o = rays.ctypes.data, out.ctypes.data
    lt = (native.Light * 1)(native.Light.point((0, 0, 1), (1, 1, 1)))
    assert L.zrt_context_trace(None, C.byref(native.RayBatch(1, r, o, 0, bit)), None) == -1
    assert L.zrt_context_direct(None, C.byref(native.DirectBatch(1, r, C.cast(lt, C.c_void_p), o, None, None, 0, bit, 1,
                                                                 16)), None) == -1
    assert L.zrt_context_radiance(None, C.byref(native.RadianceBatch(1, r, o, None, 0, bit, 1, 1, 0, 0)), None) == -1
    assert (out == 0xABABABAB).all()


# ------------------------------------------------------- the hand-derived scene
LAMP_E = (4.0, 2.0, 1.0)


def hand_soup():
    s = scenes.get_scene("sphere")

    def quad(x0, x1, y0, y1, z, up):
        a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)        # (b - a) x (c - a) = +z
        return [a + b + c, a + c + d] if up else [a + c + b, a + d + c]

    pos = (quad(-4, 4, -4, 4, 0, True) + quad(0, 4, -4, 4, 1, False) + quad(-4, -1.5, -4, 4, 1, False) +
           quad(-0.25, 0.25, -0.25, 0.25, 2, False) + quad(-0.25, 0.25, -0.25, 0.25, 2.5, True) +
           quad(5, 6, -0.5, 0.5, 0, True))
    up, dn = [0, 0, 1] * 3, [0, 0, -1] * 3
    nrm = [up] * 2 + [dn] * 6 + [up] * 4
    desc = np.zeros((3, 3, 7), np.int32)
    for m in range(3):
        for slot, off in enumerate((0, 3, 6)):
            desc[m, slot] = (7 * m + off, 1, 1, 0, 0, 0, 0)
    texels = [0.5, 0.25, 1.0, 0, 0, 0, 1.0,            # the floor and the blocker: opaque
              0.5, 0.5, 0.5, 0, 0, 0, 0.25,            # the glass
              0.5, 0.5, 0.5, *LAMP_E, 1.0]             # the lamps
    return dataclasses.replace(
        s, name="area_hand", pos=np.asarray(pos, np.float32), nrm=np.asarray(nrm, np.float32),
        uv=np.zeros((12, 6), np.float32), mat=np.asarray([0, 0, 1, 1, 0, 0, 2, 2, 2, 2, 2, 2], s.mat.dtype),
        materials=[scenes.Material()] * 3, textures=[], tex_desc=desc, texels=np.asarray(texels, np.float32))


LAMP, BACK, PLANE = slice(6, 8), slice(8, 10), slice(10, 12)
HAND_X = [-1.0, 1.0, -3.5]
HAND_T = [1.0, 0.75, 0.0]


def hand_set(soup, which):
    return alr.EmitterSet(soup.pos.reshape(-1, 9)[which], None, soup.mat[which], soup.tex_desc, soup.texels)


@pytest.fixture(scope="module")
def hand(oracle_mod):
    soup = hand_soup()
    ref = trace_ref.RayRef(oracle_mod, soup, (4, 4, 4))
    o = np.array([[x, 0.0, 4.0] for x in HAND_X], F)
    d = np.tile(np.array([0, 0, -1], F), (len(o), 1))
    bits, _ = ref.trace_batch(o, d)
    assert (bits[:, 0].view(F) == 4.0).all() and (ref.indices[bits[:, 3]] < 2).all()     # the floor, from above
    return ref, soup, o, d, bits


def test_the_whole_soup_as_a_set(hand):
    """Six of the twelve triangles emit, in source order; the lamps' two
    triangles have a = 1/8, w = 1/2, the plane's a = w' = 1/2 * 4: q = 2^24 for
    the largest, 2^22 for the others; C is their running sum."""
    _, soup, *_ = hand
    es = alr.EmitterSet.of_soup(soup)
    assert es.count == 6 and list(es.records["triangle"]) == [6, 7, 8, 9, 10, 11]
    assert list(es.records["a"]) == [0.125] * 4 + [0.5] * 2 and (es.records["material"] == 2).all()
    assert list(es.records["q"]) == [2 ** 22] * 4 + [2 ** 24] * 2
    assert list(es.C) == [0, 2 ** 22, 2 * 2 ** 22, 3 * 2 ** 22, 2 ** 24, 2 * 2 ** 24] and es.Q == 3 * 2 ** 24
    assert es.select(0) == 0 and es.select(2 ** 64 - 1) == 5
    assert (es.records["e1"][0] == [0.5, 0.5, 0]).all() and (es.records["v0"][0] == [-0.25, -0.25, 2]).all()
    assert alr.EmitterSet(np.zeros((0, 9)), None, np.zeros(0), soup.tex_desc, soup.texels).count == 0
    # NaN, negative and infinite texels: the fold drops the first two, inf makes w infinite: no emitter
    assert list(alr.material_max([[[0] * 7, [0, 2, 2, 0, 0, 0, 0], [0] * 7]],
                                 [np.nan, -1, 0.25, 0.5, -np.inf, np.nan] + [0.125] * 6)) == [0.5]
    assert alr.material_max([[[0] * 7, [0, 1, 1, 0, 0, 0, 0], [0] * 7]], [np.nan, -2, -0.0])[0] == 0
    inf = alr.EmitterSet(soup.pos[6:8], None, [0, 0], [[[0] * 7, [0, 1, 1, 0, 0, 0, 0], [0] * 7]], [1, np.inf, 0])
    assert inf.count == 0


def test_the_fold_and_the_selection():
    rng = np.random.default_rng(1)
    words = rng.integers(0, 2 ** 64, (1000, 2), dtype=np.uint64)
    folded = 0
    for x1, x2 in list(words) + [(2 ** 64 - 1, 2 ** 64 - 1), (0, 0), (2 ** 64 - 1, 0), (1 << 63, 1 << 63)]:
        bu, bv = alr.fold_uv(x1, x2)
        assert bu >= 0 and bv >= 0 and F(bu + bv) <= 1, (x1, x2, bu, bv)
        folded += F(F(int(x1) >> 40) * alr.INV24) != bu
    assert 400 < folded < 600
    assert alr.fold_uv(1 << 63, 1 << 63) == (0.5, 0.5)                 # bu + bv == 1 is not folded
    # rsel < Q at the largest word, for small and large totals
    for Q in (1, 2 ** 24, 3 * 2 ** 24, 2 ** 52 - 1):
        assert ((2 ** 64 - 1) * Q) >> 64 == Q - 1
    # a one-emitter set: q = 2^24 = Q, the ratio is exactly 1
    soup = hand_soup()
    one = hand_set(soup, slice(6, 7))
    assert one.count == 1 and one.Q == 2 ** 24 == int(one.records["q"][0]) and F(one.Q) / F(one.records["q"][0]) == 1


def test_hand_derived_scene(hand, oracle_mod):
    ref, soup, o, d, bits = hand
    spp = 8
    lamp = hand_set(soup, LAMP)
    rays = alr.make_rays(oracle_mod, ref, soup, lamp, o, d, bits, spp, seed=7)
    for ray, x in zip(rays, HAND_X):
        f = ray.words.view(F)
        assert ray.shaded and [float(v) for v in f[0:3]] == [x, 0.0, 0.0] and [float(v) for v in f[4:7]] == [0, 0, 1]
        assert len(ray.items) == spp and all(it.traced for it in ray.items)
        assert all(abs(float(it.y[0])) <= 0.25 and abs(float(it.y[1])) <= 0.25 and it.y[2] == 2 for it in ray.items)
    for ray, T in zip(rays, HAND_T):
        for it in ray.items:
            got, n, segs, *_ = it.chain(ref, soup).cut(16)
            assert (float(got), n, segs) == {1.0: (1.0, 0, 1), 0.75: (0.75, 1, 2), 0.0: (0.0, 1, 1)}[T]
    E, R, tot = alr.area_batch(ref, soup, rays, spp)
    assert tot["samples"] == 3 * spp and tot["hits"] == 2 * spp and tot["segments"] == 4 * spp
    Ef = E.view(F).astype(np.float64)
    # float64 from the formulas: g = c cl / d2 * (area 1/4), averaged over the same points
    for i, (ray, T) in enumerate(zip(rays, HAND_T)):
        want = np.zeros(3)
        for it in ray.items:
            v = np.array([float(c) for c in it.y]) - np.array([HAND_X[i], 0.0, 0.0])
            d2 = v @ v
            want += np.array(LAMP_E) * (v[2] / math.sqrt(d2)) ** 2 / d2 * 0.25 * T
        want /= spp
        assert np.allclose(Ef[i], want, rtol=1e-5, atol=0), (i, Ef[i], want)
    assert (Ef[0] > 0).all() and not Ef[2].any()
    base = np.array([0.5, 0.25, 1.0])
    assert np.allclose(R.view(F).astype(np.float64), base * Ef / math.pi, rtol=1e-6, atol=0)
    # unshadowed: T = 1 everywhere, nothing walked; only the glass and the blocker rays change
    E1, _, tot1 = alr.area_batch(ref, soup, rays, spp, unshadowed=True)
    assert tot1["samples"] == 3 * spp and tot1["segments"] == 0 and tot1["hits"] == 0
    assert [bool((E1[i] == E[i]).all()) for i in range(3)] == [True, False, False]
    assert np.allclose(E1.view(F)[1] * 0.75, E.view(F)[1], rtol=1e-6) and E1[2].all()
    # a cap of 1 cuts the glass ray's chain after its crossing: the product so far stands
    Ec, _, totc = alr.area_batch(ref, soup, rays, spp, cap=1)
    assert (Ec == E).all() and totc["segments"] == 3 * spp and totc["hits"] == 2 * spp
    # seen from behind, and in the hit point's own plane: nothing is traced
    for which, why in ((BACK, "back"), (PLANE, "behind")):
        es = hand_set(soup, which)
        rr = alr.make_rays(oracle_mod, ref, soup, es, o, d, bits, spp, seed=7)
        assert all(it.cull == why for ray in rr for it in ray.items) and sum(len(ray.items) for ray in rr) == 3 * spp
        Eb, Rb, tb = alr.area_batch(ref, soup, rr, spp)
        assert not Eb.any() and not Rb.any() and tb["samples"] == 0 and tb["segments"] == 0
    # an empty set: +0 and no item at all
    none = hand_set(soup, slice(0, 6))
    rr = alr.make_rays(oracle_mod, ref, soup, none, o, d, bits, spp)
    assert none.count == 0 and not any(ray.items for ray in rr) and not alr.area_batch(ref, soup, rr, spp)[0].any()


def test_an_unoccluded_lamp_does_not_shadow_itself(hand, oracle_mod):
    """1,000 seeded points on the lamp from the ray at x = -1: every chain ends
    in a miss with T = 1.  The lamp faces the hit point, so its own triangles
    are what a chain bounded by the full distance could meet at t ~ length(v):
    the bound is shortened by 2^-10 for this."""
    ref, soup, o, d, bits = hand
    lamp = hand_set(soup, LAMP)
    ray, = alr.make_rays(oracle_mod, ref, soup, lamp, o[:1], d[:1], bits[:1], 1000, seed=2024)
    assert len(ray.items) == 1000 and len({(float(it.bu), float(it.bv)) for it in ray.items}) == 1000
    for it in ray.items:
        ch = it.chain(ref, soup)
        assert it.traced and ch.end == "miss" and ch.cut(16)[:2] == (1.0, 0)
        assert it.b < alr.length([F(it.y[j] - it.pos[j]) for j in range(3)])


# ------------------------------------------- agreement with the path tracer
def box_soup():
    """A closed box [-1, 1]^3 of 12 inward-facing triangles with unit face
    normals, base colour (3/4, 1/2, 1/4), and inside it a lamp: a quad at
    z = 0.9 over [-0.3, 0.3]^2 facing down, emission (8, 6, 4), base colour 1/2.
    Everything opaque, every texture 1x1."""
    s = scenes.get_scene("sphere")
    pos, nrm = [], []
    for ax in range(3):
        for side in (-1.0, 1.0):
            u, v = (ax + 1) % 3, (ax + 2) % 3
            c = []
            for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = [0.0, 0.0, 0.0]
                p[ax], p[u], p[v] = side, su, sv
                c.append(p)
            inward = [0.0, 0.0, 0.0]
            inward[ax] = -side
            for tri in ((c[0], c[1], c[2]), (c[0], c[2], c[3])):
                n = np.cross(np.subtract(tri[1], tri[0]), np.subtract(tri[2], tri[0]))
                if n[ax] * inward[ax] < 0:
                    tri = (tri[0], tri[2], tri[1])
                pos.append(tri[0] + tri[1] + tri[2])
                nrm.append(inward * 3)
    a, b, c, d = (-0.3, -0.3, 0.9), (0.3, -0.3, 0.9), (0.3, 0.3, 0.9), (-0.3, 0.3, 0.9)
    pos += [a + c + b, a + d + c]                                               # facing down
    nrm += [[0, 0, -1] * 3] * 2
    desc = np.zeros((2, 3, 7), np.int32)
    for m in range(2):
        for slot, off in enumerate((0, 3, 6)):
            desc[m, slot] = (7 * m + off, 1, 1, 0, 0, 0, 0)
    texels = [0.75, 0.5, 0.25, 0, 0, 0, 1.0,
              0.5, 0.5, 0.5, 8.0, 6.0, 4.0, 1.0]
    return dataclasses.replace(
        s, name="area_box", pos=np.asarray(pos, np.float32), nrm=np.asarray(nrm, np.float32),
        uv=np.zeros((14, 6), np.float32), mat=np.asarray([0] * 12 + [1, 1], s.mat.dtype),
        materials=[scenes.Material()] * 2, textures=[], tex_desc=desc, texels=np.asarray(texels, np.float32))


BOX_O = (0.1, -0.2, 0.0)
BOX_D = [(0.2, 0.1, -1.0), (-0.5, 0.3, -1.0), (1.0, 0.2, -0.3), (-1.0, -0.4, 0.2), (0.3, 1.0, -0.1), (-0.2, -1.0, 0.5),
         (0.6, 0.5, 1.0),            # the ceiling beside the lamp: it sees the lamp's back
         (-0.1, 0.2, 1.0)]           # the lamp itself, from below
BATCHES, SPP = 32, 256


def test_the_reference_agrees_with_the_path_tracer(oracle_mod):
    """Two estimates of one integral per ray and channel: the oracle's linear
    radiance at max_bounce 2 (emission + base colour * E[Le at the second
    hit]; the box is closed, nothing reaches the sky) and the reference's
    `radiance`; each as 32 batches of distinct seeds at 256 samples, compared by
    |mean_a - mean_b| <= 6 sqrt(var_a / 32 + var_b / 32) with the variances
    taken over the batch means.

    Measured (seeds 1000.. and 2000..): the largest |difference| / sigma over
    the six lit rays is 1.83 (the two others are exact on both sides); the path
    tracer's batch standard deviation is 17 to 89 times the reference's on them
    (16.9, 19.1, 37.8, 55.1, 75.8, 89.0): the feature's variance gain at equal
    samples on this scene, whose lamp covers 2% of a hit point's hemisphere."""
    soup = box_soup()
    res = (2, 2, 2)
    ref = trace_ref.RayRef(oracle_mod, soup, res)
    o = np.tile(np.array(BOX_O, F), (len(BOX_D), 1))
    d = np.array([np.array(v) / np.linalg.norm(v) for v in BOX_D], F)
    bits, _ = ref.trace_batch(o, d)
    src = ref.indices[bits[:, 3]]
    assert (bits[:, 3] != trace_ref.MISS).all() and src[6] in (10, 11) and src[7] in (12, 13), src    # the ceiling, the lamp
    es = alr.EmitterSet.of_soup(soup)
    assert es.count == 2 and list(es.records["triangle"]) == [12, 13]
    pt = radiance_ref.RadianceRef(oracle_mod, soup, res)
    a = np.zeros((BATCHES, len(o), 3))
    b = np.zeros((BATCHES, len(o), 3))
    for k in range(BATCHES):
        a[k] = pt.radiance(o, d, SPP, 2, seed=1000 + k)[0]
        rays = alr.make_rays(oracle_mod, ref, soup, es, o, d, bits, SPP, seed=2000 + k)
        b[k] = alr.area_batch(ref, soup, rays, SPP)[1].view(F)
    ma, mb, va, vb = a.mean(0), b.mean(0), a.var(0, ddof=1), b.var(0, ddof=1)
    sigma = np.sqrt(va / BATCHES + vb / BATCHES)
    with np.errstate(all="ignore"):
        print("difference / sigma:", np.round(np.abs(ma - mb) / sigma, 2).tolist())
        print("std(path tracer) / std(reference):", np.round(np.sqrt(va / vb), 2).tolist())
    print("means:", ma.tolist(), mb.tolist())
    assert (ma[:6] > 0).all() and (mb[:6] > 0).all()
    assert not ma[6].any() and not mb[6].any()                         # the lamp's back is dark
    assert (ma[7] == [8, 6, 4]).all() and (mb[7] == [8, 6, 4]).all()   # the lamp's own emission, nothing added
    assert (np.abs(ma - mb) <= 6 * sigma).all(), (ma, mb, sigma)


# ------------------------------------------------ the fuzz rays: what they reach
FUZZ_SPP = 2


def fuzz_set(cs):
    if not hasattr(cs, "_area_set"):
        cs._area_set = alr.EmitterSet.of_soup(cs.soup)
    return cs._area_set


def cached_rays(orc, cs):
    """The Ray objects of a fuzz seed's rays at FUZZ_SPP samples, seed = the
    case's seed, made once and kept on the case with the chains they walk."""
    if not hasattr(cs, "_area_rays"):
        cs._area_rays = alr.make_rays(orc, cs.ref, cs.soup, fuzz_set(cs), cs.o, cs.d, cs.bits, FUZZ_SPP, seed=cs.seed)
    return cs._area_rays


@pytest.fixture(scope="module")
def case(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed]
    return get


def coverage(orc, cases):
    n = dict.fromkeys(("emitters", "no_emitters", "hits", "items", "T1", "Tpart", "T0", "behind", "back"), 0)
    for cs in cases:
        es = fuzz_set(cs)
        n["emitters"] += es.count
        n["no_emitters"] += es.count == 0
        for ray in cached_rays(orc, cs):
            if ray.words is None:
                continue
            n["hits"] += 1
            for it in ray.items:
                n["items"] += 1
                if not it.traced:
                    n[it.cull] += 1
                    continue
                T = it.chain(cs.ref, cs.soup).cut(alr.CAP)[0]
                n["T1" if T == 1 else "T0" if T == 0 else "Tpart"] += 1
    return n


def test_the_fuzz_seeds_reach_what_the_call_has_to_get_right(case, oracle_mod):
    """Counted from the reference alone: seeds 0..39, all 128 rays, 2 samples
    each, chains under 16 crossings.  Counted: 3562 emitters over the 40 seeds,
    18 seeds without any (their rays have no item), 1783 first hits, 1720
    items; traced with T = 1 152, with 0 < T < 1 20, with T = 0 111; culled by
    c <= 0 1048, by the emitter's back 389.  The floors are half of these.  The
    class the seeds cannot be counted on for -- an emitter in the hit point's
    own plane, c == 0 exactly -- is made by hand in test_hand_derived_scene."""
    n = coverage(oracle_mod, (case(s) for s in qf.SEEDS))
    print(n)
    assert n["items"] == n["T1"] + n["Tpart"] + n["T0"] + n["behind"] + n["back"], n
    assert n["emitters"] >= 1781 and n["no_emitters"] >= 9 and n["hits"] >= 891 and n["items"] >= 860, n
    assert n["T1"] >= 76 and n["Tpart"] >= 10 and n["T0"] >= 55 and n["behind"] >= 524 and n["back"] >= 194, n
