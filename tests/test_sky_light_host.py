"""Sky-light queries (zrt_context_sky_light), the part that runs without a GPU:
the C ABI's declaration and export, the batch's layout, the flag's bit, the
argument errors that come back before any device work, and the reference
(sky_light_ref.py) -- its sky colour against the oracle's, its estimator
against the closed form on an unoccluded hemisphere, its exact answers on a
hand-made scene, its agreement with the path tracer, and what the fuzz seeds
reach.

The hand-made scenes (every texture 1x1; y is up, as in the sky's gradient):

    floor   y = 0 over [-4, 4]^2, facing up, base colour (1/2, 1/4, 1),
            emission (1/8, 1/4, 1/2), opaque
    dome    the four walls x, z = +-h from y = -1 to y = h and the roof y = h,
            all facing inward: whatever leaves (0, 0, 0) upward crosses exactly
            one of its faces from the front.  Glass of alpha 1/4, or opaque

The ray starts at (0, 4, 0) and points straight down: it meets the floor at
t = 4, position (0, -4 eps, 0), N = (0, 1, 0).  The walls reach below the floor
so that a sample at grazing angle cannot slip under them from that position.
"""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

import area_light_ref as alr
import radiance_ref
import sky_light_ref as slr
import test_area_lights_host as tah
import test_query_fuzz_gpu as qf
import trace_ref

ROOT = tah.ROOT
F = np.float32


# ------------------------------------------------------------ the C interface
def test_header_declares_the_symbol_and_native_binds_it():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    L = native.lib()
    assert re.search(r"\bint\s+zrt_context_sky_light\s*\(\s*zrt_context\s*\*\s*\w*\s*,\s*const\s+zrt_sky_light_batch\s*\*",
                     hdr)
    assert "zrt_context_sky_light" in native.EXPORTS and hasattr(L, "zrt_context_sky_light")
    assert re.search(r"#define\s+ZRT_SKY_UNSHADOWED\s+0x1000000u", hdr) and native.SKY_UNSHADOWED == 0x1000000
    assert "sky-light queries (ABI 2, added)" in hdr and "0x1.921fb6p+1f" in hdr and "0x40490FDB" in hdr
    assert hdr.index("area-light queries (ABI 2, added)") < hdr.index("sky-light queries (ABI 2, added)") < \
        hdr.index("light-probe queries (ABI 2, added)")
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and L.zrt_abi_version() == 2
    for name in ("sky_light_raw", "sky_light"):
        assert callable(getattr(native.Context, name))
    from zig_raytracing_contest_amd import RenderScene
    assert callable(RenderScene.sky_light)


def test_batch_layout():
    """Against the header's own comment: 80 B."""
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\}\s*zrt_sky_light_batch;\s*/\*\s*80 B\s*\*/", hdr)
    sb = native.SkyLightBatch
    assert C.sizeof(sb) == 80
    assert [getattr(sb, n).offset for n, _ in sb._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 72]
    assert tah._fields(hdr, "zrt_sky_light_batch") == [n for n, _ in sb._fields_] == [
        "num_rays", "rays", "irradiance", "radiance", "visibility", "hits", "on_device", "flags", "num_samples",
        "max_crossings", "seed", "index_base"]


def test_the_flag_has_a_bit_of_its_own_and_the_other_calls_refuse_it():
    """Against every `#define ZRT_...` bit of the header; the other batch calls
    through a null context, outputs untouched (on a live context
    test_sky_light_gpu.py asks again)."""
    hdr = open(f"{ROOT}/include/zrt.h").read()
    bit = native.SKY_UNSHADOWED
    others = {n: int(v, 16) for n, v in re.findall(r"#define\s+(ZRT_\w+)\s+(0x[0-9A-Fa-f]+)u", hdr)
              if n != "ZRT_SKY_UNSHADOWED"}
    assert len(others) >= 21 and "ZRT_AREA_UNSHADOWED" in others and not any(v & bit for v in others.values()), others
    assert bit == max(others.values()) << 1 and bit & (bit - 1) == 0            # the lowest bit no flag uses
    L = native.lib()
    rays, out = np.zeros(6, np.float32), np.full(16, 0xABABABAB, np.uint32)
    r, o = rays.ctypes.data, out.ctypes.data
    lt = (native.Light * 1)(native.Light.point((0, 0, 1), (1, 1, 1)))
    fake = np.zeros(16, np.uint64).ctypes.data
    assert L.zrt_context_trace(None, C.byref(native.RayBatch(1, r, o, 0, bit)), None) == -1
    assert L.zrt_context_segments(None, C.byref(native.SegmentBatch(1, r, None, o, None, 0, bit, 1.0, 0)), None) == -1
    assert L.zrt_context_surface(None, C.byref(native.SurfaceBatch(1, r, o, None, 0, bit)), None) == -1
    assert L.zrt_context_transmittance(None, C.byref(native.TransmittanceBatch(1, r, None, o, None, 0, bit, 1.0, 16)),
                                       None) == -1
    assert L.zrt_context_occlusion(None, C.byref(native.OcclusionBatch(1, r, None, o, None, None, 0, bit, 1.0, 4, 0, 0)),
                                   None) == -1
    assert L.zrt_context_light_probes(None, C.byref(native.LightProbeBatch(1, r, o, None, None, None, None, 0, bit, 4, 1,
                                                                           1, 0, 0, 0)), None) == -1
    assert L.zrt_context_direct(None, C.byref(native.DirectBatch(1, r, C.cast(lt, C.c_void_p), o, None, None, 0, bit, 1,
                                                                 16)), None) == -1
    assert L.zrt_context_area_lights(None, C.byref(native.AreaLightBatch(1, r, fake, o, None, None, 0, bit, 4, 16, 0, 0)),
                                     None) == -1
    assert L.zrt_context_radiance(None, C.byref(native.RadianceBatch(1, r, o, None, 0, bit, 1, 1, 0, 0)), None) == -1
    assert (out == 0xABABABAB).all()


def test_sky_light_rejects_bad_batches_before_any_gpu_work():
    """No batch, valid or not, gets past a null context, and none touches an
    output on its way to ZRT_ERR_INVALID_ARG.  The null context alone refuses
    each of them, so this does not tell the batch checks apart: those are
    asked one by one on a live context, with a valid batch as their control
    (test_sky_light_gpu.py, test_empty_and_bad_batches_on_a_live_context)."""
    L = native.lib()
    assert L.zrt_context_sky_light(None, None, None) == -1
    rays = np.zeros(6, np.float32)
    irr = np.full(3, 0xABABABAB, np.uint32)
    rad = np.full(3, 0xCDCDCDCD, np.uint32)
    vis = np.full(1, 0x12121212, np.uint32)
    hit = np.full(4, 0xEFEFEFEF, np.uint32)
    r, e, q, v, h = rays.ctypes.data, irr.ctypes.data, rad.ctypes.data, vis.ctypes.data, hit.ctypes.data
    SB = native.SkyLightBatch
    for batch in (SB(0, None, None, None, None, None, 0, 0, 4, 16, 0, 0),
                  SB(1, r, e, q, v, h, 0, 0, 4, 16, 0, 0),                              # a valid batch
                  SB(1, None, e, q, v, h, 0, 0, 4, 16, 0, 0),                           # null rays
                  SB(1, r, None, None, None, h, 0, 0, 4, 16, 0, 0),                     # no output at all
                  SB(1, r, e, q, v, h, 0, 0, 0, 16, 0, 0),                              # num_samples 0
                  SB(1, r, e, q, v, h, 0, 0, 65536, 16, 0, 0),                          # ... above 65535
                  SB(1, r, e, q, v, h, 0, 0, 4, 0, 0, 0),                               # max_crossings 0
                  SB(1, r, e, q, v, h, 0, 0, 4, 257, 0, 0),                             # ... above 256
                  SB(1, r, e, q, v, h, 2, 0, 4, 16, 0, 0),                              # on_device > 1
                  SB(1, r, e, q, v, None, 0, native.FLAG_ONE_SET, 4, 16, 0, 0),         # a render-only flag
                  SB(1, r, e, q, v, None, 0, native.SEGMENT_ANY, 4, 16, 0, 0),          # another call's flags
                  SB(1, r, e, q, v, None, 0, native.DIRECT_UNSHADOWED, 4, 16, 0, 0),
                  SB(1, r, e, q, v, None, 0, native.AREA_UNSHADOWED, 4, 16, 0, 0),
                  SB(1, r, e, q, v, None, 0, native.SVGF_ROW_MAJOR, 4, 16, 0, 0),
                  SB(1, r, e, q, v, None, 0, 0x2000000, 4, 16, 0, 0),                   # a bit nobody has
                  SB(1, r, e, q, v, None, 0, native.SKY_UNSHADOWED, 4, 16, 0, 0)):      # (valid: its own flag)
        assert L.zrt_context_sky_light(None, C.byref(batch), None) == -1
    assert (irr == 0xABABABAB).all() and (rad == 0xCDCDCDCD).all() and (vis == 0x12121212).all() and \
        (hit == 0xEFEFEFEF).all()


# -------------------------------------------------------------- the sky colour
def test_env_color_is_the_oracles_bit_for_bit(oracle_mod):
    rng = np.random.default_rng(144)
    d = rng.normal(size=(1000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    for v in list(d) + [np.array(x, F) for x in ((0, 1, 0), (0, -1, 0), (1, 0, 0), (0, -0.0, 1))]:
        assert slr.env_color(v).tobytes() == oracle_mod.env_color(v).tobytes(), v
    assert list(slr.env_color(np.array([0, 1, 0], F))) == [0.5, F(0.7), 1.0]
    assert list(slr.env_color(np.array([0, -1, 0], F))) == [1.0, 1.0, 1.0]


# ------------------------------------------------------------- the hand scenes
FLOOR_BASE, FLOOR_E = (0.5, 0.25, 1.0), (0.125, 0.25, 0.5)
GLASS, OPAQUE = 1, 2


def _quad(a, b, c, d):
    """Two triangles (a, b, c), (a, c, d): the normal is (b - a) x (c - a)."""
    return [tuple(a) + tuple(b) + tuple(c), tuple(a) + tuple(c) + tuple(d)]


def floor_quad(up=True):
    a, b, c, d = (-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)                # (b - a) x (c - a) = +y
    return _quad(a, b, c, d) if up else _quad(a, d, c, b)


def dome(h):
    """Ten triangles facing the point (0, 0, 0) inside them."""
    lo = -1.0
    faces = []
    for ax, side in ((0, -1), (0, 1), (2, -1), (2, 1)):
        other = 2 - ax
        c = []
        for so, y in ((-1, lo), (1, lo), (1, h), (-1, h)):
            p = [0.0, y, 0.0]
            p[ax], p[other] = side * h, so * h
            c.append(tuple(p))
        faces.append((c, [-side if k == ax else 0 for k in range(3)]))
    faces.append(([(-h, h, -h), (h, h, -h), (h, h, h), (-h, h, h)], [0, -1, 0]))
    tris = []
    for c, inward in faces:
        n = np.cross(np.subtract(c[1], c[0]), np.subtract(c[2], c[0]))
        tris += _quad(*c) if np.dot(n, inward) > 0 else _quad(c[0], c[3], c[2], c[1])
    return tris


def hand_soup(domes=(), floor_normal=(0, 1, 0), up=True):
    """The floor, and over it domes given as (h, material)."""
    s = scenes.get_scene("sphere")
    pos, mat = floor_quad(up), [0, 0]
    for h, m in domes:
        t = dome(h)
        pos += t
        mat += [m] * len(t)
    nrm = [list(floor_normal) * 3] * 2 + [[0, 0, 0] * 3] * (len(pos) - 2)
    for k in range(2, len(pos)):                                             # the domes' own flat normals
        p = np.asarray(pos[k], np.float64).reshape(3, 3)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        nrm[k] = list(n / np.linalg.norm(n)) * 3
    desc = np.zeros((3, 3, 7), np.int32)
    for m in range(3):
        for slot, off in enumerate((0, 3, 6)):
            desc[m, slot] = (7 * m + off, 1, 1, 0, 0, 0, 0)
    texels = [*FLOOR_BASE, *FLOOR_E, 1.0,              # the floor: opaque
              0.5, 0.5, 0.5, 0, 0, 0, 0.25,            # glass of alpha 1/4
              0.5, 0.5, 0.5, 0, 0, 0, 1.0]             # the opaque roof
    return dataclasses.replace(
        s, name="sky_hand", pos=np.asarray(pos, np.float32), nrm=np.asarray(nrm, np.float32),
        uv=np.zeros((len(pos), 6), np.float32), mat=np.asarray(mat, s.mat.dtype),
        materials=[scenes.Material()] * 3, textures=[], tex_desc=desc, texels=np.asarray(texels, np.float32))


HAND_O, HAND_D = np.array([[0, 4, 0]], F), np.array([[0, -1, 0]], F)
HAND_RES = (4, 4, 4)
HAND_CASES = {"open": (), "one pane": ((1.0, GLASS),), "two panes": ((1.0, GLASS), (2.0, GLASS)),
              "roof": ((1.0, OPAQUE),)}


def hand_case(orc, name, spp, seed, **kw):
    """(ref, soup, bits, the rays) of one of HAND_CASES (or a soup of `kw`)."""
    soup = hand_soup(HAND_CASES.get(name, ()), **kw)
    ref = trace_ref.RayRef(orc, soup, HAND_RES)
    o, d = HAND_O, HAND_D
    if not kw.get("up", True):
        o, d = np.array([[0, -4, 0]], F), np.array([[0, 1, 0]], F)       # (not -HAND_D: a -0 component walks the grid the other way)
    bits, _ = ref.trace_batch(o, d)
    return ref, soup, o, d, bits, slr.make_rays(orc, ref, soup, o, d, bits, spp, seed=seed)


def test_hand_scene_with_exact_answers(oracle_mod):
    S = 16
    got = {}
    for name in HAND_CASES:
        ref, soup, o, d, bits, rays = hand_case(oracle_mod, name, S, seed=11)
        assert bits[0, 0].view(F) == 4.0 and ref.indices[bits[0, 3]] < 2, name        # the floor, from above
        f = rays[0].words.view(F)
        assert rays[0].shaded and list(rays[0].N) == [0, 1, 0] and f[0] == 0 and f[2] == 0 and -1e-6 < f[1] <= 0
        assert len(rays[0].items) == S and all(it.traced and it.d[1] > 0 for it in rays[0].items)
        got[name] = (ref, soup, rays, slr.sky_batch(ref, soup, rays, S))
    base, emis = np.array(FLOOR_BASE, F), np.array(FLOOR_E, F)
    # the open floor: every chain is one segment that meets nothing
    ref, soup, rays, (E, R, V, tot) = got["open"]
    E1, R1, V1, tot1 = slr.sky_batch(ref, soup, rays, S, unshadowed=True)
    assert V.view(F)[0] == 1.0 and (R == R1).all() and (E == E1).all() and (V == V1).all()
    assert tot == dict(tot, samples=S, segments=S, hits=0) and tot1 == dict(tot1, samples=S, segments=0, hits=0)
    mean = np.mean([it.L.astype(np.float64) for it in rays[0].items], axis=0)
    assert np.allclose(E.view(F)[0], mean * np.pi, rtol=1e-6) and np.allclose(R.view(F)[0], emis + base * mean, rtol=1e-6)
    assert (R.view(F)[0] > emis).all()
    # one pane of alpha 1/4 over the whole hemisphere: every T is 3/4 and the partial sums k * 3/4 are exact
    _, _, _, (Ep, Rp, Vp, totp) = got["one pane"]
    assert Vp.view(F)[0] == 0.75 and totp == dict(totp, samples=S, segments=2 * S, hits=S)
    assert np.allclose(Ep.view(F)[0], E.view(F)[0] * 0.75, rtol=1e-6)
    # two panes: 9/16
    ref2, soup2, rays2, (E2, R2, V2, tot2) = got["two panes"]
    assert V2.view(F)[0] == 0.5625 and tot2 == dict(tot2, samples=S, segments=3 * S, hits=2 * S)
    assert np.allclose(R2.view(F)[0], emis + base * mean * 0.5625, rtol=1e-6)
    # ... and a cap of 1 stops every chain after its first crossing: the product so far stands
    Ec, Rc, Vc, totc = slr.sky_batch(ref2, soup2, rays2, S, cap=1)
    assert Vc.view(F)[0] == 0.75 and totc["hits"] == totc["samples"] == S and totc["segments"] == S
    assert (Ec == Ep).all() and (Rc == Rp).all()
    # the opaque roof: nothing arrives; one chain segment per traced sample
    _, _, _, (Er, Rr, Vr, totr) = got["roof"]
    assert not Er.any() and not Vr.any() and Rr.tobytes() == emis.tobytes()
    assert totr == dict(totr, samples=S, segments=S, hits=S)
    # a ray that misses
    ref, soup, rays, _ = got["open"]
    o, d = np.array([[0, 4, 0]], F), np.array([[0, 1, 0]], F)
    bits, _ = ref.trace_batch(o, d)
    assert bits[0, 3] == trace_ref.MISS
    miss = slr.make_rays(oracle_mod, ref, soup, o, d, bits, S)
    Em, Rm, Vm, totm = slr.sky_batch(ref, soup, miss, S)
    assert miss[0].words is None and not Em.any() and not Rm.any() and not Vm.any() and totm["samples"] == 0
    # a zero interpolated normal: N is NaN, the ray is not shaded
    ref, soup, o, d, bits, rays = hand_case(oracle_mod, "open", S, seed=11, floor_normal=(0, 0, 0))
    assert bits[0, 3] != trace_ref.MISS and not rays[0].shaded and rays[0].items == []
    Ez, Rz, Vz, totz = slr.sky_batch(ref, soup, rays, S)
    assert not Ez.any() and not Vz.any() and Rz.tobytes() == emis.tobytes()
    assert (totz["samples"], totz["segments"], totz["hits"]) == (0, 0, 0)


TILTED = (0.6, 0.8, 0.0)


@pytest.mark.parametrize("which", ["up", "down", "tilted"])
def test_the_unoccluded_hemisphere_against_the_closed_form(which, oracle_mod):
    """A cosine-weighted direction about a unit N has the mean (2/3) N and the
    sky is linear in d.y, so the samples' mean tends to the sky's colour at
    t = 0.5 (1 + (2/3) N.y).  32 batches of 256 unshadowed samples: the grand
    mean lies within 6 standard errors of the batch means of it.  Visibility
    is 1 in every batch: every sample is traced."""
    kw = {"up": {}, "down": dict(floor_normal=(0, -1, 0), up=False), "tilted": dict(floor_normal=TILTED)}[which]
    means = np.zeros((tah.BATCHES, 3))
    for k in range(tah.BATCHES):
        ref, soup, o, d, bits, rays = hand_case(oracle_mod, "open", tah.SPP, seed=3000 + k, **kw)
        E, R, V, tot = slr.sky_batch(ref, soup, rays, tah.SPP, unshadowed=True)
        assert rays[0].shaded and tot["samples"] == tah.SPP and V.view(F)[0] == 1.0
        means[k] = E.view(F)[0].astype(np.float64) / float(slr.PI)
    N = rays[0].N.astype(np.float64)
    assert abs(np.linalg.norm(N) - 1) < 1e-6 and np.allclose(N, {"up": (0, 1, 0), "down": (0, -1, 0), "tilted": TILTED}[which])
    t = 0.5 * (1.0 + (2.0 / 3.0) * N[1])
    want = (1.0 - t) + np.array([0.5, 0.7, 1.0]) * t
    grand, se = means.mean(0), means.std(0, ddof=1) / np.sqrt(tah.BATCHES)
    print(which, "mean", grand.tolist(), "closed form", want.tolist(), "difference / standard error",
          (np.abs(grand - want)[:2] / se[:2]).tolist())
    assert (se[:2] > 0).all() and (np.abs(grand - want)[:2] <= 6 * se[:2]).all(), (grand, want, se)
    # the blue channel is (1 - t) + 1 * t: 1 whatever the direction, so it has no sampling error to measure by.
    # What moves it is rounding alone: a sample's colour within 2^-23 of 1, then 256 float32 additions of at most
    # 2^-24 relative error each, the division and the factor pi: below 2^-15
    assert want[2] == 1.0 and (np.abs(means[:, 2] - 1.0) < 2.0 ** -15).all(), means[:, 2]


# ------------------------------------------- agreement with the path tracer
def open_box_soup():
    """test_area_lights_host.box_soup without its lamp and without its face
    y = +1: an opaque box of unit flat normals, open to the sky above, with
    no emitter."""
    s = tah.box_soup()
    keep = [k for k in range(12) if k not in (6, 7)]
    assert (s.pos.reshape(-1, 3, 3)[[6, 7], :, 1] == 1).all()
    return dataclasses.replace(s, name="sky_box", pos=s.pos[keep], nrm=s.nrm[keep], uv=s.uv[keep], mat=s.mat[keep])


OPEN_D = [(0.2, 0.1, -1.0), (-0.5, 0.3, -1.0), (1.0, 0.2, -0.3), (-1.0, -0.4, 0.2), (0.3, -1.0, -0.1), (-0.2, -1.0, 0.5),
          (0.6, 0.5, 1.0), (-0.1, 0.2, 1.0)]


def compare(a, b, what):
    ma, mb, va, vb = a.mean(0), b.mean(0), a.var(0, ddof=1), b.var(0, ddof=1)
    sigma = np.sqrt(va / len(a) + vb / len(b))
    with np.errstate(all="ignore"):
        print(what, "difference / sigma:", np.round(np.abs(ma - mb) / sigma, 2).tolist())
        print(what, "std(path tracer) / std(direct calls):", np.round(np.sqrt(va / vb), 2).tolist())
    print(what, "means:", ma.tolist(), mb.tolist())
    assert (np.abs(ma - mb) <= 6 * sigma).all(), (what, ma, mb, sigma)
    return ma, mb


def test_the_sky_alone_agrees_with_the_path_tracer(oracle_mod):
    """Two estimates of one integral per ray and channel: the oracle's linear
    radiance at max_bounce 2 (base colour * E[the sky where the second segment
    misses]; nothing emits) and the reference's `radiance`; each as 32 batches
    of distinct seeds at 256 samples, compared by |mean_a - mean_b| <=
    6 sqrt(var_a / 32 + var_b / 32) with the variances over the batch means.

    Measured (seeds 1000.. and 2000..): the largest |difference| / sigma over
    the 8 rays x 3 channels is 1.78; the two sides' batch standard deviations are
    within a factor 0.78 to 1.40 of each other: the same estimator but for the draw."""
    soup = open_box_soup()
    res = (2, 2, 2)
    ref = trace_ref.RayRef(oracle_mod, soup, res)
    o = np.tile(np.array(tah.BOX_O, F), (len(OPEN_D), 1))
    d = np.array([np.array(v) / np.linalg.norm(v) for v in OPEN_D], F)
    bits, _ = ref.trace_batch(o, d)
    assert (bits[:, 3] != trace_ref.MISS).all()
    assert alr.EmitterSet.of_soup(soup).count == 0
    pt = radiance_ref.RadianceRef(oracle_mod, soup, res)
    a = np.zeros((tah.BATCHES, len(o), 3))
    b = np.zeros((tah.BATCHES, len(o), 3))
    vis = np.zeros((tah.BATCHES, len(o)))
    for k in range(tah.BATCHES):
        a[k] = pt.radiance(o, d, tah.SPP, 2, seed=1000 + k)[0]
        rays = slr.make_rays(oracle_mod, ref, soup, o, d, bits, tah.SPP, seed=2000 + k)
        _, R, V, tot = slr.sky_batch(ref, soup, rays, tah.SPP)
        b[k], vis[k] = R.view(F), V.view(F)
        assert tot["samples"] == len(o) * tah.SPP
    ma, mb = compare(a, b, "open box")
    assert (ma > 0).all() and (mb > 0).all() and ((vis.mean(0) > 0.02) & (vis.mean(0) < 0.6)).all(), vis.mean(0)


def test_emitters_plus_sky_is_the_direct_light(oracle_mod):
    """"Emitters plus sky is the direct light" on test_area_lights_host's box,
    which has a lamp: area-light radiance + sky-light radiance - emissive
    against the oracle at max_bounce 2, by the criterion above.  That box is
    closed, so every sky sample is blocked and the sky-light radiance is the
    emission exactly: the sum must not count the emission twice, and the sky
    term must add nothing where no sky is seen."""
    soup = tah.box_soup()
    res = (2, 2, 2)
    ref = trace_ref.RayRef(oracle_mod, soup, res)
    o = np.tile(np.array(tah.BOX_O, F), (len(tah.BOX_D), 1))
    d = np.array([np.array(v) / np.linalg.norm(v) for v in tah.BOX_D], F)
    bits, _ = ref.trace_batch(o, d)
    es = alr.EmitterSet.of_soup(soup)
    pt = radiance_ref.RadianceRef(oracle_mod, soup, res)
    emis = np.zeros((len(o), 3))
    a = np.zeros((tah.BATCHES, len(o), 3))
    b = np.zeros((tah.BATCHES, len(o), 3))
    for k in range(tah.BATCHES):
        a[k] = pt.radiance(o, d, tah.SPP, 2, seed=1000 + k)[0]
        ar = alr.make_rays(oracle_mod, ref, soup, es, o, d, bits, tah.SPP, seed=2000 + k)
        sr = slr.make_rays(oracle_mod, ref, soup, o, d, bits, tah.SPP, seed=4000 + k)
        _, Rs, Vs, _ = slr.sky_batch(ref, soup, sr, tah.SPP)
        for i, ray in enumerate(sr):
            emis[i] = ray.words.view(F)[12:15]
        assert not Vs.any() and np.array_equal(Rs.view(F), emis.astype(F))
        b[k] = alr.area_batch(ref, soup, ar, tah.SPP)[1].view(F).astype(np.float64) + Rs.view(F) - emis
    ma, mb = compare(a, b, "closed box with a lamp")
    assert (ma[:6] > 0).all() and (ma[7] == [8, 6, 4]).all() and (mb[7] == [8, 6, 4]).all()


# ------------------------------------------------ the fuzz rays: what they reach
FUZZ_SPP = 4


def cached_rays(orc, cs):
    """The Ray objects of a fuzz seed's rays at FUZZ_SPP samples, seed = the
    case's seed, made once and kept on the case with the chains they walk."""
    if not hasattr(cs, "_sky_rays"):
        cs._sky_rays = slr.make_rays(orc, cs.ref, cs.soup, cs.o, cs.d, cs.bits, FUZZ_SPP, seed=cs.seed)
    return cs._sky_rays


@pytest.fixture(scope="module")
def case(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed]
    return get


def coverage(orc, cases):
    n = dict.fromkeys(("rays", "miss", "unshaded", "open", "blocked", "partial", "partial_T", "capped_at_1", "capped_at_2",
                       "untraced"), 0)
    for cs in cases:
        rays = cached_rays(orc, cs)
        _, _, V, _ = slr.sky_batch(cs.ref, cs.soup, rays, FUZZ_SPP)
        for ray, v in zip(rays, V.view(F)):
            n["rays"] += 1
            if ray.words is None:
                n["miss"] += 1
                continue
            if not ray.shaded:
                n["unshaded"] += 1
                continue
            n["untraced"] += sum(not it.traced for it in ray.items)
            chains = [it.chain(cs.ref, cs.soup) for it in ray.items if it.traced]
            n["capped_at_1"] += any(c.cut(1)[5] == "cap" for c in chains)
            if v == 1:
                n["open"] += 1
            elif v == 0:
                n["blocked"] += 1
            else:
                n["partial"] += 1
                n["partial_T"] += any(0 < c.cut(slr.CAP)[0] < 1 for c in chains)
                n["capped_at_2"] += any(c.cut(2)[5] == "cap" for c in chains)
    return n


POISON_SEED = 4


def poisoned_case(orc, cs):
    """direct_ref.PoisonedCase of a fuzz case, with the case's seed for the samples."""
    import direct_ref
    pc = direct_ref.PoisonedCase(orc, cs)
    pc.seed = cs.seed
    return pc


def test_the_fuzz_seeds_reach_what_the_call_has_to_get_right(case, oracle_mod):
    """Counted from the reference alone: seeds 0..39, all 128 rays, 4 samples
    each, chains under 16 crossings.  Counted: 5120 rays; 3337 miss; of the
    1783 that hit, 866 are fully open (visibility 1), 239 fully blocked (0) and
    678 in between; of those, 128 have a sample whose chain ends with
    0 < T < 1, 137 a chain that a cap of 1 cuts and 48 one that a cap of 2
    cuts (no chain reaches 16 crossings in these soups; the GPU test runs the
    caps 16, 1 and 2).  The floors are half of these.  Every sample of a shaded
    ray is traced: N + u vanishes only for u = -N exactly.

    No seed has a hit that is not shaded: a fuzz soup's vertex normals are its
    face normals plus noise of 0.05, finite and never near zero.  The class is
    counted on seed 4's soup with the normals of three hit triangles
    overwritten (direct_ref.PoisonedCase), as the direct-light tests count it,
    and made by hand in test_hand_scene_with_exact_answers."""
    n = coverage(oracle_mod, (case(s) for s in qf.SEEDS))
    print(n)
    assert n["rays"] == n["miss"] + n["unshaded"] + n["open"] + n["blocked"] + n["partial"] == 128 * len(qf.SEEDS), n
    assert n["miss"] >= 1668 and n["open"] >= 433 and n["blocked"] >= 119 and n["partial"] >= 339, n
    assert n["partial_T"] >= 64 and n["capped_at_1"] >= 68 and n["capped_at_2"] >= 24, n
    assert n["unshaded"] == 0 and n["untraced"] == 0, n
    p = coverage(oracle_mod, [poisoned_case(oracle_mod, case(POISON_SEED))])
    print(p)
    assert p["unshaded"] >= 5, p
