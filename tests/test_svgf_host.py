"""Illumination, moments and the variance-guided filter
(zrt_context_illumination, zrt_context_svgf), the part that runs without a GPU:
the C ABI's declarations, flag, exports and bindings, the batches' layouts
against the header's own comments, the argument errors that come back before
any device work, properties of the numpy reference (svgf_ref.py) that hold
whatever the GPU does, and the quality condition of the wrapper's defaults.

The quality condition: Cornell and the textured fuzz scene of test_tall_gpu.py
at 33 x 31, grid 16^3, max_bounce 4; six frames of 4 samples, frame k at seed
`seed + 1000 k`; the guides are feature_ref.py's planes at each frame's seed;
reproject_ref.py with native.REPROJECT_DEFAULTS carries the illumination, the
moments and the lengths from frame to frame.  One sequence per scene has a
static camera; one applies the "both" move of test_reproject_host.MOVES
between frames 2 and 3.  The error is the mean absolute linear error against
the oracle's 256-sample frame at the frame's camera.  At every frame the
filtered, remodulated frame must be closer than the reprojected-only frame; on
the static sequences at frames 3 to 5 at least half of the pixels must have
taken the temporal variance (a condition, not a measurement: it keeps a run
without moments from passing).  denoise_ref.py at native.DENOISE_SIGMAS over
the same history is printed beside it and not asserted on.  Seen with this
reference (reprojected only, denoise_ref, svgf_ref, share of temporal pixels):
  cornell static  0  0.155396  0.106907  0.114616  0.000
  cornell static  1  0.122544  0.077258  0.105933  0.000
  cornell static  2  0.107192  0.068862  0.079938  0.000
  cornell static  3  0.100749  0.063514  0.057150  0.741
  cornell static  4  0.092305  0.059870  0.052252  0.750
  cornell static  5  0.092562  0.063056  0.054145  0.738
  cornell moved   3  0.107414  0.088553  0.082020  0.693
  cornell moved   4  0.105548  0.082417  0.083428  0.714
  cornell moved   5  0.099411  0.076235  0.075147  0.767
  fuzz    static  0  0.018472  0.008675  0.008379  0.000
  fuzz    static  1  0.013186  0.007822  0.007259  0.000
  fuzz    static  2  0.010863  0.007385  0.006785  0.000
  fuzz    static  3  0.010326  0.007216  0.006263  0.900
  fuzz    static  4  0.009239  0.007249  0.006086  0.900
  fuzz    static  5  0.008496  0.006959  0.005853  0.897
  fuzz    moved   3  0.009239  0.005953  0.005984  0.566
  fuzz    moved   4  0.008026  0.005679  0.005649  0.531
  fuzz    moved   5  0.007109  0.005229  0.005347  0.525
(frames 0 to 2 of a moved sequence are the static sequence's).
"""
import ctypes as C
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import camera_for, native

import denoise_ref as dr
import feature_ref
import refine_cases as rc
import reproject_ref as rr
import svgf_ref as sr
import test_reproject_host as rh
from test_denoise_host import _header, _struct

F = np.float32
INF = float("inf")
NAN = float("nan")


def test_header_declares_both_calls_and_native_exports_and_binds_them():
    hdr = _header()
    for fn, batch in (("zrt_context_illumination", "zrt_illumination_batch"), ("zrt_context_svgf", "zrt_svgf_batch")):
        assert re.search(r"\bint\s+%s\s*\(\s*zrt_context\s*\*\s*\w*\s*,\s*const\s+%s\s*\*\s*\w*\s*,\s*zrt_stats\s*\*"
                         % (fn, batch), hdr)
        assert fn in native.EXPORTS
        assert hasattr(native.lib(), fn)                           # (dlsym: libzrt.so exports it)
    sec = "svgf: luminance moments and a variance-guided a-trous filter (ABI 2, added)"
    assert hdr.index("reproject: carry a frame's history across a camera change (ABI 2, added)") < hdr.index(sec) < \
        hdr.index("typedef struct zrt_group zrt_group")
    # the next free bit after ZRT_REPROJECT_ROW_MAJOR
    assert re.search(r"#define\s+ZRT_REPROJECT_ROW_MAJOR\s+0x200000u", hdr)
    assert re.search(r"#define\s+ZRT_SVGF_ROW_MAJOR\s+0x400000u", hdr) and native.SVGF_ROW_MAJOR == 0x400000
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and native.lib().zrt_abi_version() == 2
    for name in ("illumination_raw", "illumination", "svgf_raw", "svgf"):
        assert callable(getattr(native.Context, name))
    assert callable(native.Film.illumination) and callable(native.SvgfHistory.update)
    assert native.SVGF_SIGMAS == (4.0, 0.5, 0.1)


@pytest.mark.parametrize("cls, name, size", ((native.IlluminationBatch, "zrt_illumination_batch", 72),
                                             (native.SvgfBatch, "zrt_svgf_batch", 120)))
def test_batch_layouts_are_the_headers(cls, name, size):
    names, tail = _struct(_header(), name)
    assert names == [n for n, _ in cls._fields_]
    m = re.search(r"(\d+)\s*B;\s*offsets((?:\s+\d+)+)", tail)
    assert m, tail
    assert C.sizeof(cls) == int(m.group(1)) == size
    assert [getattr(cls, n).offset for n in names] == [int(x) for x in m.group(2).split()]


# ------------------------------------------------------------------ refusals
P8 = 64
GUARD = 0xA0A0A0A0


def illumination_planes():
    return [np.full((P8, 3), 0.5, F), np.full((P8, 3), 0.25, F)]


def illumination_outputs():
    return [np.full(3 * P8, GUARD, np.uint32), np.full(3 * P8, GUARD + 1, np.uint32)]


def illumination_valid(x, outs):
    """A batch that passes every check that needs no device: 8 x 8, an albedo, host pointers."""
    return dict(w=8, h=8, tile_size=8, color=x[0].ctypes.data, film=None, albedo=x[1].ctypes.data,
                illumination=outs[0].ctypes.data, moments=outs[1].ctypes.data, on_device=0, flags=0, _reserved=0)


ILLUMINATION_REFUSALS = {
    "w 0": dict(w=0), "h 0": dict(h=0), "P above 2^31": dict(w=1 << 16, h=(1 << 15) + 1),
    "tile not a multiple of 8": dict(tile_size=12),
    "no colour source": dict(color=None),
    "color and film": dict(film=0x1000),
    "film with row major": dict(color=None, film=0x1000, flags=native.SVGF_ROW_MAJOR),
    "no output": dict(illumination=None, moments=None),
    "on_device 2": dict(on_device=2),
    "_reserved": dict(_reserved=1),
    "the denoiser's flag": dict(flags=native.DENOISE_ROW_MAJOR),
    "the reprojection's flag": dict(flags=native.REPROJECT_ROW_MAJOR),
    "a render flag": dict(flags=native.FLAG_COUNT_STATS),
    "a flag beside the valid one": dict(flags=native.SVGF_ROW_MAJOR | 0x800000),
}
ILLUMINATION_ALLOWED = {
    "no albedo": dict(albedo=None), "illumination only": dict(moments=None), "moments only": dict(illumination=None),
    "P = 2^31": dict(w=1 << 16, h=1 << 15),
    "row major ignores tile_size": dict(flags=native.SVGF_ROW_MAJOR, tile_size=12),
    "tile_size 0": dict(tile_size=0),
}


def svgf_planes():
    """colour, moments, length, normal, depth, albedo of a valid 8 x 8 call."""
    n = np.zeros((P8, 3), F)
    n[:, 2] = 1
    return [np.full((P8, 3), 0.5, F), np.full((P8, 3), 0.25, F), np.full(P8, 5, np.uint32), n, np.full(P8, 6.0, F),
            np.full((P8, 3), 0.75, F)]


def svgf_outputs():
    return [np.full(3 * P8, GUARD, np.uint32), np.full(3 * P8, 0xB1, np.uint8), np.full(P8, GUARD + 2, np.uint32)]


def svgf_untouched(outs):
    return (outs[0] == GUARD).all() and (outs[1] == 0xB1).all() and (outs[2] == GUARD + 2).all()


def svgf_valid(x, outs):
    """A batch that passes every check that needs no device: 8 x 8, everything given, host pointers."""
    c, m, l, n, z, a = (p.ctypes.data for p in x)
    return dict(w=8, h=8, tile_size=8, iterations=5, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=0.1, color=c,
                moments=m, length=l, normal=n, depth=z, albedo=a, linear=outs[0].ctypes.data, rgb=outs[1].ctypes.data,
                variance=outs[2].ctypes.data, on_device=0, flags=0, _reserved=0)


SVGF_REFUSALS = {
    "w 0": dict(w=0), "h 0": dict(h=0), "P above 2^31": dict(w=1 << 16, h=(1 << 15) + 1),
    "tile not a multiple of 8": dict(tile_size=12),
    "iterations 0": dict(iterations=0), "iterations 9": dict(iterations=9),
    "sigma_luminance 0": dict(sigma_luminance=0.0), "sigma_luminance negative": dict(sigma_luminance=-1.0),
    "sigma_luminance NaN": dict(sigma_luminance=NAN), "sigma_luminance -inf": dict(sigma_luminance=-INF),
    "sigma_normal 0": dict(sigma_normal=0.0), "sigma_normal NaN": dict(sigma_normal=NAN),
    "sigma_depth negative": dict(sigma_depth=-0.5), "sigma_depth NaN": dict(sigma_depth=NAN),
    "no colour": dict(color=None),
    "no output": dict(linear=None, rgb=None, variance=None), "variance alone is no output": dict(linear=None, rgb=None),
    "on_device 2": dict(on_device=2),
    "_reserved": dict(_reserved=1),
    "the denoiser's flag": dict(flags=native.DENOISE_ROW_MAJOR),
    "the reprojection's flag": dict(flags=native.REPROJECT_ROW_MAJOR),
    "a render flag": dict(flags=native.FLAG_COUNT_STATS),
    "a flag beside the valid one": dict(flags=native.SVGF_ROW_MAJOR | 0x800000),
}
SVGF_ALLOWED = {
    "sigma +inf": dict(sigma_luminance=INF, sigma_normal=INF, sigma_depth=INF),
    "an absent guide's sigma is not read": dict(normal=None, sigma_normal=NAN, depth=None, sigma_depth=0.0),
    "P = 2^31": dict(w=1 << 16, h=1 << 15),
    "row major ignores tile_size": dict(flags=native.SVGF_ROW_MAJOR, tile_size=12),
    "linear only": dict(rgb=None), "rgb only": dict(linear=None), "no variance": dict(variance=None),
    "8 iterations": dict(iterations=8), "1 iteration": dict(iterations=1),
    "no moments": dict(moments=None), "no lengths": dict(length=None), "no albedo": dict(albedo=None),
}


def test_both_calls_reject_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included),
    and the outputs stay as they were."""
    L = native.lib()
    assert L.zrt_context_illumination(None, None, None) == -1 and L.zrt_context_svgf(None, None, None) == -1
    st = native.Stats()
    x, outs = illumination_planes(), illumination_outputs()
    for change in [{}] + list(ILLUMINATION_REFUSALS.values()) + list(ILLUMINATION_ALLOWED.values()):
        batch = native.IlluminationBatch(**{**illumination_valid(x, outs), **change})
        assert L.zrt_context_illumination(None, C.byref(batch), C.byref(st)) == -1
    assert (outs[0] == GUARD).all() and (outs[1] == GUARD + 1).all()
    x, outs = svgf_planes(), svgf_outputs()
    for change in [{}] + list(SVGF_REFUSALS.values()) + list(SVGF_ALLOWED.values()):
        batch = native.SvgfBatch(**{**svgf_valid(x, outs), **change})
        assert L.zrt_context_svgf(None, C.byref(batch), C.byref(st)) == -1
    assert svgf_untouched(outs)
    assert st.samples == 0 and st.trace_launches == 0


def test_denoise_and_reproject_still_refuse_the_new_flag():
    """Their own refusal tables name the bit (reproject's "a flag beside the
    valid one" is this one); on a real context test_svgf_gpu.py sends it."""
    assert rh.REFUSALS["a flag beside the valid one"] == dict(flags=native.REPROJECT_ROW_MAJOR | native.SVGF_ROW_MAJOR)
    assert native.SVGF_ROW_MAJOR & (native.DENOISE_ROW_MAJOR | native.REPROJECT_ROW_MAJOR) == 0
    hdr = _header()
    for batch in ("zrt_denoise_batch", "zrt_reproject_batch"):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (batch, batch), hdr, re.S).group(1)
        assert "any other bit is ZRT_ERR_INVALID_ARG" in body


# --------------------------------------------------- properties of the reference
def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_without_an_albedo_the_illumination_is_the_colours_bits():
    rng = np.random.default_rng(21)
    c = (rng.random((7, 9, 3)) * 4 - 1).astype(F)
    c[0, 0] = (-0.0, np.inf, 0.0)
    c[1, 1, 2] = np.array([0x7FC01234], np.uint32).view(F)[0]
    I, m = sr.illumination(c)
    assert np.array_equal(_bits(I), _bits(c))
    l = sr.lum(c)
    assert np.array_equal(_bits(m[..., 0]), _bits(l)) and (_bits(m[..., 2]) == 0).all()
    with np.errstate(all="ignore"):
        assert np.array_equal(_bits(m[..., 1]), _bits(l * l))


def test_demodulate_then_remodulate_returns_the_colour_to_within_one_ulp():
    """I = c / d and f = I * d round once each: the exact I * d is within
    |c| 2^-24 < 1 ulp(c) of c, and rounding it to nearest moves it by at most
    half an ulp, so f is c or one of its neighbours."""
    rng = np.random.default_rng(22)
    c = (rng.random((40, 50, 3)) * 4).astype(F)
    a = rng.random((40, 50, 3)).astype(F)
    a[:5] *= F(0.05)                                               # below the floor
    a[5, 0] = (NAN, 0.0, -1.0)                                     # all floored to 2^-4
    I, _ = sr.illumination(c, a)
    assert np.array_equal(_bits(I[5, 0]), _bits(c[5, 0] / F(0.0625)))
    back = I * sr.dmod(a)
    ulps = np.abs(back.astype(np.float64) - c) / np.spacing(c).astype(np.float64)
    print("demodulate, remodulate: largest move %.2f ulp, %d of %d components moved" %
          (ulps.max(), int((ulps > 0).sum()), c.size))
    assert ulps.max() <= 1.0


def _constant(value, guides, shape=(11, 14)):
    c = np.empty(shape + (3,), F)
    c[:] = value
    if not guides:
        return c, {}
    n = np.zeros_like(c)
    n[..., 1] = 1
    return c, dict(normal=n, sigma_normal=0.5, depth=np.full(shape, 3.7, F), sigma_depth=0.1)


# colours of short significands whose luminance is 9 bits or shorter, and black
SHORT_LUM = ((0.125, 0.125, 0.125), (2.0, 2.0, 2.0), (0.0, 0.875, 4.75), (0.125, 1.0, 4.875), (0.0, 0.0, 0.0))
# significands of at most 12 bits, any luminance (test_denoise_host.SHORT)
SHORT = ((0.5, 0.25, 2.0), (1.0, 3.0, 0.75), (4095.0, -1.5, 2.0 ** -100), (2.0 ** 100, 0.3125, -17.0))


def test_a_constant_image_is_a_fixed_point_bit_for_bit():
    """Every luminance difference of a constant frame is 0, so xl = 0 * kl = 0
    (kl is finite: den >= 2^-16), every wl and guide factor is 1 and each tap's
    weight is exactly k: the colour is a fixed point for significands of at
    most 12 bits by test_denoise_host's argument, whatever the variance is.

    v_0 = 0 exactly needs more: in the spatial estimate S1 = j * l and
    S2 = j * l^2 (j <= 49) must be exact, which holds when the *luminance* has
    a significand of at most 9 bits (l^2: 18 bits, j l^2: 24); then m1 = l,
    m2 = l^2 = m1 * m1.  The colour's significand being short does not make
    the luminance's short, so for the other values the estimate is bounded
    instead: 49 sums and two divisions, each within 2^-24 relative, on both
    moments, (4 / 1) on top: v_0 <= 4 * 160 * 2^-24 * l^2.  Through the
    temporal branch v_0 = 0 for any value: m.y and m.x * m.x are one product."""
    for value in SHORT_LUM + SHORT:
        for guides in (False, True):
            c, g = _constant(value, guides)
            for it in (1, 5, 8):
                r = sr.svgf(c, it, 4.0, **g)
                out = r["linear"]
                same = _bits(out) == _bits(c)
                assert out.dtype == F and (same | ((out == 0) & (c == 0))).all(), (value, it, guides)
                if value in SHORT_LUM:
                    assert (_bits(r["v0"]) == 0).all() and (_bits(r["variance"]) == 0).all(), (value, guides)
                else:
                    l = float(sr.lum(c[0, 0]))
                    assert (r["v0"].astype(np.float64) <= 4 * 160 * 2.0 ** -24 * l * l).all() and (r["variance"] <= r["v0"].max()).all()
            _, m = sr.illumination(c)
            r = sr.svgf(c, 5, 4.0, moments=m, length=np.full(c.shape[:2], 4, np.uint32), **g)
            assert (_bits(r["v0"]) == 0).all() and r["hits"] == c.shape[0] * c.shape[1]
            assert ((_bits(r["linear"]) == _bits(c)) | ((r["linear"] == 0) & (c == 0))).all()


def _step(left, right, h=16, w=20):
    c = np.empty((h, w, 3), F)
    c[:, :w // 2] = left
    c[:, w // 2:] = right
    return c


def test_zero_variance_lets_no_level_mix_across_a_luminance_step():
    """v = 0 everywhere (moments of the frame itself, lengths 4): g = 0,
    den = 2^-16, kl = 2^32, so a tap whose luminance differs by 2^-16 or more
    has xl >= 1 and wl = 0.  The two sides are constant with short
    significands: each is a fixed point, and the frame comes back bit for bit."""
    c = _step((0.125, 0.125, 0.125), (0.25, 0.25, 0.25))
    _, m = sr.illumination(c)
    n4 = np.full(c.shape[:2], 4, np.uint32)
    for it in (1, 5, 8):
        r = sr.svgf(c, it, 4.0, moments=m, length=n4)
        assert np.array_equal(_bits(r["linear"]), _bits(c)) and (_bits(r["variance"]) == 0).all()
    # the control: the spatial estimate sees the step as variance near it, and the same frame mixes
    assert not np.array_equal(_bits(sr.svgf(c, 1, 4.0)["linear"]), _bits(c))


def test_a_large_variance_on_one_side_mixes_from_that_side_only():
    """Moments that give the right half a variance of 1 and the left half 0,
    one level: a pixel's kl comes from the 3 x 3 Gaussian of the variance
    around it.  Right of the step the weight is wide (sigma 4: the step of
    0.125 costs (0.125 / 4)^2): those pixels take taps from the left and
    move towards it.  Left of the step, two or more pixels away, g = 0 and
    nothing crosses: bit for bit.  (The column next to the step has g > 0
    through its right-hand neighbours and does mix.)"""
    c = _step((0.125, 0.125, 0.125), (0.25, 0.25, 0.25))
    h, w = c.shape[:2]
    _, m = sr.illumination(c)
    m[:, w // 2:, 1] += F(1.0)
    r = sr.svgf(c, 1, 4.0, moments=m, length=np.full((h, w), 4, np.uint32))
    assert (r["v0"][:, :w // 2] == 0).all() and (r["v0"][:, w // 2:] == 1).all()
    out = r["linear"]
    assert np.array_equal(_bits(out[:, :w // 2 - 1]), _bits(c[:, :w // 2 - 1]))
    for col in (w // 2, w // 2 + 1):
        assert ((out[:, col] < 0.25) & (out[:, col] > 0.125)).all()
    assert np.array_equal(_bits(out[:, w // 2 + 2:]), _bits(c[:, w // 2 + 2:]))   # out of the step's reach: constant
    assert ((out[:, w // 2 - 1] > 0.125) & (out[:, w // 2 - 1] < 0.25)).all()


def _noisy(seed, h=19, w=23):
    rng = np.random.default_rng(seed)
    c = (rng.random((h, w, 3)) * 2).astype(F)
    n = rng.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    n[:, : w // 2] = n[0, 0]
    z = (F(4.0) + rng.random((h, w)).astype(F) * F(0.2)).astype(F)
    a = rng.random((h, w, 3)).astype(F)
    return c, n, z, a


def test_a_level_never_raises_the_variance_above_its_taps():
    """v' = sum v_q wt_q^2 / (sum wt_q)^2 <= max v_q, since sum wt^2 <= (sum
    wt)^2 for non-negative weights.  In f32: 25 products and sums on each side
    and a division, each within 2^-24: 64 * 2^-24 relative is generous."""
    c, n, z, _ = _noisy(23)
    rng = np.random.default_rng(24)
    v = (rng.random(c.shape[:2]) ** 4).astype(F)
    h, w = v.shape
    for step in (1, 2, 4):
        for g in ({}, dict(normal=n, kn=F(4.0), depth=z, kz=F(100.0))):
            _, v1 = sr.level(c, v, step, 4.0, **g)
            top = np.zeros_like(v)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if abs(dx * step) >= w or abs(dy * step) >= h:
                        continue
                    P, Q = sr._shifted(v, dx * step, dy * step)
                    top[P] = np.maximum(top[P], v[Q])
            assert (v1 <= top * (1 + 64 * 2.0 ** -24)).all(), step
            assert (v1 < top).mean() > 0.9                          # and it does lower it: that is the filter


def test_a_nan_pixel_stays_and_costs_its_neighbours_one_tap():
    c, _, _, _ = _noisy(25, 20, 20)
    bad = c.copy()
    nan = np.array([0x7FC01234], np.uint32).view(F)[0]             # a payload: the input's bits come back
    bad[9, 10, 1] = nan
    for sigma in (0.75, 4.0, INF):
        for it in (1, 3):
            got = sr.svgf(bad, it, sigma)
            assert np.array_equal(_bits(got["linear"][9, 10]), _bits(bad[9, 10]))
            assert np.isnan(got["linear"]).sum() == 1 and np.isfinite(got["variance"]).all()
    # one level: its luminance is skipped by the 7 x 7 estimates around it, those reach the 3 x 3 Gaussians one
    # further out and those the 5 x 5 taps two further: beyond 6 pixels the clean image's bits
    got, clean = sr.svgf(bad, 1, 4.0), sr.svgf(c, 1, 4.0)
    far = np.ones((20, 20), bool)
    far[3:16, 4:17] = False
    assert np.array_equal(_bits(got["linear"][far]), _bits(clean["linear"][far]))
    assert np.array_equal(_bits(got["variance"][far]), _bits(clean["variance"][far]))
    assert not np.array_equal(_bits(got["linear"][9, 9]), _bits(clean["linear"][9, 9]))
    # the estimate beside it is the clean image's over 48 taps instead of 49
    l = sr.lum(c).astype(np.float64)
    win = l[6:13, 6:13].copy()                                     # around (9, 9); the NaN pixel is inside
    keep = np.ones((7, 7), bool)
    keep[0 + 3, 1 + 3] = False
    want = 4 * (np.mean(win[keep] ** 2) - np.mean(win[keep]) ** 2)
    assert abs(float(got["v0"][9, 9]) - want) < 1e-4 * want


def test_moments_are_ignored_below_length_4_and_used_from_4():
    c, n, z, a = _noisy(26)
    h, w = c.shape[:2]
    rng = np.random.default_rng(27)
    m = np.zeros_like(c)
    m[..., 0] = sr.lum(c)
    m[..., 1] = m[..., 0] * m[..., 0] + (rng.random((h, w)) * 0.1).astype(F)
    m[..., 2] = 123.0                                              # ignored
    g = dict(normal=n, sigma_normal=0.5, depth=z, sigma_depth=0.1, albedo=a)
    for N in (0, 1, 3):
        ln = np.full((h, w), N, np.uint32)
        with_m, without = sr.svgf(c, 3, 4.0, moments=m, length=ln, **g), sr.svgf(c, 3, 4.0, length=ln, **g)
        assert with_m["hits"] == 0
        for k in ("linear", "variance", "v0"):
            assert np.array_equal(_bits(with_m[k]), _bits(without[k])), (N, k)
    # the spatial estimate widens as the history shortens: 4 / min(max(N, 1), 4)
    v = {N: sr.svgf(c, 1, 4.0, length=np.full((h, w), N, np.uint32))["v0"] for N in (0, 1, 2, 3, 4, 9)}
    assert np.array_equal(_bits(v[0]), _bits(v[1])) and np.array_equal(_bits(v[4]), _bits(v[9]))
    assert np.array_equal(_bits(v[1]), _bits(v[4] * F(4))) and np.array_equal(_bits(v[2]), _bits(v[4] * F(2)))
    assert np.array_equal(_bits(sr.svgf(c, 1, 4.0)["v0"]), _bits(v[1]))          # no lengths: 1 everywhere
    for N in (4, 5, 65535, 0xFFFFFFFF):
        r = sr.svgf(c, 3, 4.0, moments=m, length=np.full((h, w), N, np.uint32), **g)
        assert r["hits"] == h * w
        assert np.array_equal(_bits(r["v0"]), _bits(np.fmax(m[..., 1] - m[..., 0] * m[..., 0], F(0))))
    # a mixed plane: each pixel by its own length; moments without lengths are never used
    ln = rng.integers(0, 8, (h, w)).astype(np.uint32)
    r = sr.svgf(c, 3, 4.0, moments=m, length=ln, **g)
    assert np.array_equal(r["temporal"], ln >= 4) and r["hits"] == int((ln >= 4).sum())
    assert sr.svgf(c, 3, 4.0, moments=m, **g)["hits"] == 0


def test_row_major_and_packed_are_one_filter():
    rng = np.random.default_rng(28)
    w, h = 13, 5
    c = rng.random((h, w, 3)).astype(F)
    z = (F(1.0) + rng.random((h, w)).astype(F) * F(0.1)).astype(F)
    a = rng.random((h, w, 3)).astype(F)
    _, m = sr.illumination(c)
    ln = rng.integers(0, 8, (h, w)).astype(np.uint32)
    pix = native.tile_pixels(w, h, 8)
    want = sr.svgf(c, 3, 2.0, moments=m, length=ln, depth=z, sigma_depth=0.3, albedo=a)
    got = sr.svgf_packed(pix, w, h, c.reshape(-1, 3)[pix], 3, 2.0, moments=m.reshape(-1, 3)[pix],
                         length=ln.reshape(-1)[pix], depth=z.reshape(-1)[pix], sigma_depth=0.3,
                         albedo=a.reshape(-1, 3)[pix])
    assert got["hits"] == want["hits"] > 0
    assert np.array_equal(_bits(got["linear"]), _bits(want["linear"].reshape(-1, 3)[pix]))
    assert np.array_equal(_bits(got["variance"]), _bits(want["variance"].reshape(-1)[pix]))
    same = sr.svgf_packed(None, w, h, c, 3, 2.0, moments=m, length=ln, depth=z, sigma_depth=0.3, albedo=a)
    assert np.array_equal(_bits(same["linear"]), _bits(want["linear"].reshape(-1, 3)))


# ----------------------------------------------------------- the quality condition
QUALITY = (33, 31, 4, 256, 6, 1000, 3)     # w, h, a frame's samples, the converged frame's, frames, seed stride, the move's frame
_FRAMES = {}


def frame_inputs(orc, name, k, moved):
    """(camera, the 4-sample frame (h, w, 3), guide planes) of frame k at the
    scene's camera, or at the moved one; computed once."""
    key = (name, k, moved)
    if key in _FRAMES:
        return _FRAMES[key]
    w, h, spp, _, _, stride, _ = QUALITY
    t = rc.tall_scene(orc, name)
    seed = t.seed + stride * k
    if moved:
        cam = rr.moved(camera_for(t.soup, None, w, h), *rh.MOVES[name]["both"])
        ocam = orc.camera_from_dict(dict(w=w, h=h, origin=cam.origin, llc=cam.llc, right=cam.right, up=cam.up))
    else:
        cam = rr.cam_of(camera_for(t.soup, None, w, h))
        ocam = t.ocam(w, h)
    lin = t.oracle.render(ocam, spp, rc.MB, orc.RNG_PATH, seed, rc.THREADS)[1].reshape(h, w, 3).copy()
    rec = feature_ref.PixelRecords(orc, t.ray_ref, t.soup, rh.to_native(cam), seed, np.arange(w * h), spp)
    pl = rec.planes(spp)
    out = (cam, lin, {"normal": pl["normal"].reshape(h, w, 3), "depth": pl["depth"].reshape(h, w),
                      "albedo": pl["base_color"].reshape(h, w, 3)})
    lin.setflags(write=False)
    _FRAMES[key] = out
    return out


@pytest.mark.parametrize("moved", (False, True), ids=("static", "moved"))
@pytest.mark.parametrize("name", rc.SCENES)
def test_the_filter_brings_every_frame_of_a_sequence_closer_to_the_converged_one(name, moved, oracle_mod):
    w, h, spp, many, frames, _, at = QUALITY
    mx, dt, nt = native.REPROJECT_DEFAULTS
    sl, sn, sz = native.SVGF_SIGMAS
    truth = {False: rh.frame_of(rh.scene_frames(oracle_mod, name, "identical"), many).reshape(h, w, 3).astype(np.float64)}
    if moved:
        truth[True] = rh.frame_of(rh.scene_frames(oracle_mod, name, "both"), many).reshape(h, w, 3).astype(np.float64)
    prev = None
    for k in range(frames):
        at_b = moved and k >= at
        cam, noisy, g = frame_inputs(oracle_mod, name, k, at_b)
        I, m = sr.illumination(noisy, g["albedo"])
        if prev is None:
            color, moments, length = I, m, np.ones((h, w), np.uint32)
        else:
            pcam, pg, pc, pm, pl = prev
            args = (g["depth"], pc, pg["depth"], g["normal"], pg["normal"], pl, mx, dt, nt)
            rc_, rm_ = rr.reproject(cam, pcam, I, *args), rr.reproject(cam, pcam, m, g["depth"], pm, *args[2:])
            color, moments, length = rc_["color"], rm_["color"], rm_["length"]
        prev = (cam, g, color, moments, length)
        dm = sr.dmod(g["albedo"])
        r = sr.svgf(color, 5, sl, moments=moments, length=length, normal=g["normal"], sigma_normal=sn,
                    depth=g["depth"], sigma_depth=sz, albedo=g["albedo"])
        today = dr.denoise(color * dm, 5, native.DENOISE_SIGMAS[0], g["normal"], native.DENOISE_SIGMAS[1], g["depth"],
                           native.DENOISE_SIGMAS[2], g["albedo"], native.DENOISE_SIGMAS[3])
        e_rep = float(np.abs(color * dm - truth[at_b]).mean())
        e_today = float(np.abs(today - truth[at_b]).mean())
        e_svgf = float(np.abs(r["linear"] - truth[at_b]).mean())
        share = r["hits"] / (w * h)
        print(f"{name} {'moved' if moved else 'static'} frame {k}: mean absolute error against {many} samples: "
              f"reprojected only {e_rep:.6f}, denoise_ref {e_today:.6f}, svgf_ref {e_svgf:.6f}; temporal variance at "
              f"{share:.3f} of the pixels")
        assert e_svgf < e_rep, k
        if not moved and k >= 3:
            assert share >= 0.5, k
