"""Illumination, moments and the variance-guided filter on the GPU
(zrt_context_illumination, zrt_context_svgf, SvgfHistory), bit for bit:
`linear`, `variance`, `illumination`, `moments` as uint32 patterns, `rgb` and
stats.hits against svgf_ref.py (the header's contract in numpy float32) and the
oracle's to_rgb.  Any small scene gives the context; the planes are
test_denoise_gpu.py's synthetic ones (ordinary values, exact zeros, a depth-0
"sky" region, a NaN, +inf and -inf in every plane) with a moments plane made
the same way and lengths drawn from 0, 1, 3, 4, 65535 and 0xFFFFFFFF.

Shapes, the smallest at which the kernels can still go wrong:
  1 x 1             every tap but the centre outside; one workgroup, one thread live
  3 x 3, tile 8     at step 1 only the 3 x 3 centre of the 5 x 5 taps is
                    inside; the 7 x 7 estimate sees the whole frame
  13 x 5, tile 8    partial tiles and partial 8 x 8 blocks
  33 x 31, tile 32  four tiles, three partial; 3 x 2 workgroups of 16 x 16 with
                    ragged edges, so the LDS halos cross workgroups; 5 levels
                    (steps 1, 2: tiled kernels; 4, 8, 16: plain) and 8
  70 x 9, tile 64   five workgroups in a row, a partial last
each packed and row-major, with both guides, each single guide and none, with
and without moments, lengths and albedo, host and device pointers.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import camera_for, native

import refine_cases as rc
import svgf_ref as sr
import test_svgf_host as sh
from test_denoise_gpu import _scene, context, planes, tall  # noqa: F401  (fixtures and the synthetic planes)

pytestmark = pytest.mark.gpu
F = np.float32
MB = rc.MB
SIGMAS = dict(sigma_luminance=2.0, sigma_normal=0.5, sigma_depth=0.25)
# (w, h, tile, iterations), each packed and row-major
FRAMES = ((1, 1, 8, 5), (3, 3, 8, 5), (13, 5, 8, 5), (33, 31, 32, 5), (33, 31, 32, 8), (70, 9, 64, 5))
SHAPES = tuple(f + (rm,) for f in FRAMES for rm in (False, True))
GUIDES = {"both": ("normal", "depth"), "normal": ("normal",), "depth": ("depth",), "none": ()}
# (moments, length, albedo) given
OPTIONS = ((True, True, True), (False, False, False), (True, False, False), (False, True, True))
LENGTHS = np.array([0, 1, 3, 4, 65535, 0xFFFFFFFF], np.uint32)
WIDTH = {"color": 3, "moments": 3, "length": 1, "normal": 3, "depth": 1, "albedo": 3}

_MORE = {}


def more(w, h):
    """{"moments" (P, 3) float32, "length" (P,) uint32} for planes(w, h), row-major, made once."""
    if (w, h) in _MORE:
        return _MORE[(w, h)]
    pl = planes(w, h)
    rng = np.random.default_rng(7000 * w + h)
    P = w * h
    with np.errstate(all="ignore"):
        l = np.nan_to_num(sr.lum(pl["color"]), nan=0.5, posinf=1.0, neginf=0.25).astype(F)
    m = np.zeros((P, 3), F)
    m[:, 0] = l * (F(0.75) + rng.random(P).astype(F) * F(0.5))
    spread = (rng.random(P).astype(F) - F(0.25)) * F(0.2)           # a quarter below the square: clamped to 0
    second = m[:, 0] * m[:, 0] + spread
    m[:, 1] = np.where(second > 0, second, F(0.0))                  # (no -0: the sign of that zero v_0 is unspecified)
    m[:, 2] = rng.random(P).astype(F)                               # ignored
    m[rng.random(P) < 0.1, :2] = 0.0                                # exact zeros
    spots = rng.permutation(P)
    for i, v in enumerate((np.nan, np.inf, -np.inf)[:3 if P >= 64 else 1]):
        m[int(spots[i % P]), i % 2] = v
    length = LENGTHS[rng.integers(0, len(LENGTHS), P)]
    if P >= 64:
        length[:6] = LENGTHS                                # every value is there
    out = {"moments": m, "length": length}
    for a in out.values():
        a.setflags(write=False)
    _MORE[(w, h)] = out
    return out


def source(w, h):
    return {**{k: planes(w, h)[k] for k in ("color", "normal", "depth", "albedo")}, **more(w, h)}


_WANT = {}


def want(orc, w, h, iterations, guides, options):
    """The reference's row-major {"linear" (P, 3), "variance" (P,), "rgb" (P, 3) uint8, "hits"}, once per case."""
    key = (w, h, iterations, guides, options)
    if key not in _WANT:
        src = source(w, h)
        kw = {}
        for g in guides:
            kw[g] = src[g].reshape((h, w, 3) if WIDTH[g] == 3 else (h, w))
            kw["sigma_" + g] = SIGMAS["sigma_" + g]
        mom, ln, alb = options
        r = sr.svgf(src["color"].reshape(h, w, 3), iterations, SIGMAS["sigma_luminance"],
                    moments=src["moments"].reshape(h, w, 3) if mom else None,
                    length=src["length"].reshape(h, w) if ln else None,
                    albedo=src["albedo"].reshape(h, w, 3) if alb else None, **kw)
        lin = r["linear"].reshape(-1, 3)
        out = {"linear": lin, "variance": r["variance"].reshape(-1), "rgb": np.stack([orc.to_rgb(v) for v in lin]),
               "hits": r["hits"]}
        _WANT[key] = out
    return _WANT[key]


def _np(a):
    return a.cpu().numpy() if not isinstance(a, np.ndarray) else a


def _bits(a, ch=3):
    return np.ascontiguousarray(_np(a)).reshape(-1, ch).view(np.uint32)


def _diff(got, ref, what):
    got, ref = got.reshape(len(got), -1), ref.reshape(len(ref), -1)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} pixels differ, first at index {bad[0]}: got "
                           f"{[hex(int(v)) for v in got[bad[0]]]}, reference {[hex(int(v)) for v in ref[bad[0]]]}")


def given_planes(w, h, order, guides, options, device):
    src = source(w, h)
    mom, ln, alb = options
    names = ("color",) + guides + (("moments",) if mom else ()) + (("length",) if ln else ()) + \
        (("albedo",) if alb else ())
    out = {k: np.ascontiguousarray(src[k][order]) for k in names}
    if device:
        out = {k: torch.from_numpy(v.view(np.int32) if k == "length" else v).cuda() for k, v in out.items()}
    return out


@pytest.mark.parametrize("guides", list(GUIDES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-t%d-%d-%s" % (s[0], s[1], s[2], s[3], "rm" if s[4] else "pk"))
def test_the_filter_is_the_references_bit_for_bit(shape, guides, oracle_mod, context):
    w, h, tile, iterations, row_major = shape
    P = w * h
    ctx = context("cornell").context
    order = np.arange(P) if row_major else native.tile_pixels(w, h, tile)
    assert torch is not None, "the device-pointer half needs torch"
    for options in OPTIONS:
        ref = want(oracle_mod, w, h, iterations, GUIDES[guides], options)
        if P >= 64 and options[0] and options[1]:
            assert 0 < ref["hits"] < P                               # both variance branches in one frame
        if not (options[0] and options[1]):
            assert ref["hits"] == 0
        for device in (False, True):
            what = (shape, guides, options, "device" if device else "host")
            src = given_planes(w, h, order, GUIDES[guides], options, device)
            res = ctx.svgf(w, h, iterations=iterations, tile=tile, row_major=row_major, rgb=True, variance=True,
                           **src, **SIGMAS)
            _diff(_bits(res["variance"], 1), ref["variance"].view(np.uint32)[order], what + ("variance",))
            _diff(_bits(res["linear"]), ref["linear"].view(np.uint32)[order], what + ("linear",))
            _diff(_np(res["rgb"]).reshape(-1, 3), ref["rgb"][order], what + ("rgb",))
            st = res["stats"]
            assert st["hits"] == ref["hits"], what
            assert st["samples"] == P and st["trace_launches"] == iterations + 3, what
            if not device:                                           # the same planes as images: row-major
                assert sorted(res["images"]) == ["linear", "rgb", "variance"], what
                _diff(_bits(res["images"]["linear"]), ref["linear"].view(np.uint32), what + ("image",))
                _diff(_bits(res["images"]["variance"], 1), ref["variance"].view(np.uint32).reshape(-1, 1), what)
                assert res["images"]["rgb"].shape == (h, w, 3) and res["images"]["variance"].shape == (h, w)


@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: "%dx%d-t%d-%d-%s" % (s[0], s[1], s[2], s[3], "rm" if s[4] else "pk"))
def test_illumination_is_the_references_bit_for_bit(shape, context):
    w, h, tile, _, row_major = shape
    P = w * h
    ctx = context("cornell").context
    order = np.arange(P) if row_major else native.tile_pixels(w, h, tile)
    src = source(w, h)
    for alb in (True, False):
        I, m = sr.illumination(src["color"], src["albedo"] if alb else None)
        if not alb:
            assert np.array_equal(I.view(np.uint32), src["color"].view(np.uint32))
        for device in (False, True):
            given = {"color": np.ascontiguousarray(src["color"][order])}
            if alb:
                given["albedo"] = np.ascontiguousarray(src["albedo"][order])
            if device:
                given = {k: torch.from_numpy(v).cuda() for k, v in given.items()}
            for ask in ((True, True), (True, False), (False, True)):
                what = (shape, alb, device, ask)
                res = ctx.illumination(w, h, tile=tile, row_major=row_major, illumination=ask[0], moments=ask[1], **given)
                assert ("illumination" in res, "moments" in res) == ask, what
                if ask[0]:
                    _diff(_bits(res["illumination"]), I.view(np.uint32)[order], what + ("illumination",))
                if ask[1]:
                    _diff(_bits(res["moments"]), m.view(np.uint32)[order], what + ("moments",))
                st = res["stats"]
                assert st["samples"] == P and st["trace_launches"] == 1 and st["hits"] == 0, what


# ------------------------------------------------------------------ guard rows
SENT32, SENT8 = 0xABABABAB, 0xAB


@pytest.mark.parametrize("ask", ((True, False, False), (False, True, True), (True, True, True)),
                         ids=("linear", "rgb+variance", "all"))
def test_guard_rows_and_unasked_outputs_stay_untouched(ask, oracle_mod, context):
    assert torch is not None, "device buffers need torch"
    w, h, tile = 33, 31, 32
    P = w * h
    ctx = context("cornell").context
    order = native.tile_pixels(w, h, tile)
    options = (True, True, True)
    src = given_planes(w, h, order, GUIDES["both"], options, True)
    ref = want(oracle_mod, w, h, 5, GUIDES["both"], options)
    guard = 64
    d_lin = torch.full((3 * (P + 2 * guard),), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
    d_rgb = torch.full((3 * (P + 2 * guard),), SENT8, dtype=torch.uint8, device="cuda")
    d_var = torch.full((P + 2 * guard,), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
    d_il = torch.full((3 * (P + 2 * guard),), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
    d_mo = torch.full((3 * (P + 2 * guard),), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = {k: v.data_ptr() for k, v in src.items()}
    ctx.svgf_raw(w, h, ptr["color"], ptr["moments"], ptr["length"], ptr["normal"], ptr["depth"], ptr["albedo"],
                 d_lin.data_ptr() + 12 * guard if ask[0] else None, d_rgb.data_ptr() + 3 * guard if ask[1] else None,
                 d_var.data_ptr() + 4 * guard if ask[2] else None, True, 5, tile_size=tile, **SIGMAS)
    ctx.illumination_raw(w, h, ptr["color"], None, ptr["albedo"], d_il.data_ptr() + 12 * guard if ask[0] else None,
                         d_mo.data_ptr() + 12 * guard if ask[1] else None, True, tile_size=tile)
    I, m = sr.illumination(source(w, h)["color"], source(w, h)["albedo"])
    rows = ((d_lin, 3, ref["linear"].view(np.uint32)[order], SENT32, ask[0]),
            (d_rgb, 3, ref["rgb"][order], SENT8, ask[1]),
            (d_var, 1, ref["variance"].view(np.uint32)[order].reshape(-1, 1), SENT32, ask[2]),
            (d_il, 3, I.view(np.uint32)[order], SENT32, ask[0]), (d_mo, 3, m.view(np.uint32)[order], SENT32, ask[1]))
    for j, (buf, ch, want_, sent, asked) in enumerate(rows):
        got = buf.cpu().numpy()
        got = (got.view(np.uint32) if got.dtype == np.int32 else got).reshape(-1, ch)
        assert (got[:guard] == sent).all() and (got[guard + P:] == sent).all(), j
        if asked:
            _diff(got[guard:guard + P], want_, ("guarded", ask, j))
        else:
            assert (got == sent).all(), j
    for k, v in src.items():                                         # the inputs are read, never written
        assert np.array_equal(v.cpu().numpy().view(np.uint32), np.ascontiguousarray(source(w, h)[k][order]).view(np.uint32)), k


# ------------------------------------------------------------------ film source
def _film_equals_color(ctx, film, w, h, shown, albedo, what):
    """illumination(film) == illumination(color = the frame the film's last
    call showed), both == the reference; the film is read, never written."""
    before = film.read()
    counts = film.counts()
    a = ctx.illumination(w, h, film=film, albedo=albedo)
    b = ctx.illumination(w, h, color=shown, albedo=albedo)
    c = film.illumination(albedo)
    d = film.illumination()                                          # no albedo: the film's frame itself
    I, m = sr.illumination(shown, albedo)
    for k, ref in (("illumination", I), ("moments", m)):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
        assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), (what, k)
        _diff(_bits(a[k]), ref.view(np.uint32), what + (k,))
    assert np.array_equal(d["illumination"].view(np.uint32), shown.view(np.uint32)), what
    after = film.read()
    assert after[1] == before[1] and np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32)), what
    assert np.array_equal(film.counts()[0], counts[0]) and film.counts()[1] == counts[1], what


@pytest.mark.parametrize("case", [k for k in rc.PARITY if k[3] == rc.SCHEDULE and k[5] == 0 and k[4] == 0.125 and
                                  k[1:3] == (13, 5)], ids=lambda k: "%s-%dx%d" % k[:3])
def test_a_films_illumination_is_its_presented_colours(case, tall, context):
    name, w, h, schedule, thr, min_s = case
    t, rs = tall(name), context(name)
    ctx = rs.context
    cam = camera_for(t.soup, None, w, h)
    albedo = ctx.features(cam, 4, seed=t.seed, planes=("base_color",))["base_color"]
    film = ctx.film(w, h)
    res = ctx.accumulate(film, cam, 4, MB, seed=t.seed, linear=True)
    _film_equals_color(ctx, film, w, h, res["linear"], albedo, (case, "accumulate"))
    film.reset()
    frozen = False
    for j, n in enumerate(schedule[:4]):
        res = ctx.refine(film, cam, n, MB, thr, min_s, seed=t.seed, linear=True, counts=True)
        assert res["active"] == rc.PARITY[case][j]
        if 0 < res["active"] < w * h:                              # per-pixel counts are in play
            frozen = True
            _film_equals_color(ctx, film, w, h, res["linear"], albedo, (case, j))
    assert frozen
    film.close()


def test_film_refusals_with_their_control(tall, context):
    t, rs = tall("cornell"), context("cornell")
    ctx = rs.context
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    film = ctx.film(w, h)
    out = np.full((w * h, 3), 0xA0A0A0A0, np.uint32)
    col = np.zeros((w * h, 3), F)

    def call(w_=w, h_=h, tile=64, f=film, color=None, flags=0, on=ctx):
        return on.illumination_raw(w_, h_, color, f, None, out.ctypes.data, None, False, tile_size=tile, flags=flags)

    def refused(**kw):
        with pytest.raises(native.ZrtError) as e:
            call(**kw)
        assert e.value.status == -1, kw
        assert (out == 0xA0A0A0A0).all(), kw

    refused()                                                      # an empty film
    ctx.accumulate(film, cam, 4, MB, seed=t.seed)
    refused(w_=h, h_=w)                                            # another frame
    refused(tile=32)                                               # another tile
    refused(color=col.ctypes.data)                                 # both sources
    refused(flags=native.SVGF_ROW_MAJOR)                           # a film is never row-major
    other = _scene(t)
    refused(on=other.context)                                      # another context's film
    other.close()
    part = ctx.film(w, h, 8, 1, 2)                                 # rank 1 of 2
    ctx.accumulate(part, cam, 4, MB, seed=t.seed)
    refused(f=part, tile=8)
    part.close()
    assert call()["samples"] == w * h                              # the control
    assert (out != 0xA0A0A0A0).any()
    film.close()


# ------------------------------------------------------------------ the history
@pytest.mark.parametrize("name", rc.SCENES)
def test_the_history_is_the_calls_made_by_hand(name, tall, context):
    """Three frames under a static camera: SvgfHistory.update's planes and the
    filter over them against features, illumination, two reprojections and the
    filter called one by one on host arrays.  Lengths: 1, then 2, then 3
    wherever the history holds, 1 elsewhere."""
    assert torch is not None, "SvgfHistory keeps torch tensors"
    t, rs = tall(name), context(name)
    ctx = rs.context
    w, h = 33, 31
    P = w * h
    cam = camera_for(t.soup, None, w, h)
    film = ctx.film(w, h)
    hist = native.SvgfHistory(ctx, w, h)
    prev = None
    for k in range(3):
        seed = t.seed + 1000 * k
        film.reset()
        ctx.accumulate(film, cam, 4, MB, seed=seed)
        got = hist.update(film, cam, seed=seed, num_samples=4)
        assert sorted(got) == ["albedo", "color", "depth", "length", "moments", "normal"]
        filtered = ctx.svgf(w, h, tile=hist.tile, variance=True, **got)
        f = ctx.features(cam, 4, seed=seed, planes=("base_color", "normal", "depth"))
        il = ctx.illumination(w, h, film=film, albedo=f["base_color"])
        if prev is None:
            color, moments, length = il["illumination"], il["moments"], np.ones(P, np.uint32)
        else:
            pf, pc, pm, pl = prev
            kw = dict(depth=f["depth"], normal=f["normal"], prev_depth=pf["depth"], prev_normal=pf["normal"], prev_length=pl)
            rcol = ctx.reproject(cam, cam, color=il["illumination"], prev_color=pc, **kw)
            rmom = ctx.reproject(cam, cam, color=il["moments"], prev_color=pm, **kw)
            color, moments, length = rcol["color"], rmom["color"], rmom["length"]
            assert hist.stats[0]["hits"] == rcol["stats"]["hits"] and hist.stats[1]["hits"] == rmom["stats"]["hits"]
        prev = (f, color, moments, length)
        what = (name, k)
        _diff(_bits(got["color"]), color.view(np.uint32), what + ("color",))
        _diff(_bits(got["moments"]), moments.view(np.uint32), what + ("moments",))
        assert np.array_equal(got["length"].cpu().numpy().view(np.uint32), length), what
        assert set(np.unique(length)) <= set(range(1, k + 2)) and (length == k + 1).mean() > 0.5, what
        for key, a in (("albedo", f["base_color"]), ("normal", f["normal"]), ("depth", f["depth"])):
            assert np.array_equal(got[key].cpu().numpy().view(np.uint32).reshape(-1), a.view(np.uint32).reshape(-1)), what
        by_hand = ctx.svgf(w, h, color=color, moments=moments, length=length, normal=f["normal"], depth=f["depth"],
                           albedo=f["base_color"], variance=True)
        _diff(_bits(filtered["linear"]), by_hand["linear"].view(np.uint32), what + ("linear",))
        _diff(_bits(filtered["variance"], 1), by_hand["variance"].view(np.uint32).reshape(-1, 1), what + ("variance",))
        assert filtered["stats"]["hits"] == by_hand["stats"]["hits"] == 0          # lengths below 4 so far
        pix = native.tile_pixels(w, h)
        sl, sn, sz = native.SVGF_SIGMAS
        ref = sr.svgf_packed(pix, w, h, color, 5, sl, moments, length, f["normal"], sn, f["depth"], sz, f["base_color"])
        _diff(by_hand["linear"].view(np.uint32), ref["linear"].view(np.uint32), what + ("reference",))
    film.close()


# ------------------------------------------------------------------ alternation, stats, refusals
def test_svgf_alternates_with_renders_and_features(tall, oracle_mod):
    t = tall("cornell")
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    order = native.tile_pixels(w, h)
    options = (True, True, True)
    src = given_planes(w, h, order, GUIDES["both"], options, False)

    def render(rs, spp):
        r = rs.context.render(cam, spp, MB, seed=t.seed, packed=True, linear=True)
        return r["packed"], r["linear"].view(np.uint32), {k: r["stats"][k] for k in ("segments", "samples")}, \
            rs.context.profile()

    def svgf(rs, it):
        r = rs.context.svgf(w, h, iterations=it, rgb=True, variance=True, **src, **SIGMAS)
        return r["linear"].view(np.uint32), r["rgb"], r["variance"].view(np.uint32)

    def features(rs):
        f = rs.context.features(cam, 3, seed=t.seed)
        return [f[n].view(np.uint32) for n, _ in native.FEATURE_PLANES]

    def illumination(rs):
        r = rs.context.illumination(w, h, color=src["color"], albedo=src["albedo"])
        return r["illumination"].view(np.uint32), r["moments"].view(np.uint32)

    steps = ((render, 5), (svgf, 5), (features,), (illumination,), (svgf, 2), (render, 7))
    fresh = []
    for fn, *a in steps:                                           # each on a context of its own
        rs = _scene(t)
        fresh.append(fn(rs, *a))
        rs.close()
    rs = _scene(t)
    for j, (fn, *a) in enumerate(steps):
        got = fn(rs, *a)
        for g, f in zip(got, fresh[j]):
            assert np.array_equal(g, f) if isinstance(g, np.ndarray) else g == f, (j, fn.__name__)
    assert rs.context.profile() == fresh[-1][3]                    # the last render's, untouched by the filter
    rs.close()
    ref = want(oracle_mod, w, h, 5, GUIDES["both"], options)
    assert np.array_equal(fresh[1][0], ref["linear"].view(np.uint32)[order]) and np.array_equal(fresh[1][1], ref["rgb"][order])


@pytest.mark.parametrize("iterations", (1, 5, 8))
def test_stats(iterations, oracle_mod, context):
    ctx = context("cornell").context
    w, h = 33, 31
    order = native.tile_pixels(w, h, 32)
    options = (True, True, True)
    hits = want(oracle_mod, w, h, iterations, GUIDES["both"], options)["hits"]
    zero = dict(segments=0, cells_visited=0, triangle_tests=0)
    src = given_planes(w, h, order, GUIDES["both"], options, False)
    st = ctx.svgf(w, h, iterations=iterations, tile=32, **src, **SIGMAS)["stats"]
    assert {k: st[k] for k in zero} == zero and st["samples"] == w * h and st["hits"] == hits
    assert st["trace_launches"] == iterations + 3                  # gather + variance + one per level + present
    assert 0 < st["trace_kernel_ms"] <= st["render_ms"]            # a host call: the copies are not kernel time
    assert torch is not None
    dev = given_planes(w, h, order, GUIDES["both"], options, True)
    sd = ctx.svgf(w, h, iterations=iterations, tile=32, **dev, **SIGMAS)["stats"]
    assert {k: sd[k] for k in zero} == zero and sd["samples"] == w * h and sd["hits"] == hits
    assert sd["trace_launches"] == iterations + 3 and 0 < sd["trace_kernel_ms"] == sd["render_ms"]


def test_refusals_with_their_control(context):
    """test_svgf_host.py's refusals on a real context: each is refused for its
    own reason, the outputs untouched -- the same batch, made valid, succeeds,
    and so does what the header allows."""
    ctx = context("cornell").context
    L = native.lib()
    st = native.Stats()
    x, outs = sh.illumination_planes(), sh.illumination_outputs()
    for name, change in sh.ILLUMINATION_REFUSALS.items():
        batch = native.IlluminationBatch(**{**sh.illumination_valid(x, outs), **change})
        assert L.zrt_context_illumination(ctx._h, C.byref(batch), C.byref(st)) == -1, name
        assert (outs[0] == sh.GUARD).all() and (outs[1] == sh.GUARD + 1).all(), name
    for name, change in [("valid", {})] + [(k, v) for k, v in sh.ILLUMINATION_ALLOWED.items() if k != "P = 2^31"]:
        outs[0][:], outs[1][:] = sh.GUARD, sh.GUARD + 1
        batch = native.IlluminationBatch(**{**sh.illumination_valid(x, outs), **change})
        assert L.zrt_context_illumination(ctx._h, C.byref(batch), C.byref(st)) == 0, name
        assert st.samples == 64 and st.trace_launches == 1, name
        assert (outs[0] != sh.GUARD).all() == bool(batch.illumination), name
        assert (outs[1] != sh.GUARD + 1).all() == bool(batch.moments), name
    x, outs = sh.svgf_planes(), sh.svgf_outputs()
    for name, change in sh.SVGF_REFUSALS.items():
        batch = native.SvgfBatch(**{**sh.svgf_valid(x, outs), **change})
        assert L.zrt_context_svgf(ctx._h, C.byref(batch), C.byref(st)) == -1, name
        assert sh.svgf_untouched(outs), name
    for name, change in [("valid", {})] + [(k, v) for k, v in sh.SVGF_ALLOWED.items() if k != "P = 2^31"]:
        outs[0][:], outs[1][:], outs[2][:] = sh.GUARD, 0xB1, sh.GUARD + 2
        batch = native.SvgfBatch(**{**sh.svgf_valid(x, outs), **change})
        assert L.zrt_context_svgf(ctx._h, C.byref(batch), C.byref(st)) == 0, name
        assert st.samples == 64 and st.trace_launches == batch.iterations + 3, name
        assert st.hits == (64 if batch.moments and batch.length else 0), name
        assert (outs[0] != sh.GUARD).all() == bool(batch.linear), name
        assert (outs[1] != 0xB1).any() == bool(batch.rgb), name
        assert (outs[2] != sh.GUARD + 2).all() == bool(batch.variance), name


def test_denoise_and_reproject_refuse_the_new_flag_on_a_real_context(context):
    import test_denoise_host as dh
    import test_reproject_host as rh
    ctx = context("cornell").context
    L = native.lib()
    st = native.Stats()
    x = [np.full(192, 0.5, F), np.zeros(192, F), np.ones(64, F), np.full(192, 0.25, F)]
    outs = [np.full(192, 0xA0A0A0A0, np.uint32), np.full(192, 0xB1, np.uint8)]
    for flags in (native.SVGF_ROW_MAJOR, native.SVGF_ROW_MAJOR | native.DENOISE_ROW_MAJOR):
        batch = native.DenoiseBatch(**{**dh._valid(x, outs), "flags": flags})
        assert L.zrt_context_denoise(ctx._h, C.byref(batch), C.byref(st)) == -1
    assert (outs[0] == 0xA0A0A0A0).all() and (outs[1] == 0xB1).all()
    batch = native.DenoiseBatch(**dh._valid(x, outs))
    assert L.zrt_context_denoise(ctx._h, C.byref(batch), C.byref(st)) == 0            # the control
    x, outs = rh.host_planes(), rh.guarded_outputs()
    for flags in (native.SVGF_ROW_MAJOR, native.SVGF_ROW_MAJOR | native.REPROJECT_ROW_MAJOR):
        batch = native.ReprojectBatch(**{**rh._valid(x, outs), "flags": flags})
        assert L.zrt_context_reproject(ctx._h, C.byref(batch), C.byref(st)) == -1
    assert rh.untouched(outs)
    batch = native.ReprojectBatch(**rh._valid(x, outs))
    assert L.zrt_context_reproject(ctx._h, C.byref(batch), C.byref(st)) == 0          # the control
