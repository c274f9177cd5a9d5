"""The denoiser on the GPU (zrt_context_denoise, Context.denoise), bit for bit:
`linear` as uint32 patterns and `rgb` against denoise_ref.py (the header's
contract in numpy float32) and the oracle's to_rgb.  Any small scene gives the
context; the planes are synthetic, from a seeded generator: ordinary values,
exact zeros, a depth-0 "sky" region, and a sprinkle of NaN and +-inf in every
plane, the colour included.

Shapes, the smallest at which the kernels can still go wrong:
  3 x 3, tile 8      at step 1 only the 3 x 3 centre of the 5 x 5 taps is
                     inside, from step 4 on the centre tap alone
  13 x 5, tile 8     partial tiles and partial 8 x 8 blocks
  33 x 31, tile 32   four tiles, three partial; 16 x 16 workgroups with ragged
                     edges; 5 levels (step 16 reaches across the frame) and 8
                     (step 128 leaves the centre tap alone)
  70 x 9, tile 64    and the same frame row-major
each with all three guides, each single guide and none, host and device
pointers, and linear only, rgb only and both.

The film source is compared with the colour source on the GPU (the film's
presented frame is the oracle's, test_film_gpu.py and test_refine_gpu.py), and
both with the reference.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native

import denoise_ref as dr
import refine_cases as rc
import test_denoise_host as dh

pytestmark = pytest.mark.gpu
F = np.float32
MB = rc.MB
SIGMAS = dict(sigma_color=0.75, sigma_normal=0.5, sigma_depth=0.25, sigma_albedo=0.5)
# (w, h, tile, row_major, iterations)
SHAPES = ((3, 3, 8, False, 5), (13, 5, 8, False, 5), (33, 31, 32, False, 5), (33, 31, 32, False, 8),
          (70, 9, 64, False, 5), (70, 9, 64, True, 5))
GUIDES = {"all": ("normal", "depth", "albedo"), "normal": ("normal",), "depth": ("depth",), "albedo": ("albedo",),
          "none": ()}
WIDTH = {"color": 3, "normal": 3, "depth": 1, "albedo": 3}


@pytest.fixture(scope="module")
def tall(oracle_mod):
    return lambda name: rc.tall_scene(oracle_mod, name)


def _scene(t):
    return RenderScene(t.soup, rc.RES, device=0, device_build=t.name == "fuzz")


@pytest.fixture(scope="module")
def context(tall):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _scene(tall(name))
        return made[name]
    yield get
    for rs in made.values():
        rs.close()


# ------------------------------------------------------------------ the planes
_PLANES = {}


def planes(w, h):
    """Row-major synthetic planes of a w x h frame, made once: {"color" (P, 3),
    "normal" (P, 3), "depth" (P,), "albedo" (P, 3)} float32 and the pixel sets
    the generator placed ("nan_color", "bad_normal": image indices)."""
    if (w, h) in _PLANES:
        return _PLANES[(w, h)]
    rng = np.random.default_rng(1000 * w + h)
    P = w * h
    y, x = np.divmod(np.arange(P), w)
    region = ((x * 3) // max(w, 1) + 3 * ((y * 2) // max(h, 1))).astype(np.int64)      # 3 x 2 flat regions
    base = rng.random((6, 3)).astype(F)
    color = (base[region] * F(1.5) + (rng.random((P, 3)).astype(F) - F(0.5)) * F(0.5)).astype(F)
    color = np.abs(color)
    color[rng.random(P) < 0.1] = 0.0                                # exact zeros
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], F)
    normal = (axes[region] + (rng.random((P, 3)).astype(F) - F(0.5)) * F(0.2)).astype(F)
    depth = (F(1.0) + region.astype(F) * F(0.5) + rng.random(P).astype(F) * F(0.1)).astype(F)
    albedo = (rng.random((6, 3)).astype(F)[region] + (rng.random((P, 3)).astype(F) - F(0.5)) * F(0.1)).astype(F)
    sky = y < max(1, h // 4)                                         # a miss: the features planes hold +0 there
    if P > 9:
        depth[sky], normal[sky], albedo[sky] = 0.0, 0.0, 0.0
    out = {"color": color, "normal": normal, "depth": depth, "albedo": albedo}
    # the sprinkle: distinct pixels, a NaN, a +inf and a -inf per plane (tiny frames: one of them per plane)
    spots = rng.permutation(P)
    bad = [np.nan, np.inf, -np.inf]
    per = 3 if P >= 64 else 1
    k = 0
    placed = {}
    for j, name in enumerate(("color", "normal", "depth", "albedo")):
        for i in range(per):
            p = int(spots[k % P])
            k += 1
            v = bad[(i + j) % 3] if per == 1 else bad[i]
            if out[name].ndim == 2:
                out[name][p, (i + j) % 3] = v
            else:
                out[name][p] = v
            placed.setdefault(name, []).append((p, v))
    out["nan_color"] = np.nonzero(np.isnan(color).any(axis=1))[0]
    out["bad_normal"] = np.array([p for p, _ in placed["normal"]])
    assert out["nan_color"].size >= (1 if per == 3 else 0)
    for a in out.values():
        a.setflags(write=False)
    _PLANES[(w, h)] = out
    return out


_WANT = {}


def want(orc, w, h, iterations, guides):
    """(linear (P, 3) float32, rgb (P, 3) uint8) of the reference in row-major
    order, once per (frame, iterations, guides)."""
    key = (w, h, iterations, guides)
    if key not in _WANT:
        pl = planes(w, h)
        kw = {}
        for g in guides:
            kw[g] = pl[g].reshape((h, w, 3) if WIDTH[g] == 3 else (h, w))
            kw["sigma_" + g] = SIGMAS["sigma_" + g]
        lin = dr.denoise(pl["color"].reshape(h, w, 3), iterations, SIGMAS["sigma_color"], **kw).reshape(-1, 3)
        rgb = np.stack([orc.to_rgb(v) for v in lin])
        lin.setflags(write=False)
        rgb.setflags(write=False)
        _WANT[key] = (lin, rgb)
    return _WANT[key]


def _bits(a):
    a = a.cpu().numpy() if not isinstance(a, np.ndarray) else a
    return np.ascontiguousarray(a, F).reshape(-1, 3).view(np.uint32)


def _u8(a):
    a = a.cpu().numpy() if not isinstance(a, np.ndarray) else a
    return np.ascontiguousarray(a).reshape(-1, 3)


def _diff(got, ref, what):
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} pixels differ, first at index {bad[0]}: got "
                           f"{[hex(int(v)) for v in got[bad[0]]]}, reference {[hex(int(v)) for v in ref[bad[0]]]}")


@pytest.mark.parametrize("guides", list(GUIDES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-t%d-%s-%d" % (s[0], s[1], s[2], "rm" if s[3] else "pk", s[4]))
def test_the_filter_is_the_references_bit_for_bit(shape, guides, oracle_mod, tall, context):
    w, h, tile, row_major, iterations = shape
    ctx = context("cornell").context
    pl = planes(w, h)
    lin, rgb = want(oracle_mod, w, h, iterations, GUIDES[guides])
    order = np.arange(w * h) if row_major else native.tile_pixels(w, h, tile)
    given = {k: np.ascontiguousarray(pl[k][order]) for k in ("color",) + GUIDES[guides]}
    # the reference itself: a NaN colour pixel keeps its bits (W == 0, every tap dropped), and so does a
    # pixel whose own normal is not finite wherever the normal guides
    keep = [pl["nan_color"]] + ([pl["bad_normal"]] if "normal" in GUIDES[guides] else [])
    for px in keep:
        assert np.array_equal(lin[px].view(np.uint32), pl["color"][px].view(np.uint32))
    if w * h >= 64:
        assert pl["nan_color"].size >= 1
        assert (lin.view(np.uint32) != pl["color"].view(np.uint32)).any(axis=1).sum() > w * h // 2   # it filtered
    assert torch is not None, "the device-pointer half needs torch"
    for device in (False, True):
        src = {k: torch.from_numpy(v).cuda() for k, v in given.items()} if device else given
        for ask in ((True, False), (False, True), (True, True)):
            what = (shape, guides, "device" if device else "host", ask)
            res = ctx.denoise(w, h, iterations=iterations, tile=tile, row_major=row_major, linear=ask[0], rgb=ask[1],
                              **src, **SIGMAS)
            assert ("linear" in res, "rgb" in res) == ask, what
            if ask[0]:
                _diff(_bits(res["linear"]), lin.view(np.uint32)[order], what + ("linear",))
            if ask[1]:
                _diff(_u8(res["rgb"]), rgb[order], what + ("rgb",))
            if not device:                                           # the same planes as images: row-major
                assert sorted(res["images"]) == sorted(k for k in ("linear", "rgb") if k in res), what
                for k, img in res["images"].items():
                    assert img.shape == (h, w, 3), what
                    _diff(_bits(img) if k == "linear" else _u8(img), lin.view(np.uint32) if k == "linear" else rgb,
                          what + ("image", k))
            st = res["stats"]
            assert st["samples"] == w * h and st["trace_launches"] == iterations + 2, what


# ------------------------------------------------------------------ guard rows
SENT32, SENT8 = 0xABABABAB, 0xAB


def _raw_call(ctx, w, h, tile, src, lin_ptr, rgb_ptr, on_device, iterations=5, **kw):
    ptr = {k: (v.data_ptr() if on_device else v.ctypes.data) for k, v in src.items()}
    return ctx.denoise_raw(w, h, ptr.get("color"), kw.pop("film", None), ptr.get("normal"), ptr.get("depth"),
                           ptr.get("albedo"), lin_ptr, rgb_ptr, on_device, iterations, SIGMAS["sigma_color"],
                           SIGMAS["sigma_normal"], SIGMAS["sigma_depth"], SIGMAS["sigma_albedo"], tile_size=tile, **kw)


@pytest.mark.parametrize("ask", ((True, False), (False, True), (True, True)), ids=("linear", "rgb", "both"))
def test_guard_rows_and_unasked_outputs_stay_untouched(ask, oracle_mod, context):
    assert torch is not None, "device buffers need torch"
    w, h, tile = 33, 31, 32
    P = w * h
    ctx = context("cornell").context
    pl = planes(w, h)
    order = native.tile_pixels(w, h, tile)
    src = {k: torch.from_numpy(np.ascontiguousarray(pl[k][order])).cuda() for k in ("color",) + GUIDES["all"]}
    lin, rgb = want(oracle_mod, w, h, 5, GUIDES["all"])
    guard = 64
    d_lin = torch.full((3 * (P + 2 * guard),), SENT32 - (1 << 32), dtype=torch.int32, device="cuda")
    d_rgb = torch.full((3 * (P + 2 * guard),), SENT8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _raw_call(ctx, w, h, tile, src, d_lin.data_ptr() + 12 * guard if ask[0] else None,
              d_rgb.data_ptr() + 3 * guard if ask[1] else None, True)
    got_lin = d_lin.cpu().numpy().view(np.uint32).reshape(-1, 3)
    got_rgb = d_rgb.cpu().numpy().reshape(-1, 3)
    for got, ref, sent, asked in ((got_lin, lin.view(np.uint32)[order], SENT32, ask[0]), (got_rgb, rgb[order], SENT8, ask[1])):
        assert (got[:guard] == sent).all() and (got[guard + P:] == sent).all()
        if asked:
            _diff(got[guard:guard + P], ref, ("guarded", ask))
        else:
            assert (got == sent).all()
    for k, v in src.items():                                         # the inputs are read, never written
        assert np.array_equal(v.cpu().numpy().view(np.uint32), np.ascontiguousarray(pl[k][order]).view(np.uint32)), k


# ------------------------------------------------------------------ film source
def _guides_of(ctx, cam, spp, seed):
    f = ctx.features(cam, spp, seed=seed, planes=("base_color", "normal", "depth"))
    return dict(normal=f["normal"], depth=f["depth"], albedo=f["base_color"])


def _film_equals_color(ctx, film, w, h, shown, guides, what):
    """denoise(film) == denoise(color = the frame the film's last call showed),
    both == the reference; the film is read, never written."""
    before = film.read()
    counts = film.counts()
    a = ctx.denoise(w, h, film=film, rgb=True, **guides)
    b = ctx.denoise(w, h, color=shown, rgb=True, **guides)
    c = film.denoise(rgb=True, **guides)
    for k in ("linear", "rgb"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)
        assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), (what, k)
    pix = native.tile_pixels(w, h)
    sc, sn, sz, sa = native.DENOISE_SIGMAS
    ref = dr.denoise_packed(pix, w, h, shown, 5, sc, guides["normal"], sn, guides["depth"], sz, guides["albedo"], sa)
    _diff(_bits(a["linear"]), ref.view(np.uint32), what)
    after = film.read()
    assert after[1] == before[1] and np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32)), what
    assert np.array_equal(film.counts()[0], counts[0]) and film.counts()[1] == counts[1], what
    return a


@pytest.mark.parametrize("name", rc.SCENES)
def test_a_films_frame_is_its_colour_plane(name, tall, context):
    t, rs = tall(name), context(name)
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    film = rs.context.film(w, h)
    res = rs.context.accumulate(film, cam, 4, MB, seed=t.seed, linear=True)
    assert np.array_equal(res["linear"].view(np.uint32), t.frame(w, h, 4, MB)[1][native.tile_pixels(w, h)])
    guides = _guides_of(rs.context, cam, 4, t.seed)
    a = _film_equals_color(rs.context, film, w, h, res["linear"], guides, (name, "accumulate"))
    assert (a["linear"].view(np.uint32) != res["linear"].view(np.uint32)).any()
    film.close()


@pytest.mark.parametrize("case", [k for k in rc.PARITY if k[3] == rc.SCHEDULE and k[5] == 0 and k[4] == 0.125 and
                                  k[1:3] in ((13, 5), (33, 31))], ids=lambda k: "%s-%dx%d" % k[:3])
def test_a_refined_films_frame_uses_every_pixels_own_count(case, tall, context):
    name, w, h, schedule, thr, min_s = case
    t, rs = tall(name), context(name)
    cam = camera_for(t.soup, None, w, h)
    film = rs.context.film(w, h)
    guides = _guides_of(rs.context, cam, 4, t.seed)
    frozen = False
    for j, n in enumerate(schedule[:4]):
        res = rs.context.refine(film, cam, n, MB, thr, min_s, seed=t.seed, linear=True, counts=True)
        assert res["active"] == rc.PARITY[case][j]
        if 0 < res["active"] < w * h:                              # per-pixel counts are in play
            assert len(np.unique(res["counts"])) > 1
            frozen = True
            _film_equals_color(rs.context, film, w, h, res["linear"], guides, (case, j))
    assert frozen
    film.reset()                                                   # stale flags: every pixel at the film's samples again
    res = rs.context.accumulate(film, cam, 4, MB, seed=t.seed, linear=True)
    _film_equals_color(rs.context, film, w, h, res["linear"], guides, (case, "after reset"))
    film.close()


def test_film_refusals_with_their_control(tall, context):
    t, rs = tall("cornell"), context("cornell")
    ctx = rs.context
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    film = ctx.film(w, h)
    lin = np.full((w * h, 3), 0xA0A0A0A0, np.uint32)
    col = np.zeros((w * h, 3), F)

    def call(w_=w, h_=h, tile=64, f=film, color=None, flags=0, on=ctx):
        return on.denoise_raw(w_, h_, color, f, None, None, None, lin.ctypes.data, None, False, 5, 1.0,
                              tile_size=tile, flags=flags)

    def refused(**kw):
        with pytest.raises(native.ZrtError) as e:
            call(**kw)
        assert e.value.status == -1, kw
        assert (lin == 0xA0A0A0A0).all(), kw

    refused()                                                      # an empty film
    ctx.accumulate(film, cam, 4, MB, seed=t.seed)
    refused(w_=h, h_=w)                                            # another frame
    refused(tile=32)                                               # another tile
    refused(color=col.ctypes.data)                                 # both sources
    refused(flags=native.DENOISE_ROW_MAJOR)                        # a film is never row-major
    other = _scene(t)
    refused(on=other.context)                                      # another context's film
    other.close()
    part = ctx.film(w, h, 8, 1, 2)                                 # rank 1 of 2
    ctx.accumulate(part, cam, 4, MB, seed=t.seed)
    refused(f=part, tile=8)
    part.close()
    assert call()["samples"] == w * h                              # the control
    assert (lin != 0xA0A0A0A0).all()
    film.close()


# ------------------------------------------------------------------ alternation, stats, refusals
def test_denoise_alternates_with_renders_and_features(tall, oracle_mod):
    t = tall("cornell")
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    pl = planes(w, h)
    order = native.tile_pixels(w, h)
    src = {k: np.ascontiguousarray(pl[k][order]) for k in ("color",) + GUIDES["all"]}

    def render(rs, spp):
        r = rs.context.render(cam, spp, MB, seed=t.seed, packed=True, linear=True)
        return r["packed"], r["linear"].view(np.uint32), {k: r["stats"][k] for k in ("segments", "samples")}, \
            rs.context.profile()

    def denoise(rs, it):
        r = rs.context.denoise(w, h, iterations=it, rgb=True, **src, **SIGMAS)
        return r["linear"].view(np.uint32), r["rgb"]

    def features(rs):
        f = rs.context.features(cam, 3, seed=t.seed)
        return [f[n].view(np.uint32) for n, _ in native.FEATURE_PLANES]

    steps = ((render, 5), (denoise, 5), (features,), (denoise, 2), (render, 7))
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
    assert rs.context.profile() == fresh[-1][3]                    # the last render's, untouched by the denoiser
    rs.close()
    lin, rgb = want(oracle_mod, w, h, 5, GUIDES["all"])
    assert np.array_equal(fresh[1][0], lin.view(np.uint32)[order]) and np.array_equal(fresh[1][1], rgb[order])


@pytest.mark.parametrize("iterations", (1, 5, 8))
def test_stats(iterations, context):
    ctx = context("cornell").context
    w, h = 33, 31
    pl = planes(w, h)
    order = native.tile_pixels(w, h, 32)
    src = {k: np.ascontiguousarray(pl[k][order]) for k in ("color",) + GUIDES["all"]}
    zero = dict(segments=0, cells_visited=0, triangle_tests=0, hits=0)
    st = ctx.denoise(w, h, iterations=iterations, tile=32, **src, **SIGMAS)["stats"]
    assert {k: st[k] for k in zero} == zero and st["samples"] == w * h
    assert st["trace_launches"] == iterations + 2                  # gather + one per level + present
    assert 0 < st["trace_kernel_ms"] <= st["render_ms"]            # a host call: the copies are not kernel time
    if torch is not None:
        dev = {k: torch.from_numpy(v).cuda() for k, v in src.items()}
        sd = ctx.denoise(w, h, iterations=iterations, tile=32, **dev, **SIGMAS)["stats"]
        assert {k: sd[k] for k in zero} == zero and sd["samples"] == w * h
        assert sd["trace_launches"] == iterations + 2 and 0 < sd["trace_kernel_ms"] == sd["render_ms"]


def test_refusals_with_their_control(context):
    """test_denoise_host.py's refusals on a real context: each is refused for
    its own reason, the outputs untouched -- the same batch, made valid,
    succeeds, and so does what the header allows."""
    ctx = context("cornell").context
    L = native.lib()
    x = [np.full(192, 0.5, F), np.zeros(192, F), np.ones(64, F), np.full(192, 0.25, F)]
    outs = [np.full(192, 0xA0A0A0A0, np.uint32), np.full(192, 0xB1, np.uint8)]
    st = native.Stats()
    for name, change in dh.REFUSALS.items():
        batch = native.DenoiseBatch(**{**dh._valid(x, outs), **change})
        assert L.zrt_context_denoise(ctx._h, C.byref(batch), C.byref(st)) == -1, name
        assert (outs[0] == 0xA0A0A0A0).all() and (outs[1] == 0xB1).all(), name
    for name, change in [("valid", {})] + [(k, v) for k, v in dh.ALLOWED.items() if k != "P = 2^31"]:
        outs[0][:], outs[1][:] = 0xA0A0A0A0, 0xB1
        batch = native.DenoiseBatch(**{**dh._valid(x, outs), **change})
        assert L.zrt_context_denoise(ctx._h, C.byref(batch), C.byref(st)) == 0, name
        assert st.samples == 64 and st.trace_launches == batch.iterations + 2, name
        if batch.linear:
            assert (outs[0] != 0xA0A0A0A0).all(), name
        if batch.rgb:
            assert (outs[1] != 0xB1).any(), name
