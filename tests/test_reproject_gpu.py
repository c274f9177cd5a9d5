"""Reprojection on the GPU (zrt_context_reproject, Context.reproject,
native.History), bit for bit: `color_out` as uint32 patterns, `length_out`,
`motion` bits and stats.hits against reproject_ref.py (the header's contract in
numpy float32); no pixel is left out.  Any small scene gives the context; the
planes are synthetic, from a seeded generator.  The depths are those of the
world plane z = 0 under the two cameras (so taps land in the frame), times a
per-pixel factor within the tolerance, with a depth-0 sky band, a band whose
previous depth is 20 % off (a disocclusion), exact zeros in the colour, and a
sprinkle of NaN, +inf and -inf in every plane; prev_length holds 0, 1, 65535
and 0xFFFFFFFF among ordinary values.

Shapes, the smallest at which the kernels can still go wrong:
  1 x 1, tile 8      at most one tap inside
  3 x 3, tile 8      every pixel has taps outside
  13 x 5, tile 8     partial tiles and partial 8 x 8 blocks; 65 pixels: two waves
  33 x 31, tile 32   four tiles, three partial; several workgroups
  70 x 9, tile 64    and the same frame row-major
each under six camera pairs (identical, translated, yawed, turned away,
mirrored: D < 0, degenerate: D = 0), with and without the normal guide, with
and without prev_length, with and without motion, host and device pointers.
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
import reproject_ref as rr
import test_reproject_host as rh

pytestmark = pytest.mark.gpu
F = np.float32
MB = rc.MB
TOL = dict(max_history=32, depth_tolerance=0.05, normal_tolerance=0.5)
# (w, h, tile, row_major)
SHAPES = ((1, 1, 8, False), (3, 3, 8, False), (13, 5, 8, False), (33, 31, 32, False), (70, 9, 64, False),
          (70, 9, 64, True))


def _mirrored(c):
    """The same view with the columns reversed: right negated, the corner moved across (D < 0)."""
    return c._replace(llc=(c.llc + c.right * F(c.w)).astype(F), right=-c.right)


PAIRS = {
    "identical": lambda c: c,
    "translated": lambda c: rr.moved(c, (0.3, 0.1, 0.2)),
    "yawed": lambda c: rr.moved(c, yaw=0.05),
    "turned away": lambda c: rr.moved(c, yaw=np.pi),
    "mirrored": lambda c: _mirrored(rr.moved(c, (0.1, 0.0, 0.0))),
    "degenerate": lambda c: c._replace(right=np.zeros(3, F)),
}


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
def surface_depth(c):
    """The distance from the camera to the world plane z = 0 along each pixel
    centre's ray, (h, w) float32; 6 where the ray does not meet it."""
    ys, xs = np.mgrid[0:c.h, 0:c.w]
    v = c.llc.astype(np.float64) + c.right.astype(np.float64) * (xs + 0.5)[..., None] + \
        c.up.astype(np.float64) * (ys + 0.5)[..., None]
    with np.errstate(all="ignore"):
        d = v / np.linalg.norm(v, axis=-1)[..., None]
        t = -float(c.origin[2]) / d[..., 2]
    return np.where(np.isfinite(t) & (t > 0), t, 6.0).astype(F)


PLANE_NAMES = ("color", "depth", "normal", "prev_color", "prev_depth", "prev_normal", "prev_length")
_PLANES = {}


def planes(w, h, pair):
    """(current camera, previous camera, row-major synthetic planes of a w x h
    frame under them), made once and left unchanged."""
    key = (w, h, pair)
    if key in _PLANES:
        return _PLANES[key]
    rng = np.random.default_rng(100000 * w + 100 * h + list(PAIRS).index(pair))
    P = w * h
    cam = rh.pinhole(w, h)
    prev = PAIRS[pair](cam)
    y = np.arange(P) // w
    color = rng.random((P, 3)).astype(F) * F(2.0)
    color[rng.random(P) < 0.1] = 0.0                                # exact zeros
    prev_color = rng.random((P, 3)).astype(F) * F(2.0)
    depth = (surface_depth(cam).reshape(P) * (F(1.0) + (rng.random(P).astype(F) - F(0.5)) * F(0.02))).astype(F)
    prev_depth = (surface_depth(prev).reshape(P) * (F(1.0) + (rng.random(P).astype(F) - F(0.5)) * F(0.02))).astype(F)
    axis = np.array([0, 0, 1], F)
    normal = (axis + (rng.random((P, 3)).astype(F) - F(0.5)) * F(0.2)).astype(F)
    prev_normal = (axis + (rng.random((P, 3)).astype(F) - F(0.5)) * F(0.2)).astype(F)
    prev_length = rng.integers(1, 40, P).astype(np.uint32)
    if P > 9:
        depth[y < max(1, h // 4)] = 0.0                             # a miss: the features planes hold +0 there
        prev_depth[y < max(1, h // 5)] = 0.0
        prev_depth[y == h - 1] *= F(1.2)                            # a disocclusion: outside the depth tolerance
        prev_normal[(np.arange(P) % w) == w - 1] = (1, 0, 0)        # another surface: outside the normal tolerance
        prev_length[rng.permutation(P)[:8]] = (0, 1, 65535, 0xFFFFFFFF, 0, 1, 65535, 0xFFFFFFFF)
    out = dict(zip(PLANE_NAMES, (color, depth, normal, prev_color, prev_depth, prev_normal, prev_length)))
    if P >= 9:
        # the sprinkle: distinct pixels, a NaN, a +inf and a -inf per float plane (tiny frames: one of them per plane)
        spots = rng.permutation(P)
        bad = [np.nan, np.inf, -np.inf]
        per = 3 if P >= 64 else 1
        k = 0
        for j, name in enumerate(PLANE_NAMES[:6]):
            for i in range(per):
                p = int(spots[k % P])
                k += 1
                v = bad[(i + j) % 3]
                if out[name].ndim == 2:
                    out[name][p, (i + j) % 3] = v
                else:
                    out[name][p] = v
    for a in out.values():
        a.setflags(write=False)
    _PLANES[key] = (cam, prev, out)
    return _PLANES[key]


_WANT = {}


def want(w, h, pair, nrm, lens):
    """The reference's row-major result, once per (frame, pair, guides)."""
    key = (w, h, pair, nrm, lens)
    if key not in _WANT:
        cam, prev, pl = planes(w, h, pair)
        r = rr.reproject(cam, prev, pl["color"], pl["depth"], pl["prev_color"], pl["prev_depth"],
                         pl["normal"] if nrm else None, pl["prev_normal"] if nrm else None,
                         pl["prev_length"] if lens else None, **TOL)
        r = {"color": r["color"].reshape(-1, 3), "length": r["length"].reshape(-1), "motion": r["motion"].reshape(-1, 2),
             "hits": r["hits"]}
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[key] = r
    return _WANT[key]


def _np(a):
    return a.cpu().numpy() if not isinstance(a, np.ndarray) else a


def _bits(a, ch):
    return np.ascontiguousarray(_np(a)).reshape(-1, ch).view(np.uint32)


def _diff(got, ref, what):
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} pixels differ, first at index {bad[0]}: got "
                           f"{[hex(int(v)) for v in got[bad[0]]]}, reference {[hex(int(v)) for v in ref[bad[0]]]}")


def _check(res, ref, order, motion, what):
    _diff(_bits(res["color"], 3), ref["color"].view(np.uint32)[order], what + ("color",))
    _diff(_bits(res["length"], 1), ref["length"].reshape(-1, 1)[order], what + ("length",))
    assert ("motion" in res) == motion, what
    if motion:
        _diff(_bits(res["motion"], 2), ref["motion"].view(np.uint32)[order], what + ("motion",))
    st = res["stats"]
    assert st["hits"] == ref["hits"] and st["samples"] == order.size and st["trace_launches"] == 2, (what, st)
    assert st["segments"] == st["cells_visited"] == st["triangle_tests"] == 0, what


def _given(pl, order, nrm, lens, device):
    names = [k for k in PLANE_NAMES if (nrm or "normal" not in k) and (lens or k != "prev_length")]
    g = {k: np.ascontiguousarray(pl[k][order]) for k in names}
    if device:
        g = {k: torch.from_numpy(v.view(np.int32) if k == "prev_length" else v).cuda() for k, v in g.items()}
    return g


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-t%d-%s" % (s[0], s[1], s[2], "rm" if s[3] else "pk"))
def test_reprojection_is_the_references_bit_for_bit(shape, pair, context):
    w, h, tile, row_major = shape
    ctx = context("cornell").context
    cam, prev, pl = planes(w, h, pair)
    ncam, nprev = rh.to_native(cam), rh.to_native(prev)
    order = np.arange(w * h) if row_major else native.tile_pixels(w, h, tile)
    full = want(w, h, pair, True, True)
    # the reference itself: the pairs do what their names say
    if pair in ("turned away", "degenerate"):
        assert full["hits"] == 0 and (full["motion"].view(np.uint32) == 0x7FC00000).all()
    elif w * h > 9:
        assert 0 < full["hits"] < w * h and len(np.unique(full["length"])) > 3
        assert want(w, h, pair, False, True)["hits"] > full["hits"]  # the normal guide drops taps of its own
    if w * h == 1 and pair == "identical":
        assert full["hits"] == 1 and full["length"][0] == pl["prev_length"][0] + 1
    assert torch is not None, "the device-pointer half needs torch"
    for nrm in (True, False):
        for lens in (True, False):
            ref = want(w, h, pair, nrm, lens)
            for device in (False, True):
                src = _given(pl, order, nrm, lens, device)
                for motion in (True, False):
                    what = (shape, pair, nrm, lens, "device" if device else "host", motion)
                    res = ctx.reproject(ncam, nprev, tile=tile, row_major=row_major, motion=motion, **src, **TOL)
                    _check(res, ref, order, motion, what)


# ------------------------------------------------------------------ guard rows, aliasing
SENT = 0xABABABAB


def _sentinel(n):
    return torch.full((n,), SENT - (1 << 32), dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("ask", ((True, True), (True, False), (False, True), (False, False)),
                         ids=("length+motion", "length", "motion", "colour only"))
def test_guard_rows_and_unasked_outputs_stay_untouched(ask, context):
    assert torch is not None, "device buffers need torch"
    w, h, tile, pair = 33, 31, 32, "translated"
    P = w * h
    ctx = context("cornell").context
    cam, prev, pl = planes(w, h, pair)
    order = native.tile_pixels(w, h, tile)
    src = _given(pl, order, True, True, True)
    ref = want(w, h, pair, True, True)
    guard = 64
    outs = {"color": (_sentinel(3 * (P + 2 * guard)), 3, True), "length": (_sentinel(P + 2 * guard), 1, ask[0]),
            "motion": (_sentinel(2 * (P + 2 * guard)), 2, ask[1])}
    torch.cuda.synchronize()
    ptr = {k: (t.data_ptr() + 4 * ch * guard if asked else None) for k, (t, ch, asked) in outs.items()}
    st = ctx.reproject_raw(rh.to_native(cam), rh.to_native(prev), src["color"].data_ptr(), None, src["depth"].data_ptr(),
                           src["normal"].data_ptr(), src["prev_color"].data_ptr(), src["prev_depth"].data_ptr(),
                           src["prev_normal"].data_ptr(), src["prev_length"].data_ptr(), ptr["color"], ptr["length"],
                           ptr["motion"], True, tile_size=tile, **TOL)
    assert st["hits"] == ref["hits"]
    for k, (t, ch, asked) in outs.items():
        got = t.cpu().numpy().view(np.uint32).reshape(-1, ch)
        assert (got[:guard] == SENT).all() and (got[guard + P:] == SENT).all(), k
        if asked:
            _diff(got[guard:guard + P], ref[k].reshape(-1, ch).view(np.uint32)[order], ("guarded", ask, k))
        else:
            assert (got == SENT).all(), k
    for k, v in src.items():                                         # the inputs are read, never written
        assert np.array_equal(v.cpu().numpy().view(np.uint32), np.ascontiguousarray(pl[k][order]).view(np.uint32)), k


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("pair", ("translated", "mirrored"))
def test_outputs_may_alias_the_planes_the_header_names(pair, device, context):
    assert torch is not None
    w, h, tile = 33, 31, 32
    ctx = context("cornell").context
    cam, prev, pl = planes(w, h, pair)
    ncam, nprev = rh.to_native(cam), rh.to_native(prev)
    order = native.tile_pixels(w, h, tile)
    ref = want(w, h, pair, True, True)

    def call(src, color_out, length_out):
        p = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
        st = ctx.reproject_raw(ncam, nprev, p(src["color"]), None, p(src["depth"]), p(src["normal"]),
                               p(src["prev_color"]), p(src["prev_depth"]), p(src["prev_normal"]),
                               p(src["prev_length"]), p(color_out), p(length_out), None, device, tile_size=tile, **TOL)
        if device:
            torch.cuda.synchronize()
        assert st["hits"] == ref["hits"]

    # the history buffers updated in place
    src = _given(pl, order, True, True, device)
    call(src, src["prev_color"], src["prev_length"])
    _diff(_bits(src["prev_color"], 3), ref["color"].view(np.uint32)[order], (pair, "in place: colour"))
    _diff(_bits(src["prev_length"], 1), ref["length"].reshape(-1, 1)[order], (pair, "in place: length"))
    # the current colour overwritten
    src = _given(pl, order, True, True, device)
    lens = torch.zeros(w * h, dtype=torch.int32, device="cuda") if device else np.zeros(w * h, np.uint32)
    call(src, src["color"], lens)
    _diff(_bits(src["color"], 3), ref["color"].view(np.uint32)[order], (pair, "over the colour"))
    _diff(_bits(lens, 1), ref["length"].reshape(-1, 1)[order], (pair, "over the colour: length"))


# ------------------------------------------------------------------ film source
def _film_equals_color(ctx, film, cam, prev, shown, pl, order, what):
    """reproject(film) == reproject(color = the frame the film's last call
    showed), both == the reference; the film is read, never written."""
    before = film.read()
    counts = film.counts()
    src = _given(pl, order, True, True, False)
    del src["color"]
    a = ctx.reproject(cam, prev, film=film, motion=True, **src, **TOL)
    b = ctx.reproject(cam, prev, color=shown, motion=True, **src, **TOL)
    c = film.reproject(cam, prev, motion=True, **src, **TOL)
    dev = {k: torch.from_numpy(v.view(np.int32) if k == "prev_length" else v).cuda() for k, v in src.items()}
    d = ctx.reproject(cam, prev, film=film, motion=True, **dev, **TOL)
    for k in ("color", "length", "motion"):
        for other in (b, c, d):
            assert np.array_equal(_np(a[k]).view(np.uint32), _np(other[k]).view(np.uint32)), (what, k)
    ref = rr.reproject_packed(order, cam, prev, shown, src["depth"], src["prev_color"], src["prev_depth"], src["normal"],
                              src["prev_normal"], src["prev_length"], **TOL)
    _diff(_bits(a["color"], 3), ref["color"].view(np.uint32), what)
    assert a["stats"]["hits"] == ref["hits"] > 0, what
    after = film.read()
    assert after[1] == before[1] and np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32)), what
    assert np.array_equal(film.counts()[0], counts[0]) and film.counts()[1] == counts[1], what
    return a


@pytest.mark.parametrize("name", rc.SCENES)
def test_a_films_frame_is_its_colour_plane(name, tall, context):
    t, rs = tall(name), context(name)
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)                             # the film's camera; the planes are synthetic
    pcam, pprev, pl = planes(w, h, "translated")
    order = native.tile_pixels(w, h)
    film = rs.context.film(w, h)
    res = rs.context.accumulate(film, cam, 4, MB, seed=t.seed, linear=True)
    assert np.array_equal(res["linear"].view(np.uint32), t.frame(w, h, 4, MB)[1][order])
    a = _film_equals_color(rs.context, film, rh.to_native(pcam), rh.to_native(pprev), res["linear"], pl, order,
                           (name, "accumulate"))
    assert (_np(a["color"]).view(np.uint32) != res["linear"].view(np.uint32)).any()
    film.close()


@pytest.mark.parametrize("case", [k for k in rc.PARITY if k[3] == rc.SCHEDULE and k[5] == 0 and k[4] == 0.125 and
                                  k[1:3] == (13, 5)], ids=lambda k: "%s-%dx%d" % k[:3])
def test_a_refined_films_frame_uses_every_pixels_own_count(case, tall, context):
    name, w, h, schedule, thr, min_s = case
    t, rs = tall(name), context(name)
    cam = camera_for(t.soup, None, w, h)
    pcam, pprev, pl = planes(w, h, "yawed")
    order = native.tile_pixels(w, h)
    film = rs.context.film(w, h)
    frozen = False
    for j, n in enumerate(schedule[:4]):
        res = rs.context.refine(film, cam, n, MB, thr, min_s, seed=t.seed, linear=True, counts=True)
        assert res["active"] == rc.PARITY[case][j]
        if 0 < res["active"] < w * h:                              # per-pixel counts are in play
            assert len(np.unique(res["counts"])) > 1
            frozen = True
            _film_equals_color(rs.context, film, rh.to_native(pcam), rh.to_native(pprev), res["linear"], pl, order, (case, j))
    assert frozen
    film.close()


def test_film_refusals_with_their_control(tall, context):
    t, rs = tall("cornell"), context("cornell")
    ctx = rs.context
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    pcam, pprev, pl = planes(w, h, "translated")
    ncam, nprev = rh.to_native(pcam), rh.to_native(pprev)
    swapped = rh.to_native(rh.pinhole(h, w))
    src = _given(pl, native.tile_pixels(w, h), False, False, False)
    film = ctx.film(w, h)
    out = np.full((w * h, 3), 0xA0A0A0A0, np.uint32)

    def call(cams=(ncam, nprev), tile=64, f=film, color=None, flags=0, on=ctx):
        return on.reproject_raw(cams[0], cams[1], color, f, src["depth"].ctypes.data, None, src["prev_color"].ctypes.data,
                                src["prev_depth"].ctypes.data, None, None, out.ctypes.data, None, None, False,
                                tile_size=tile, flags=flags, **TOL)

    def refused(**kw):
        with pytest.raises(native.ZrtError) as e:
            call(**kw)
        assert e.value.status == -1, kw
        assert (out == 0xA0A0A0A0).all(), kw

    refused()                                                      # an empty film
    ctx.accumulate(film, cam, 4, MB, seed=t.seed)
    refused(cams=(swapped, swapped))                               # another frame
    refused(tile=32)                                               # another tile
    refused(color=src["color"].ctypes.data)                        # both sources
    refused(flags=native.REPROJECT_ROW_MAJOR)                      # a film is never row-major
    other = _scene(t)
    refused(on=other.context)                                      # another context's film
    other.close()
    part = ctx.film(w, h, 8, 1, 2)                                 # rank 1 of 2
    ctx.accumulate(part, cam, 4, MB, seed=t.seed)
    refused(f=part, tile=8)
    part.close()
    assert call()["samples"] == w * h                              # the control
    assert (out != 0xA0A0A0A0).all()
    film.close()


# ------------------------------------------------------------------ scene frames
def _device_features(ctx, cam, spp, seed, P):
    buf = {"base_color": torch.zeros((P, 3), dtype=torch.float32, device="cuda"),
           "normal": torch.zeros((P, 3), dtype=torch.float32, device="cuda"),
           "depth": torch.zeros((P,), dtype=torch.float32, device="cuda")}
    torch.cuda.synchronize()
    ctx.features_raw(cam, spp, {k: v.data_ptr() for k, v in buf.items()}, True, seed)
    return buf


@pytest.mark.parametrize("name", rc.SCENES)
def test_scene_frames_through_reproject_and_denoise(name, tall, context):
    """The GPU's own planes: features at A and B, a 64-sample frame at A with
    history length 16, a 4-sample film at B; the result and its denoised frame
    against the references fed the same planes."""
    assert torch is not None
    t, ctx = tall(name), context(name).context
    w, h, spp, before, _, length = rh.QUALITY
    P = w * h
    order = native.tile_pixels(w, h)
    A = camera_for(t.soup, None, w, h)
    B = rh.to_native(rr.moved(A, *rh.MOVES[name]["both"]))
    fa, fb = _device_features(ctx, A, spp, t.seed, P), _device_features(ctx, B, spp, t.seed, P)
    prev = ctx.render(A, before, MB, seed=t.seed, packed=True, linear=True)["linear"]
    assert np.array_equal(prev.view(np.uint32), t.frame(w, h, before, MB)[1][order])
    film = ctx.film(w, h)
    shown = ctx.accumulate(film, B, spp, MB, seed=t.seed, linear=True)["linear"]
    lens = torch.full((P,), length, dtype=torch.int32, device="cuda")
    res = ctx.reproject(B, A, film=film, depth=fb["depth"], normal=fb["normal"], prev_color=torch.from_numpy(prev).cuda(),
                        prev_depth=fa["depth"], prev_normal=fa["normal"], prev_length=lens, motion=True)
    host = {k: {n: v.cpu().numpy() for n, v in f.items()} for k, f in (("a", fa), ("b", fb))}
    mx, dt, nt = native.REPROJECT_DEFAULTS
    ref = rr.reproject_packed(order, B, A, shown, host["b"]["depth"], prev, host["a"]["depth"], host["b"]["normal"],
                              host["a"]["normal"], np.full(P, length, np.uint32), max_history=mx, depth_tolerance=dt,
                              normal_tolerance=nt)
    _check(res, {"color": ref["color"], "length": ref["length"], "motion": ref["motion"], "hits": ref["hits"]},
           np.arange(P), True, (name, "scene"))
    assert ref["hits"] >= P // 2                                   # the host test's condition holds for the GPU's planes too
    den = ctx.denoise(w, h, color=res["color"], normal=fb["normal"], depth=fb["depth"], albedo=fb["base_color"])
    sc, sn, sz, sa = native.DENOISE_SIGMAS
    dref = dr.denoise_packed(order, w, h, ref["color"], 5, sc, host["b"]["normal"], sn, host["b"]["depth"], sz,
                             host["b"]["base_color"], sa)
    _diff(_bits(den["linear"], 3), dref.view(np.uint32), (name, "denoised"))
    film.close()


# ------------------------------------------------------------------ History
def test_history_updates_equal_the_calls_made_by_hand(tall, context):
    assert torch is not None
    t, ctx = tall("cornell"), context("cornell").context
    w, h = 33, 31
    P = w * h
    A = camera_for(t.soup, None, w, h)
    cams = [A, rh.to_native(rr.moved(A, (0.1, 0.05, 0.0))), rh.to_native(rr.moved(A, (0.2, 0.1, 0.1), 0.05))]
    film = ctx.film(w, h)
    hist = native.History(ctx, w, h)
    by_hand = None
    for j, cam in enumerate(cams):
        film.reset()
        shown = ctx.accumulate(film, cam, 4, MB, seed=t.seed + j, linear=True)["linear"]
        got = hist.update(film, cam, seed=t.seed + j, num_samples=4)
        assert sorted(got) == ["albedo", "color", "depth", "normal"]
        f = _device_features(ctx, cam, 4, t.seed + j, P)
        if by_hand is None:
            color, lens = torch.from_numpy(shown).cuda(), torch.ones(P, dtype=torch.int32, device="cuda")
            assert hist.stats["samples"] == P
        else:
            r = ctx.reproject(cam, cams[j - 1], color=torch.from_numpy(shown).cuda(), depth=f["depth"], normal=f["normal"],
                              prev_color=by_hand[0], prev_depth=by_hand[2]["depth"], prev_normal=by_hand[2]["normal"],
                              prev_length=by_hand[1])
            color, lens = r["color"], r["length"]
            assert hist.stats["hits"] == r["stats"]["hits"] > P // 2
        by_hand = (color, lens, f)
        what = ("update", j)
        _diff(_bits(got["color"], 3), _bits(color, 3), what + ("color",))
        _diff(_bits(hist.length, 1), _bits(lens, 1), what + ("length",))
        for k, n in (("normal", "normal"), ("depth", "depth"), ("albedo", "base_color")):
            assert np.array_equal(_np(got[k]).view(np.uint32), _np(f[n]).view(np.uint32)), what + (k,)
    assert len(np.unique(_np(hist.length))) == 3                   # 1, 2 and 3
    den = ctx.denoise(w, h, tile=hist.tile, **got)                 # what Context.denoise takes
    assert _np(den["linear"]).shape == (P, 3)
    film.close()


def test_a_static_camera_grows_the_history_by_one_per_update(tall, context):
    assert torch is not None
    t, ctx = tall("cornell"), context("cornell").context
    w, h = 33, 31                                                  # (Cornell at 13 x 5 is mostly sky)
    A = camera_for(t.soup, None, w, h)
    film = ctx.film(w, h)
    hist = native.History(ctx, w, h)
    for j in (1, 2, 3):
        film.reset()
        ctx.accumulate(film, A, 4, MB, seed=t.seed)
        got = hist.update(film, A, seed=t.seed, num_samples=4)
        lens, depth, color = _np(hist.length), _np(got["depth"]), _np(got["color"])
        seen = (depth > 0) & np.isfinite(color).all(axis=1)
        assert seen.sum() > w * h // 2
        assert (lens[seen] == j).all() and (lens[~seen] == 1).all(), j
    hist.reset()
    film.reset()
    shown = ctx.accumulate(film, A, 4, MB, seed=t.seed, linear=True)["linear"]
    got = hist.update(film, A, seed=t.seed, num_samples=4)
    assert (_np(hist.length) == 1).all() and np.array_equal(_np(got["color"]).view(np.uint32), shown.view(np.uint32))
    film.close()


# ------------------------------------------------------------------ alternation, stats, refusals
def test_reproject_alternates_with_renders_features_and_denoise(tall):
    t = tall("cornell")
    w, h = 13, 5
    cam = camera_for(t.soup, None, w, h)
    order = native.tile_pixels(w, h)
    sets = {}
    for pair in ("translated", "yawed"):
        pcam, pprev, pl = planes(w, h, pair)
        sets[pair] = (rh.to_native(pcam), rh.to_native(pprev), _given(pl, order, True, True, False))

    def render(rs, spp):
        r = rs.context.render(cam, spp, MB, seed=t.seed, packed=True, linear=True)
        return r["packed"], r["linear"].view(np.uint32), {k: r["stats"][k] for k in ("segments", "samples")}, \
            rs.context.profile()

    def reproject(rs, pair):
        a, b, src = sets[pair]
        r = rs.context.reproject(a, b, motion=True, **src, **TOL)
        return r["color"].view(np.uint32), r["length"], r["motion"].view(np.uint32), r["stats"]["hits"]

    def features(rs):
        f = rs.context.features(cam, 3, seed=t.seed)
        return [f[n].view(np.uint32) for n, _ in native.FEATURE_PLANES]

    def denoise(rs):
        src = sets["translated"][2]
        r = rs.context.denoise(w, h, color=np.abs(np.nan_to_num(src["color"], posinf=1.0, neginf=1.0)), rgb=True)
        return r["linear"].view(np.uint32), r["rgb"]

    steps = ((render, 5), (reproject, "translated"), (features,), (denoise,), (reproject, "yawed"), (render, 7))
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
        if fn is reproject and j == 1:
            assert rs.context.profile() == fresh[0][3]             # still the first render's
    assert rs.context.profile() == fresh[-1][3]                    # the last render's, untouched by the reprojection
    rs.close()
    ref = want(w, h, "translated", True, True)
    assert np.array_equal(fresh[1][0], ref["color"].view(np.uint32)[order]) and fresh[1][3] == ref["hits"]


def test_stats(context):
    ctx = context("cornell").context
    w, h, pair = 33, 31, "translated"
    cam, prev, pl = planes(w, h, pair)
    order = native.tile_pixels(w, h, 32)
    ref = want(w, h, pair, True, True)
    zero = dict(segments=0, cells_visited=0, triangle_tests=0)
    st = ctx.reproject(rh.to_native(cam), rh.to_native(prev), tile=32, **_given(pl, order, True, True, False), **TOL)["stats"]
    assert {k: st[k] for k in zero} == zero and st["samples"] == w * h and st["hits"] == ref["hits"]
    assert st["trace_launches"] == 2                               # the gather and the reprojection
    assert 0 < st["trace_kernel_ms"] <= st["render_ms"]            # a host call: the copies are not kernel time
    if torch is not None:
        sd = ctx.reproject(rh.to_native(cam), rh.to_native(prev), tile=32, **_given(pl, order, True, True, True), **TOL)["stats"]
        assert {k: sd[k] for k in zero} == zero and sd["samples"] == w * h and sd["hits"] == ref["hits"]
        assert sd["trace_launches"] == 2 and 0 < sd["trace_kernel_ms"] == sd["render_ms"]


def test_refusals_with_their_control(context):
    """test_reproject_host.py's refusals on a real context: each is refused for
    its own reason, the outputs untouched -- the same batch, made valid,
    succeeds, and so does what the header allows."""
    ctx = context("cornell").context
    L = native.lib()
    x, outs = rh.host_planes(), rh.guarded_outputs()
    st = native.Stats()
    for name, change in rh.REFUSALS.items():
        batch = native.ReprojectBatch(**{**rh._valid(x, outs), **change})
        assert L.zrt_context_reproject(ctx._h, C.byref(batch), C.byref(st)) == -1, name
        assert rh.untouched(outs), name
    for name, change in [("valid", {})] + [(k, v) for k, v in rh.ALLOWED.items() if k != "P = 2^31"]:
        outs = rh.guarded_outputs()
        batch = native.ReprojectBatch(**{**rh._valid(x, outs), **change})
        assert L.zrt_context_reproject(ctx._h, C.byref(batch), C.byref(st)) == 0, name
        assert st.samples == 64 and st.trace_launches == 2, name
        assert (outs[0] != 0xA0A0A0A0).all(), name
        assert (outs[1] == 0xB1B1B1B1).all() == (batch.length_out is None), name
        assert (outs[2] == 0xC2C2C2C2).all() == (batch.motion is None), name
        if name in ("valid", "tolerances +inf"):
            assert st.hits == 64, name                             # a flat wall 6 away, moved by 0.05: history everywhere
        if name == "max_history 1":
            assert (outs[1] == 1).all() and (outs[0].view(F) == 0.5).all(), name
