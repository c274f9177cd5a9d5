"""Adaptive films: zrt_context_refine samples only unconverged pixels.

The contract: every pixel of an adaptive frame is, bit for bit, the oracle's
pixel at that pixel's own sample count -- RGB8 and the linear radiance as uint32
patterns -- and which pixels a call traces follows from oracle frames alone
(refine_ref.py).  A call's stats are those of the traced paths: the oracle's
counters of the active pixels at b + n samples minus those at b.  The reference
is always the CPU oracle (refine_cases.py), never a GPU render.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native

import refine_cases as rc
import refine_ref

pytestmark = pytest.mark.gpu
MB = rc.MB
ZERO = dict(segments=0, cells_visited=0, triangle_tests=0, hits=0, samples=0, trace_launches=0)


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


def _pixels_at_their_counts(t, w, h, pix, counts, res, what):
    """Every owned pixel's outputs against the oracle's frame at that pixel's count."""
    assert np.array_equal(res["counts"], counts), what
    for N in np.unique(counts):
        rgb, bits, _ = t.frame(w, h, int(N), MB)
        at = counts == N
        assert np.array_equal(res["packed"][at], rgb[pix[at]]), (what, int(N))
        assert np.array_equal(res["linear"].view(np.uint32)[at], bits[pix[at]]), (what, int(N))


def _stats(t, w, h, b, n, traced, st, counting, what):
    """A call's stats against the oracle's counters of the traced pixels' samples b .. b + n - 1."""
    if traced.size == 0:
        assert {k: st[k] for k in ZERO} == ZERO and st["render_ms"] == 0.0, what
        return
    ctr = rc.call_counters(t, w, h, b, n, traced)
    assert st["samples"] == traced.size * n and st["segments"] == int(ctr[0]), what
    if counting:
        assert (st["cells_visited"], st["triangle_tests"], st["hits"]) == tuple(int(x) for x in ctr[1:4]), what


def _refine(t, rs, film, w, h, schedule, thr, min_s, flags=0, counting=False, pix=None, calls=None, passes=None,
            image=None):
    """The schedule into the reset film; every call's active count, counts,
    outputs, stats and the film's own account against the oracle.  Returns the
    calls' stats."""
    cam = camera_for(t.soup, None, w, h)
    if pix is None:
        pix = native.tile_pixels(w, h)
    if calls is None:
        calls = rc.expect(t, w, h, schedule, thr, min_s)
    film.reset()
    assert film.counts()[1] == pix.size and not film.counts()[0].any()
    out = []
    for j, (n, (b, active, counts)) in enumerate(zip(schedule, calls)):
        what = (t.name, w, h, schedule, thr, min_s, j, hex(flags), counting)
        A = int(active.sum())
        res = rs.context.refine(film, cam, n, MB, thr, min_s, seed=t.seed, stats=counting, flags=flags, packed=True,
                                linear=True, counts=True, image=image,
                                samples_per_pass=passes[j] if passes else 0)
        assert res["active"] == A, (what, res["active"], A)
        after = b + n if A else b
        assert res["samples"] == after and film.info() == (pix.size, after), what
        _pixels_at_their_counts(t, w, h, pix, counts, res, what)
        got, act = film.counts()
        assert act == A and np.array_equal(got, counts), what
        _stats(t, w, h, b, n, pix[active], res["stats"], counting, what)
        out.append(res["stats"])
    return out


@pytest.mark.parametrize("mode", list(rc.RENDER_MODES))
@pytest.mark.parametrize("case", list(rc.PARITY), ids=lambda k: "%s-%dx%d-%d-%g-%d" % (k[0], k[1], k[2], len(k[3]), k[4], k[5]))
def test_every_pixel_is_the_oracles_at_its_own_count(case, mode, tall, context):
    name, w, h, schedule, thr, min_s = case
    t, rs = tall(name), context(name)
    flags, counting = rc.RENDER_MODES[mode]
    film = rs.context.film(w, h)
    stats = _refine(t, rs, film, w, h, schedule, thr, min_s, flags, counting)
    active = rc.PARITY[case]
    one = 1 if counting else MB
    if schedule == rc.BIG_SCHEDULE:
        # 2^23 samples or more on the sparse list: two pass sets, as a render of 819 pixels takes them
        assert active[3] * schedule[3] >= rc.BIG > w * h * schedule[2]
        prof = rs.context.profile()
        assert prof["sets"] == 1 if counting else (prof["sets"] == 2 and prof["passes"] >= 2)
        assert [s["trace_launches"] for s in stats[:3]] == [one] * 3
        assert stats[3]["trace_launches"] == prof["passes"] * one
    else:
        assert [s["trace_launches"] for s in stats] == [one if a else 0 for a in active]
    film.close()


@pytest.mark.parametrize("mode", list(rc.RENDER_MODES))
@pytest.mark.parametrize("name", rc.SCENES)
def test_nothing_frozen_is_accumulate(name, mode, tall, context):
    """min_samples no film reaches: the calls are accumulate's, the frame so far and its stats."""
    t, rs = tall(name), context(name)
    flags, counting = rc.RENDER_MODES[mode]
    w, h, schedule = 13, 5, (15, 17, 32)
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(w, h)
    film = rs.context.film(w, h)
    done, prev = 0, np.zeros(5, np.uint64)
    for n in schedule:
        res = rs.context.refine(film, cam, n, MB, 0.125, rc.NEVER, seed=t.seed, stats=counting, flags=flags,
                                packed=True, linear=True, counts=True)
        done += n
        rgb, bits, ctr = t.frame(w, h, done, MB)
        assert res["active"] == w * h and res["samples"] == done and (res["counts"] == done).all()
        assert np.array_equal(res["packed"], rgb[pix]) and np.array_equal(res["linear"].view(np.uint32), bits[pix])
        st = res["stats"]
        assert st["samples"] == w * h * n and st["segments"] == int(ctr[0] - prev[0])
        assert st["trace_launches"] == (1 if counting else MB)
        if counting:
            assert (st["cells_visited"], st["triangle_tests"], st["hits"]) == tuple(int(x) for x in (ctr - prev)[1:4])
        prev = ctr
    film.close()


@pytest.mark.parametrize("mode", list(rc.RENDER_MODES))
def test_passes_on_a_sparse_list(mode, tall, context):
    """The last call: 32 samples as 7 passes of 5 on 16 of 65 pixels -- the
    sparse resolve's first pass of a call and its later ones; launches as a
    fresh context's render of a 16-pixel-wide frame."""
    name, w, h, schedule, thr, min_s, spp_pass = rc.PASSES
    t, rs = tall(name), context(name)
    flags, counting = rc.RENDER_MODES[mode]
    A = rc.PARITY[(name, w, h, schedule, thr, min_s)][-1]
    assert 0 < A < w * h
    fresh = _scene(t)
    want = fresh.render(camera_for(t.soup, None, A, 1), num_samples=schedule[-1], max_bounce=MB, seed=t.seed,
                        samples_per_pass=spp_pass, stats=counting, flags=flags)[1]["stats"]["trace_launches"]
    fresh.close()
    assert want == 7 * (1 if counting else MB)
    film = rs.context.film(w, h)
    stats = _refine(t, rs, film, w, h, schedule, thr, min_s, flags, counting, passes=(0, 0, 0, 0, spp_pass))
    assert stats[-1]["trace_launches"] == want and rs.context.profile()["passes"] == 7
    # ... and in every call, the first (from +0) included
    _refine(t, rs, film, w, h, schedule, thr, min_s, flags, counting, passes=(3, 3, 3, 5, 5))
    film.close()


@pytest.mark.parametrize("name", rc.SCENES)
def test_ranks_each_with_a_film(name, tall, context):
    t, rs = tall(name), context(name)
    w, h, schedule, thr, min_s, tile, nranks = rc.RANKS
    films = [rs.context.film(w, h, tile, r, nranks) for r in range(nranks)]
    pixs = [native.tile_pixels(w, h, tile, r, nranks) for r in range(nranks)]
    img = np.full((h, w, 3), 0x5A, np.uint8)
    counts = np.zeros(w * h, np.uint32)
    frozen = 0
    for f, pix in zip(films, pixs):
        calls = rc.expect(t, w, h, schedule, thr, min_s, pix)
        _refine(t, rs, f, w, h, schedule, thr, min_s, pix=pix, calls=calls, image=img)
        counts[pix] = calls[-1][2]
        frozen += int((~calls[-1][1]).sum())
    assert frozen > 0 and np.unique(counts).size >= 3
    # the rgb_image scatter of the ranks' last calls: the whole frame, every pixel at its count
    flat = img.reshape(-1, 3)
    for N in np.unique(counts):
        assert np.array_equal(flat[counts == N], t.frame(w, h, int(N), MB)[0][counts == N]), (name, int(N))
    for f in films:
        f.close()


def test_an_all_converged_call_traces_nothing(tall, context):
    name, w, h, schedule, thr, min_s = rc.CONVERGED
    t, rs = tall(name), context(name)
    more = schedule + (32, 1)
    calls = rc.expect(t, w, h, more, thr, min_s)
    assert [int(a.sum()) for _, a, _ in calls][-3:] == [0, 0, 0]
    assert calls[-1][0] == calls[-3][0] == sum(schedule[:-1]) and np.array_equal(calls[-1][2], calls[-3][2])
    film = rs.context.film(w, h)
    for flags, counting in rc.RENDER_MODES.values():
        stats = _refine(t, rs, film, w, h, more, thr, min_s, flags, counting)       # (_stats: all zero when A == 0)
        assert all(s["trace_kernel_ms"] == 0.0 for s in stats[-3:])
    sums = film.read()
    assert sums[1] == sum(schedule[:-1])
    # the sums as stored, over each pixel's own count, are the oracle's pixels
    n = calls[-1][2]
    lin = sums[0] * (np.float32(1.0) / n.astype(np.float32))[:, None]
    pix = native.tile_pixels(w, h)
    for N in np.unique(n):
        assert np.array_equal(lin.view(np.uint32)[n == N], t.frame(w, h, int(N), MB)[1][pix[n == N]])
    film.close()


def test_accumulate_and_refine_on_one_film(tall, context):
    """accumulate is allowed while nothing is frozen and leaves the checkpoint
    alone -- the next refine compares 16 samples with 4, k = 16 / 12 -- and is
    refused once a pixel is frozen.  Reset and write clear the state."""
    name, w, h, thr = rc.ACCUMULATE
    t, rs = tall(name), context(name)
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(w, h)
    P = w * h
    lin = rc.lin_of(t, w, h, pix)
    film = rs.context.film(w, h)
    ask = dict(seed=t.seed, packed=True, linear=True)
    assert rs.context.refine(film, cam, 4, MB, thr, **ask)["active"] == P          # b 0 -> 4, no checkpoint
    assert rs.context.refine(film, cam, 4, MB, thr, **ask)["active"] == P          # b 4 -> 8, checkpoints at 4
    res = rs.context.accumulate(film, cam, 8, MB, **ask)                           # b 8 -> 16
    assert np.array_equal(res["linear"].view(np.uint32), t.frame(w, h, 16, MB)[1][pix])
    with np.errstate(invalid="ignore"):
        active = refine_ref.error(lin(16), lin(4), 16, 4) > np.float32(thr)
        near = refine_ref.error(lin(16), lin(8), 16, 8) > np.float32(thr)
    assert 0 < active.sum() < P and not np.array_equal(active, near)               # (the longer gap decides otherwise)
    counts = np.where(active, 32, 16).astype(np.uint32)
    res = rs.context.refine(film, cam, 16, MB, thr, counts=True, stats=True, **ask)
    assert res["active"] == int(active.sum()) and film.info() == (P, 32)
    _pixels_at_their_counts(t, w, h, pix, counts, res, name)
    _stats(t, w, h, 16, 16, pix[active], res["stats"], True, name)

    sums = film.read()[0].copy()
    cfg = native.RenderConfig()
    cfg.num_samples, cfg.max_bounce, cfg.seed, cfg.device = 4, MB, t.seed, -1
    packed = np.full((P, 3), 0xC3, np.uint8)
    outs = native.Outputs(None, packed.ctypes.data, None, None)
    st = native.Stats()
    L = native.lib()
    assert L.zrt_context_accumulate(rs.context._h, film._h, C.byref(cam), C.byref(cfg), C.byref(outs), C.byref(st)) == -1
    assert (packed == 0xC3).all() and film.info() == (P, 32)
    assert np.array_equal(film.read()[0].view(np.uint32), sums.view(np.uint32))
    got, act = film.counts()
    assert act == int(active.sum()) and np.array_equal(got, counts)

    # write and reset thaw every pixel and forget the checkpoint
    film.write(sums, 32)
    got, act = film.counts()
    assert act == P and (got == 32).all()
    film.reset()
    got, act = film.counts()
    assert act == P and not got.any()
    res = rs.context.accumulate(film, cam, 8, MB, **ask)
    assert np.array_equal(res["linear"].view(np.uint32), t.frame(w, h, 8, MB)[1][pix])
    res = rs.context.refine(film, cam, 8, MB, 1e30, counts=True, **ask)            # no checkpoint: nothing to decide
    assert res["active"] == P and (res["counts"] == 16).all()
    res = rs.context.refine(film, cam, 16, MB, 1e30, counts=True, **ask)           # ... now everything freezes, at 16
    assert res["active"] == 0 and (res["counts"] == 16).all() and film.info() == (P, 16)
    assert np.array_equal(res["linear"].view(np.uint32), t.frame(w, h, 16, MB)[1][pix])
    film.close()


def test_a_refined_film_is_isolated_from_the_context(tall, context):
    """Between refine calls the context renders a frame of several passes,
    traces, takes feature planes and serves another film; calls ask for no
    output, and one writes RGB8 into device memory between guard bytes."""
    assert torch is not None
    name, w, h, schedule, thr = rc.ISOLATION
    t, rs = tall(name), context(name)
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(w, h)
    calls = rc.expect(t, w, h, schedule, thr, 0)
    assert 0 < calls[-1][1].sum() < w * h
    film = rs.context.film(w, h)
    rw, rh, rspp, rmb, rpass = 13, 10, 64, 4, 16
    rcam = camera_for(t.soup, None, rw, rh)
    other = rs.context.film(rw, rh)
    guard, nb = 64, 3 * w * h
    buf = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    for j, (n, (b, active, counts)) in enumerate(zip(schedule, calls)):
        last = j + 1 == len(schedule)
        res = rs.context.refine(film, cam, n, MB, thr, seed=t.seed, counts=last, linear=last,
                                device_ptr=buf.data_ptr() + guard if last else None)
        assert res["active"] == int(active.sum()) and "packed" not in res
        before = film.read()
        img, _ = rs.render(rcam, num_samples=rspp, max_bounce=rmb, seed=t.seed, samples_per_pass=rpass)
        assert np.array_equal(img.reshape(-1, 3), t.frame(rw, rh, rspp, rmb)[0])
        rs.trace(t.o[:65], t.d[:65])
        rs.features(rcam, 3, seed=t.seed)
        rs.context.accumulate(other, rcam, 3, rmb, seed=t.seed, packed=True, linear=True)
        after = film.read()
        assert after[1] == before[1] and np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32))
        assert np.array_equal(film.counts()[0], counts)
    got = buf.cpu().numpy()
    assert (got[:guard] == 0xA5).all() and (got[guard + nb:] == 0xA5).all()
    res["packed"] = got[guard:guard + nb].reshape(-1, 3)
    _pixels_at_their_counts(t, w, h, pix, calls[-1][2], res, name)
    other.close()
    film.close()


def _raw(ctx, film, cam, n, mb, seed, outs, rf, tile=64, rank=0, num_ranks=2, active=None):
    cfg = native.RenderConfig()
    cfg.num_samples, cfg.max_bounce, cfg.seed, cfg.device = n, mb, seed, -1
    cfg.tile_size, cfg.rank, cfg.num_ranks = tile, rank, num_ranks
    st = native.Stats()
    return native.lib().zrt_context_refine(ctx._h, film._h, C.byref(cam), C.byref(cfg),
                                           C.byref(rf) if rf is not None else None, C.byref(outs), C.byref(st),
                                           C.byref(active) if active is not None else None)


def test_refusals_leave_film_counts_and_outputs_untouched(tall, context):
    t, rs, rs2 = tall("cornell"), context("cornell"), context("fuzz")
    w, h, thr = 13, 5, 0.125
    P = w * h
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(w, h)
    film = rs.context.film(w, h, 64, 0, 2)               # rank 0 of 2 owns the one tile
    foreign = rs2.context.film(w, h, 64, 0, 2)
    calls = rc.expect(t, w, h, (4, 4, 8, 16), thr, 0)
    for n in (4, 4, 8):
        rs.context.refine(film, cam, n, MB, thr, seed=t.seed)
    base, counts0 = 16, calls[2][2]
    A0 = int(calls[2][1].sum())
    assert 0 < A0 < P and film.info() == (P, base)
    sums = film.read()[0].copy()

    img = np.full((h, w, 3), 0xC3, np.uint8)
    packed = np.full((P, 3), 0xC3, np.uint8)
    lin = np.full((P, 3), -7.0, np.float32)
    cnt = np.full(P, 0xC3C3C3C3, np.uint32)
    outs = native.Outputs(img.ctypes.data, packed.ctypes.data, lin.ctypes.data, None)

    def config(threshold=thr):
        rf = native.RefineConfig()
        rf.sample_counts, rf.threshold, rf.min_samples = cnt.ctypes.data, threshold, 0
        return rf

    def untouched(what):
        assert film.info() == (P, base), what
        got, s = film.read()
        assert s == base and np.array_equal(got.view(np.uint32), sums.view(np.uint32)), what
        got, act = film.counts()
        assert act == A0 and np.array_equal(got, counts0), what
        assert (img == 0xC3).all() and (packed == 0xC3).all() and (lin == -7.0).all(), what
        assert (cnt == 0xC3C3C3C3).all(), what

    ctx = rs.context
    wide, tall_cam = camera_for(t.soup, None, w + 1, h), camera_for(t.soup, None, w, h + 1)
    refused = {
        "n = 0": (film, cam, dict(n=0)),
        "b + n = 65536": (film, cam, dict(n=65536 - base)),
        "w": (film, wide, {}), "h": (film, tall_cam, {}),
        "tile_size": (film, cam, dict(tile=32)), "tile_size default": (film, cam, dict(tile=8)),
        "rank": (film, cam, dict(rank=1)), "num_ranks": (film, cam, dict(num_ranks=3)),
        "num_ranks default": (film, cam, dict(num_ranks=0)),
        "another context's film": (foreign, cam, {}),
        "null refine": (film, cam, dict(rf=None)),
        "NaN threshold": (film, cam, dict(rf=config(float("nan")))),
    }
    for what, (f, c, kw) in refused.items():
        args = dict(n=16, mb=MB, seed=t.seed, outs=outs, rf=config())
        args.update(kw)
        assert _raw(ctx, f, c, **args) == -1, what
        untouched(what)
    assert foreign.info() == (P, 0)
    assert _raw(ctx, film, cam, 16, 33, t.seed, outs, config()) == -5             # ZRT_ERR_UNSUPPORTED
    untouched("max_bounce 33")
    # the control: the same call with nothing wrong goes through (tile 0 = 64)
    active = C.c_uint32(0)
    assert _raw(ctx, film, cam, 16, MB, t.seed, outs, config(), tile=0, active=active) == 0
    b, act, counts = calls[3]
    assert active.value == int(act.sum()) and film.info() == (P, 32) and np.array_equal(cnt, counts)
    _pixels_at_their_counts(t, w, h, pix, counts, dict(counts=cnt, packed=packed, linear=lin), "control")
    flat = img.reshape(-1, 3)
    assert np.array_equal(flat[pix], packed)
    film.close()
    foreign.close()
