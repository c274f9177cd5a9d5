"""Films: zrt_context_accumulate continues a frame's samples across calls.

The contract: any split of N samples over calls is, bit for bit, one render of
N samples -- RGB8, the linear radiance as uint32 patterns, and the calls'
segments (with the counting build also cells_visited, triangle_tests and hits)
summed.  The reference is the CPU oracle at the total sample count
(film_cases.py: the scenes, frames and oracle cache of test_tall_gpu.py), never
a GPU render.

Split parity: frames 1x1, 3x3 and 13x5; 64 samples as (64), (1, 63), (63, 1),
4 x 16, (15, 17, 32) and 64 x 1; 4096 as (4095, 1) and (1, 4095); 65535 on 1x1
as (65534, 1) and (1, 65534); the default kernels, the lane walk, the
IEEE-division kernels and the counting build; max_bounce 4, and 0 and 1 on
1x1.  Then: every intermediate call, several passes inside a continuing call,
two pass sets with a non-zero base, ranks, isolation from what else a context
does between a film's calls, checkpoints, and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native

import film_cases as fc

pytestmark = pytest.mark.gpu
COUNTERS = ("segments", "cells_visited", "triangle_tests", "hits", "samples")


@pytest.fixture(scope="module")
def tall(oracle_mod):
    return lambda name: fc.tall_scene(oracle_mod, name)


def _scene(t):
    return RenderScene(t.soup, fc.RES, device=0, device_build=t.name == "fuzz")


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


def _add(tot, st):
    for k in COUNTERS:
        tot[k] = tot.get(k, 0) + st[k]


def _same(t, w, h, spp, mb, res, pix, what):
    """A call's packed outputs against the oracle's frame at spp."""
    rgb, bits, _ = t.frame(w, h, spp, mb)
    assert np.array_equal(res["packed"], rgb[pix]), what
    assert np.array_equal(res["linear"].view(np.uint32), bits[pix]), what


def _totals(t, w, h, spp, mb, tot, counting, what):
    ctr = t.frame(w, h, spp, mb)[2]
    assert tot["segments"] == int(ctr[0]) and tot["samples"] == w * h * spp, what
    if counting:
        assert tuple(tot[k] for k in COUNTERS[1:4]) == tuple(int(x) for x in ctr[1:4]), what


def _split(t, rs, film, w, h, counts, mb, flags=0, counting=False, every=False, **kw):
    """counts over calls into the reset film; the last call's outputs (every
    call's, with `every`) and the summed stats against the oracle.  Calls
    whose outputs are not compared ask for none."""
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(w, h)
    film.reset()
    tot, done, stats = {}, 0, []
    for j, n in enumerate(counts):
        ask = every or j + 1 == len(counts)
        res = rs.context.accumulate(film, cam, n, mb, seed=t.seed, stats=counting, flags=flags, packed=ask,
                                    want_linear=ask, **kw)
        done += n
        what = (t.name, w, h, counts, j, mb, hex(flags), counting)
        assert res["samples"] == done == film.info()[1], what
        assert res["stats"]["samples"] == w * h * n, what
        if ask:
            _same(t, w, h, done, mb, res, pix, what)
        _add(tot, res["stats"])
        stats.append(res["stats"])
    _totals(t, w, h, done, mb, tot, counting, (t.name, w, h, counts, mb, hex(flags), counting))
    return stats


@pytest.mark.parametrize("w,h,total,mb", fc.PARITY)
@pytest.mark.parametrize("name", fc.SCENES)
def test_any_split_is_the_one_shot_frame(name, w, h, total, mb, tall, context):
    t, rs = tall(name), context(name)
    film = rs.context.film(w, h)
    assert film.info() == (w * h, 0)
    for counts in fc.SPLITS[total]:
        for flags, counting in fc.RENDER_MODES.values():
            for st in _split(t, rs, film, w, h, counts, mb, flags, counting):
                assert st["trace_launches"] == (1 if counting else max(mb, 1))      # one pass each
    film.close()


@pytest.mark.parametrize("name", fc.SCENES)
def test_every_intermediate_call_is_the_frame_so_far(name, tall, context):
    t, rs = tall(name), context(name)
    w, h, counts, mb = fc.PREFIX
    film = rs.context.film(w, h)
    for flags, counting in fc.RENDER_MODES.values():
        _split(t, rs, film, w, h, counts, mb, flags, counting, every=True)
    film.close()


@pytest.mark.parametrize("name", fc.SCENES)
def test_passes_inside_a_continuing_call(name, tall, context):
    """Base 1000, then 3096 samples as passes of 1000, 1000, 1000 and 96: each
    call launches what a fresh context's render of its own count launches."""
    t, rs = tall(name), context(name)
    w, h, counts, mb, spp_pass = fc.PASSES
    cam = camera_for(t.soup, None, w, h)
    fresh = _scene(t)
    want = [fresh.render(cam, num_samples=n, max_bounce=mb, seed=t.seed, samples_per_pass=p)[1]["stats"]["trace_launches"]
            for n, p in zip(counts, (0, spp_pass))]
    fresh.close()
    assert want == [mb, 4 * mb]
    film = rs.context.film(w, h)
    pix = native.tile_pixels(w, h)
    tot, done = {}, 0
    for n, p, launches in zip(counts, (0, spp_pass), want):
        res = rs.context.accumulate(film, cam, n, mb, seed=t.seed, packed=True, linear=True, samples_per_pass=p)
        done += n
        _same(t, w, h, done, mb, res, pix, (name, done))
        assert res["stats"]["trace_launches"] == launches and rs.context.profile()["passes"] == launches // mb
        _add(tot, res["stats"])
    _totals(t, w, h, done, mb, tot, False, name)
    # the other modes, and the split of the first call too
    for flags, counting in list(fc.RENDER_MODES.values())[1:]:
        _split(t, rs, film, w, h, counts, mb, flags, counting, every=True, samples_per_pass=spp_pass)
    film.close()


@pytest.mark.parametrize("name", fc.SCENES)
def test_two_pass_sets_with_a_base(name, tall, context):
    """The second call is 2^23 samples or more by itself: two pass sets with a
    lead, and its first resolve reads the film."""
    t, rs = tall(name), context(name)
    w, h, counts, mb = fc.SETS
    film = rs.context.film(w, h)
    st = _split(t, rs, film, w, h, counts, mb)
    assert st[0]["trace_launches"] == mb and st[1]["trace_launches"] == 2 * mb
    prof = rs.context.profile()
    assert prof["sets"] == 2 and prof["passes"] == 2
    film.close()


@pytest.mark.parametrize("name", fc.SCENES)
def test_ranks_each_with_a_film(name, tall, context):
    t, rs = tall(name), context(name)
    w, h, counts, mb, tile, nranks = fc.RANKS
    cam = camera_for(t.soup, None, w, h)
    films = [rs.context.film(w, h, tile, r, nranks) for r in range(nranks)]
    pixs = [native.tile_pixels(w, h, tile, r, nranks) for r in range(nranks)]
    assert [f.n_owned for f in films] == [p.size for p in pixs] and sum(p.size for p in pixs) == w * h
    tot, done = {}, 0
    for n in counts:                      # the ranks take turns call by call: three films of one context
        done += n
        img = np.full((h, w, 3), 0x5A, np.uint8)
        for f, pix in zip(films, pixs):
            res = rs.context.accumulate(f, cam, n, mb, seed=t.seed, image=img, packed=True, linear=True)
            _same(t, w, h, done, mb, res, pix, (name, f.rank, done))
            _add(tot, res["stats"])
        assert np.array_equal(img.reshape(-1, 3), t.frame(w, h, done, mb)[0]), (name, done)
    _totals(t, w, h, done, mb, tot, False, name)
    # a rank that owns no tile: accepted, and its sample count still advances
    empty = rs.context.film(w, h, tile, 4, 5)
    assert empty.info() == (0, 0)
    res = rs.context.accumulate(empty, cam, 3, mb, seed=t.seed, packed=True, linear=True)
    assert empty.info() == (0, 3) and res["stats"]["samples"] == 0 and res["packed"].shape == (0, 3)
    assert empty.read()[1] == 3
    for f in films + [empty]:
        f.close()


@pytest.mark.parametrize("name", fc.SCENES)
def test_a_film_is_isolated_from_the_context(name, tall, context):
    """Between a film's two calls the context renders a frame of several
    passes (which uses its own accumulator), traces, takes feature planes and
    serves a second film; the second call writes RGB8 into device memory."""
    assert torch is not None
    t, rs = tall(name), context(name)
    w, h, counts, mb = fc.ISOLATION
    cam = camera_for(t.soup, None, w, h)
    film = rs.context.film(w, h)
    rs.context.accumulate(film, cam, counts[0], mb, seed=t.seed)                  # no outputs at all
    assert film.info() == (w * h, counts[0])
    before = film.read()

    rw, rh, rspp, rmb, rpass = fc.ISOLATION_RENDER
    rcam = camera_for(t.soup, None, rw, rh)
    img, out = rs.render(rcam, num_samples=rspp, max_bounce=rmb, seed=t.seed, linear=True, samples_per_pass=rpass)
    assert rs.context.profile()["passes"] == rspp // rpass > 1
    assert np.array_equal(img.reshape(-1, 3), t.frame(rw, rh, rspp, rmb)[0])
    rs.trace(t.o[:65], t.d[:65])
    rs.features(rcam, 3, seed=t.seed)
    other = rs.context.film(rw, rh)
    res = rs.context.accumulate(other, rcam, rspp, rmb, seed=t.seed, packed=True, linear=True)
    _same(t, rw, rh, rspp, rmb, res, native.tile_pixels(rw, rh), name)
    after = film.read()
    assert after[1] == before[1] and np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32))

    guard, nb = 64, 3 * w * h
    buf = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    res = rs.context.accumulate(film, cam, counts[1], mb, seed=t.seed, linear=True, device_ptr=buf.data_ptr() + guard)
    got = buf.cpu().numpy()
    pix = native.tile_pixels(w, h)
    rgb, bits, _ = t.frame(w, h, sum(counts), mb)
    assert np.array_equal(got[guard:guard + nb].reshape(-1, 3), rgb[pix])
    assert (got[:guard] == 0xA5).all() and (got[guard + nb:] == 0xA5).all()
    assert np.array_equal(res["linear"].view(np.uint32), bits[pix])
    other.close()
    film.close()


@pytest.mark.parametrize("name", fc.SCENES)
def test_checkpoint_and_resume(name, tall, context):
    t, rs = tall(name), context(name)
    w, h, counts, mb = fc.CHECKPOINT
    total = sum(counts)
    cam = camera_for(t.soup, None, w, h)
    pix = native.tile_pixels(w, h)
    film = rs.context.film(w, h)
    assert not film.read()[0].view(np.uint32).any()                # an empty film reads as +0
    rs.context.accumulate(film, cam, counts[0], mb, seed=t.seed)
    sums, s = film.read()
    assert s == counts[0] and sums.shape == (w * h, 3)
    # the sums as stored: times the f32 reciprocal they are the oracle's linear frame, bit for bit
    lin = sums * (np.float32(1.0) / np.float32(s))
    assert lin.dtype == np.float32 and np.array_equal(lin.view(np.uint32), t.frame(w, h, s, mb)[1][pix])

    fresh = _scene(t)                                                # resume in another context
    f2 = fresh.context.film(w, h)
    f2.write(sums, s)
    assert f2.info() == (w * h, s)
    res = fresh.context.accumulate(f2, cam, counts[1], mb, seed=t.seed, packed=True, linear=True)
    _same(t, w, h, total, mb, res, pix, (name, "resumed"))
    f2.close()
    fresh.close()

    # a reset film starts from +0 whatever its sums hold
    film.write(np.full((w * h, 3), np.nan, np.float32), 5)
    assert film.info()[1] == 5 and np.isnan(film.read()[0]).all()
    film.reset()
    assert film.info()[1] == 0
    res = rs.context.accumulate(film, cam, total, mb, seed=t.seed, packed=True, linear=True)
    _same(t, w, h, total, mb, res, pix, (name, "after NaN"))
    film.write(np.full((w * h, 3), np.nan, np.float32), 0)         # samples 0: a reset, too
    res = rs.context.accumulate(film, cam, total, mb, seed=t.seed, packed=True, linear=True)
    _same(t, w, h, total, mb, res, pix, (name, "after write 0"))
    film.close()


def _raw(ctx, film, cam, n, mb, seed, outs, tile=64, rank=0, num_ranks=2):
    cfg = native.RenderConfig()
    cfg.num_samples, cfg.max_bounce, cfg.seed, cfg.device = n, mb, seed, -1
    cfg.tile_size, cfg.rank, cfg.num_ranks = tile, rank, num_ranks
    st = native.Stats()
    return native.lib().zrt_context_accumulate(ctx._h, film._h, C.byref(cam), C.byref(cfg), C.byref(outs), C.byref(st))


def test_refusals_leave_film_and_outputs_untouched(tall, context):
    t, rs, rs2 = tall("cornell"), context("cornell"), context("fuzz")
    w, h, mb, base = 3, 3, 4, 17
    cam = camera_for(t.soup, None, w, h)
    film = rs.context.film(w, h, 64, 0, 2)               # rank 0 of 2 owns the one tile
    assert film.n_owned == w * h
    foreign = rs2.context.film(w, h, 64, 0, 2)
    rs.context.accumulate(film, cam, base, mb, seed=t.seed)
    sums = film.read()[0].copy()

    img = np.full((h, w, 3), 0xC3, np.uint8)
    packed = np.full((w * h, 3), 0xC3, np.uint8)
    lin = np.full((w * h, 3), -7.0, np.float32)
    outs = native.Outputs(img.ctypes.data, packed.ctypes.data, lin.ctypes.data, None)

    def untouched(what):
        assert film.info() == (w * h, base), what
        got, s = film.read()
        assert s == base and np.array_equal(got.view(np.uint32), sums.view(np.uint32)), what
        assert (img == 0xC3).all() and (packed == 0xC3).all() and (lin == -7.0).all(), what

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
    }
    for what, (f, c, kw) in refused.items():
        args = dict(n=1, mb=mb, seed=t.seed, outs=outs)
        args.update(kw)
        assert _raw(ctx, f, c, **args) == -1, what
        untouched(what)
    assert foreign.info() == (w * h, 0)
    assert _raw(ctx, film, cam, 1, 33, t.seed, outs) == -5             # ZRT_ERR_UNSUPPORTED
    untouched("max_bounce 33")
    assert native.lib().zrt_film_write(film._h, sums.ctypes.data, 65536) == -1
    untouched("write 65536")
    # the control: the same call with nothing wrong goes through (tile 0 = 64)
    assert _raw(ctx, film, cam, 65535 - base, mb, t.seed, outs, tile=0) == 0
    assert film.info() == (w * h, 65535) and not (packed == 0xC3).all()
    rgb, bits, _ = t.frame(w, h, 65535, mb)
    pix = native.tile_pixels(w, h)
    assert np.array_equal(packed, rgb[pix]) and np.array_equal(lin.view(np.uint32), bits[pix])
    assert np.array_equal(img.reshape(-1, 3), rgb)
    assert _raw(ctx, film, cam, 1, mb, t.seed, outs) == -1             # full: sample 65535 has no key
    film.close()
    foreign.close()
