"""Films (zrt_film_*, zrt_context_accumulate), the part that runs without a GPU:
the C ABI and its Python binding exist, and the oracle alone shows that the
cases of test_film_gpu.py prove something -- every frame hits geometry and
scatters, and the frame after each call of the prefix case differs from the
frame after the call before, so a film that ignored its base could not pass.
"""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native

import film_cases as fc

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
SYMBOLS = ("zrt_film_create", "zrt_film_reset", "zrt_film_info", "zrt_film_read", "zrt_film_write",
           "zrt_film_destroy", "zrt_context_accumulate")


def test_film_symbols_are_declared_exported_and_bound():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    L = native.lib()
    for s in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
        assert s in native.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert re.search(r"typedef struct zrt_film zrt_film;", hdr)
    assert re.search(r"\bint\s+zrt_context_accumulate\s*\(\s*zrt_context\s*\*\s*\w*\s*,\s*zrt_film\s*\*\s*\w*\s*,"
                     r"\s*const\s+zrt_camera\s*\*\s*\w*\s*,\s*const\s+zrt_render_config\s*\*\s*\w*\s*,"
                     r"\s*const\s+zrt_outputs\s*\*\s*\w*\s*,\s*zrt_stats\s*\*\s*\w*\s*\)", hdr)
    assert L.zrt_abi_version() == 2                     # added, not a new ABI
    assert L.zrt_film_destroy.restype is None
    assert len(L.zrt_film_create.argtypes) == 7 and len(L.zrt_context_accumulate.argtypes) == 6
    assert L.zrt_context_accumulate.argtypes[2:] == L.zrt_context_render.argtypes[1:]


def test_film_python_interface():
    for m in ("reset", "info", "read", "write", "close"):
        assert callable(getattr(native.Film, m)), m
    acc = inspect.signature(native.Context.accumulate).parameters
    ren = inspect.signature(native.Context.render).parameters
    for p in ("film", "cam", "spp", "max_bounce", "seed", "flags", "samples_per_pass", "want_linear", "stats"):
        assert p in acc, p
    # mirrors render, but for what the film fixes
    assert set(ren) - set(acc) == {"rank", "num_ranks", "tile"}


def test_null_arguments_are_refused_without_a_device():
    L = native.lib()
    cam, cfg, h = native.Camera(), native.RenderConfig(), C.c_void_p()
    cfg.num_samples = 1
    assert L.zrt_context_accumulate(None, None, C.byref(cam), C.byref(cfg), None, None) == -1
    assert L.zrt_film_create(None, 3, 3, 0, 0, 1, C.byref(h)) == -1 and not h.value
    assert L.zrt_film_reset(None) == -1 and L.zrt_film_info(None, None, None) == -1
    assert L.zrt_film_read(None, None, None) == -1 and L.zrt_film_write(None, None, 0) == -1
    L.zrt_film_destroy(None)


def test_the_cases_are_the_ones_asked_for():
    assert fc.FRAMES == ((1, 1), (3, 3), (13, 5))
    for total, splits in fc.SPLITS.items():
        assert all(sum(s) == total and min(s) >= 1 for s in splits), total
    assert (1,) * 64 in fc.SPLITS[64] and (15, 17, 32) in fc.SPLITS[64]
    w, h, counts, _ = fc.SETS
    assert w * h * counts[1] >= fc.BIG > w * h * counts[0] and sum(counts) == 65535
    assert set(fc.RENDER_MODES) == {"default", "lane_walk", "mt_exact", "counting"}
    w, h, _, _, tile, nranks = fc.RANKS
    assert -(-w // tile) * -(-h // tile) > nranks      # a rank with two tiles
    assert fc.PASSES[2][1] % fc.PASSES[4] == 96


@pytest.mark.parametrize("name", fc.SCENES)
def test_film_cases_hit_and_scatter(name, oracle_mod):
    t = fc.tall_scene(oracle_mod, name)
    for w, h, spp, mb in fc.oracle_frames():
        _, bits, ctr = t.frame(w, h, spp, mb)
        if mb == 0:
            assert int(ctr[0]) == 0 and not bits.any()
            continue
        fc._scatters(ctr, w * h * spp, mb)


@pytest.mark.parametrize("name", fc.SCENES)
def test_the_prefix_frames_differ(name, oracle_mod):
    """The frames after 15, 32 and 64 samples are three different images, linear
    and RGB8, and the later ones traced more segments."""
    t = fc.tall_scene(oracle_mod, name)
    w, h, counts, mb = fc.PREFIX
    fr = [t.frame(w, h, s, mb) for s in fc.prefixes(counts)]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not np.array_equal(fr[a][1], fr[b][1]), (a, b)
        assert not np.array_equal(fr[a][0], fr[b][0]), (a, b)
        assert int(fr[a][2][0]) < int(fr[b][2][0]), (a, b)
