"""Adaptive films (zrt_context_refine, zrt_film_counts), the part that runs
without a GPU: the C ABI and its binding exist, the refusals that need no
device, and the oracle alone gives the sequences of active pixels the GPU
tests expect -- and shows that those cases prove something: pixels do freeze,
at different counts, on lists that are no multiple of a wave.
"""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native

import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zrt_context_refine", "zrt_film_counts")


def test_refine_symbols_are_declared_exported_and_bound():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    L = native.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert s in native.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert re.search(r"typedef struct zrt_refine_config\s*\{[^}]*uint32_t\s*\*\s*sample_counts;[^}]*float\s+threshold;"
                     r"[^}]*uint32_t\s+min_samples;[^}]*\}\s*zrt_refine_config;", hdr)
    assert L.zrt_abi_version() == 2                     # added, not a new ABI
    assert C.sizeof(native.RefineConfig) == 16
    assert [f[0] for f in native.RefineConfig._fields_] == ["sample_counts", "threshold", "min_samples"]
    assert len(L.zrt_context_refine.argtypes) == 8 and len(L.zrt_film_counts.argtypes) == 3
    acc = L.zrt_context_accumulate.argtypes
    assert L.zrt_context_refine.argtypes[:4] == acc[:4] and L.zrt_context_refine.argtypes[5:7] == acc[4:]


def test_refine_python_interface():
    assert callable(native.Film.counts)
    ref = inspect.signature(native.Context.refine).parameters
    acc = inspect.signature(native.Context.accumulate).parameters
    assert set(ref) - set(acc) == {"threshold", "min_samples", "counts"} and not set(acc) - set(ref)
    assert ref["min_samples"].default == 0 and ref["counts"].default is False
    assert list(ref)[:6] == ["self", "film", "cam", "spp", "max_bounce", "threshold"]


def test_null_and_nan_are_refused_without_a_device():
    L = native.lib()
    cam, cfg, rf = native.Camera(), native.RenderConfig(), native.RefineConfig()
    cfg.num_samples = 1
    fake = C.c_void_p(8)       # never dereferenced: the null checks come first
    assert L.zrt_context_refine(None, None, C.byref(cam), C.byref(cfg), C.byref(rf), None, None, None) == -1
    assert L.zrt_context_refine(fake, None, C.byref(cam), C.byref(cfg), C.byref(rf), None, None, None) == -1
    assert L.zrt_context_refine(None, fake, C.byref(cam), C.byref(cfg), C.byref(rf), None, None, None) == -1
    assert L.zrt_film_counts(None, None, None) == -1
    rf.threshold = math.nan
    assert L.zrt_context_refine(None, None, C.byref(cam), C.byref(cfg), C.byref(rf), None, None, None) == -1


def test_the_cases_are_the_ones_asked_for():
    assert len(rc.PARITY) == 10 and rc.SCHEDULE == (4, 4, 8, 16, 32) and rc.MB == 4
    assert set(rc.RENDER_MODES) == {"default", "lane_walk", "mt_exact", "counting"}
    assert {(k[1], k[2]) for k in rc.PARITY} == {(3, 3), (13, 5), (33, 31)}
    big = [k for k in rc.PARITY if k[3] == rc.BIG_SCHEDULE]
    assert len(big) == 1 and rc.PARITY[big[0]][3] * rc.BIG_SCHEDULE[3] >= rc.BIG and sum(rc.BIG_SCHEDULE[:3]) == 16
    assert rc.PARITY[rc.CONVERGED][-1] == 0
    assert rc.PASSES[3][-1] == 32 and -(-32 // rc.PASSES[6]) == 7


@pytest.mark.parametrize("case", list(rc.PARITY), ids=lambda k: "%s-%dx%d-%s-%g-%d" % (k[0], k[1], k[2], len(k[3]), k[4], k[5]))
def test_the_oracle_gives_the_active_sequences(case, oracle_mod):
    name, w, h, schedule, thr, min_s = case
    t = rc.tall_scene(oracle_mod, name)
    calls = rc.expect(t, w, h, schedule, thr, min_s)
    active = tuple(int(a.sum()) for _, a, _ in calls)
    assert active == rc.PARITY[case]
    # a frozen pixel stays frozen, at the samples the film held when it was
    for (b0, a0, n0), (b1, a1, n1) in zip(calls, calls[1:]):
        assert not (a1 & ~a0).any() and np.array_equal(n1[~a0], n0[~a0]) and (n1[~a1 & a0] == b1).all()
    if case == rc.CONVERGED:
        assert calls[-1][0] == calls[-2][0] + schedule[-2] and (calls[-1][2] <= calls[-1][0]).all()
        return
    # the condition: without it a test could pass with nothing ever frozen
    P = w * h
    assert any(0 < a < P and a % 64 for a in active), active
    assert np.unique(calls[-1][2]).size >= 3, np.unique(calls[-1][2])


@pytest.mark.parametrize("name", rc.SCENES)
def test_render_pixels_is_the_frame_per_subset(name, oracle_mod):
    """What the stats reference rests on: the oracle's pixel subsets are the
    frame's pixels, and their counters are those of the subset alone."""
    t = rc.tall_scene(oracle_mod, name)
    w, h, N = 13, 5, 8
    rgb, bits, ctr = t.frame(w, h, N, rc.MB)
    odd = np.arange(1, w * h, 2, dtype=np.uint32)
    even = np.arange(0, w * h, 2, dtype=np.uint32)
    got = [t.oracle.render_pixels(t.ocam(w, h), N, rc.MB, p, t.orc.RNG_PATH, t.seed, rc.THREADS) for p in (odd, even)]
    for p, (r, l, _) in zip((odd, even), got):
        assert np.array_equal(r, rgb[p]) and np.array_equal(l.view(np.uint32), bits[p])
    assert np.array_equal(got[0][2][:4] + got[1][2][:4], ctr[:4])
    assert np.array_equal(rc.call_counters(t, w, h, 0, N, odd)[:4], got[0][2][:4])
