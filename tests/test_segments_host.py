"""Segment queries (zrt_context_segments), the part that runs without a GPU:
the C ABI's declarations and exports, the batch's layout, the argument errors
that come back before any device work, and the bounded per-ray reference
(segment_ref.py) on hand-derived cases.

The triangle is test_trace_host.py's: from o = (0, 0, 2) along d = (0, 0, -1)
it is hit at t = 3/2, u = 1/4, v = 1/2, every value exact in f32.  A bound is
the initial nearest (stage3.zig:154) and the keep test is strict
(`nearest > t`), so t_max = 3/2 cuts the hit off and the next float above keeps
it, bit-equal to the unbounded one.
"""
import ctypes as C
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native

import segment_ref
import trace_ref
from test_trace_host import TRI, _soup

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
INF_BITS = 0x7F800000
O, D = [0, 0, 2], [0, 0, -1]
MISS_REC = ((np.float32(np.inf), np.float32(0), np.float32(0)), trace_ref.MISS)


def test_header_declares_the_segment_query_and_native_exports_it():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\bint\s+zrt_context_segments\s*\(\s*zrt_context\s*\*\s*\w*\s*,\s*const\s+zrt_segment_batch\s*\*", hdr)
    assert re.search(r"typedef\s+struct\s+zrt_segment_batch\s*\{", hdr)
    assert "stage3.zig:152-186" in hdr and "stage3.zig:154" in hdr
    assert "zrt_context_segments" in native.EXPORTS
    assert hasattr(native.lib(), "zrt_context_segments")
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and native.lib().zrt_abi_version() == 2


def test_the_any_flag_is_a_bit_of_its_own():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    m = re.search(r"#define\s+ZRT_SEGMENT_ANY\s+(0x[0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == native.SEGMENT_ANY
    assert bin(native.SEGMENT_ANY).count("1") == 1
    others = {n: int(v, 16) for n, v in
              re.findall(r"#define\s+(ZRT_FLAG_[A-Z_]+|ZRT_TRACE_PARK|ZRT_RADIANCE_PER_SAMPLE)\s+(0x[0-9a-fA-F]+)u", hdr)}
    assert "ZRT_TRACE_PARK" in others and "ZRT_RADIANCE_PER_SAMPLE" in others and len(others) >= 15
    assert all(native.SEGMENT_ANY & v == 0 for v in others.values()), others
    assert native.SEGMENT_ANY & (0x4 | 0x8) == 0            # the reserved render bits


def test_segment_batch_layout():
    sb = native.SegmentBatch
    assert C.sizeof(sb) == 56
    assert [sb.num_rays.offset, sb.rays.offset, sb.t_max.offset, sb.hits.offset, sb.occluded.offset,
            sb.on_device.offset, sb.flags.offset, sb.t_max_all.offset, sb._reserved.offset] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52]
    hdr = open(f"{ROOT}/include/zrt.h").read()
    body = re.search(r"typedef\s+struct\s+zrt_segment_batch\s*\{(.*?)\}\s*zrt_segment_batch\s*;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]
    assert names == [n for n, _ in sb._fields_]


def test_segments_rejects_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included)."""
    L = native.lib()
    assert L.zrt_context_segments(None, None, None) == -1
    rays = np.zeros(6, np.float32)
    hits = np.zeros(4, np.uint32)
    occ = np.zeros(1, np.uint8)
    r, h, o = rays.ctypes.data, hits.ctypes.data, occ.ctypes.data
    inf = float("inf")
    for batch in (native.SegmentBatch(0, None, None, None, None, 0, 0, inf, 0),
                  native.SegmentBatch(1, r, None, h, o, 0, 0, inf, 0),                      # a valid batch
                  native.SegmentBatch(1, None, None, h, None, 0, 0, inf, 0),                # null rays
                  native.SegmentBatch(1, r, None, None, None, 0, 0, inf, 0),                # both outputs null
                  native.SegmentBatch(1, r, None, h, o, 0, native.SEGMENT_ANY, inf, 0),     # any mode with hits
                  native.SegmentBatch(1, r, None, None, None, 0, native.SEGMENT_ANY, inf, 0),   # ... without bytes
                  native.SegmentBatch(1, r, None, h, None, 0, 0, inf, 7),                   # _reserved
                  native.SegmentBatch(1, r, None, h, None, 0, native.FLAG_ONE_SET, inf, 0),
                  native.SegmentBatch(1, r, None, h, None, 0, native.RADIANCE_PER_SAMPLE, inf, 0)):
        assert L.zrt_context_segments(None, C.byref(batch), None) == -1
    assert (hits == 0).all() and (occ == 0).all()


@pytest.fixture(scope="module")
def one(oracle_mod):
    return trace_ref.RayRef(oracle_mod, _soup([TRI]), (2, 2, 2))


def _both(ref, o, d, t_max):
    """The closest-mode record; any mode must agree with it on hit / miss and,
    on a hit in its stopping cell, need not hold the same record."""
    best, r, cells, tests = segment_ref.segment(ref, o, d, t_max)
    _, ra, cells_a, tests_a = segment_ref.segment(ref, o, d, t_max, any_hit=True)
    assert (ra != trace_ref.MISS) == (r != trace_ref.MISS)
    assert cells_a <= cells and tests_a <= tests
    return best, r


def test_a_bound_at_the_hit_cuts_it_off(one):
    (t, u, v), ref = _both(one, O, D, 1.5)
    assert np.float32(t).view(np.uint32) == INF_BITS and (float(u), float(v)) == (0.0, 0.0) and ref == trace_ref.MISS


def test_the_next_float_above_the_hit_keeps_it_bit_for_bit(one):
    free = one.trace(O, D)
    (t, u, v), ref = _both(one, O, D, np.nextafter(np.float32(1.5), np.float32(np.inf)))
    assert (float(t), float(u), float(v)) == (1.5, 0.25, 0.5)
    assert [np.float32(x).view(np.uint32) for x in (t, u, v)] == [np.float32(x).view(np.uint32) for x in free[0]]
    assert ref == free[1] and one.indices[ref] == 0


@pytest.mark.parametrize("t_max", [1.0, 0.0, -1.0, float("nan"), -0.0, float("-inf")])
def test_short_zero_negative_and_nan_bounds_miss(one, t_max):
    (t, u, v), ref = _both(one, O, D, t_max)
    assert np.float32(t).view(np.uint32) == INF_BITS and (float(u), float(v)) == (0.0, 0.0) and ref == trace_ref.MISS
    # the first cell is always tested, and a NaN bound walks to the grid's exit
    _, _, cells, _ = segment_ref.segment(one, O, D, t_max)
    assert cells >= 1
    if t_max != t_max:
        walk = one.orc.grid_trace(one.bmin, one.bmax, one.res, np.float32(O), np.float32(D), one.max_steps)
        assert cells == len(walk[2]) >= 2


def test_an_infinite_bound_is_the_unbounded_trace(one):
    for o, d in ((O, D), ([0, 0, -2], [0, 0, 1]), ([5, 5, 2], [0, 0, -1]), ([0, 0, 0.75], [0, 0, -1]),
                 ([0, 0, 2], [0, 0, -4]), ([0.3, -0.2, 3], [-0.1, 0.05, -1])):
        assert segment_ref.segment(one, o, d, np.inf) == one.trace(o, d)
        _both(one, o, d, np.inf)


def test_bounds_are_in_the_rays_own_parameter(one):
    # d four times as long: the hit is at t = 3/8, and the bound scales with it
    assert _both(one, O, [0, 0, -4], 0.375)[1] == trace_ref.MISS
    (t, _, _), ref = _both(one, O, [0, 0, -4], 0.5)
    assert float(t) == 0.375 and ref != trace_ref.MISS


def test_coincident_triangles_lower_ref_wins_in_closest_mode(oracle_mod):
    two = trace_ref.RayRef(oracle_mod, _soup([TRI, TRI]), (2, 2, 2))
    (t, u, v), ref, _, tests = segment_ref.segment(two, O, D, 2.0)
    assert (float(t), float(u), float(v)) == (1.5, 0.25, 0.5)
    b, e = next((b, e) for b, e in two.cells if b <= ref < e)
    assert sorted(two.indices[b:e]) == [0, 1] and two.indices[ref] == 0 and ref == b and tests >= 2
    assert segment_ref.segment(two, O, D, 2.0, any_hit=True)[1] != trace_ref.MISS
    assert segment_ref.segment(two, O, D, 1.5)[1] == trace_ref.MISS


def test_reference_batch_packs_bits_counts_and_misses(one):
    o = np.array([O, O, [0, 0, -2], [5, 5, 2]], np.float32)
    d = np.array([D, D, [0, 0, 1], [0, 0, -1]], np.float32)
    bits, (cells, tests, hits), per_ray = segment_ref.segment_batch(one, o, d, np.array([2.0, 1.5, 9, 9], np.float32))
    assert bits[0, 0] == np.float32(1.5).view(np.uint32) and bits[0, 3] != trace_ref.MISS
    for k in (1, 2, 3):
        assert [int(x) for x in bits[k]] == [INF_BITS, 0, 0, trace_ref.MISS]
    assert hits == 1 and cells == per_ray.sum() and per_ray[3] == 0 and tests >= 3
    same, counts, _ = segment_ref.segment_batch(one, o, d, np.float32(np.inf))
    assert np.array_equal(same, one.trace_batch(o, d)[0]) and counts == one.trace_batch(o, d)[1]
