"""Transmittance queries (zrt_context_transmittance), the part that runs
without a GPU: the C ABI's declarations and exports, the batch's layout, the
argument errors that come back before any device work, and the per-ray
reference (transmit_ref.py) -- on a hand-derived stack and counted for what
the fuzz rays reach.

The hand-derived stack: three quads in the planes z = 1, 2, 3 over
[-1, 1]^2, materials with 1x1 alpha textures 1/4, 1/2 and 1, and the ray
o = (1/4, 1/2, 0), d = (0, 0, 1) (off the quads' diagonals).  The first
crossing is at t = 1 with p = 3/4, the second at z = 2 with p = 1/2, the third
is opaque: T = 3/4, then 3/8, then 0, every product exact.  The chain continues
from z = 1 + 2^-23 with the bound shortened by the same 1 + 2^-23, so the second
segment's t is 1 - 2^-23 (exact), and a bound t_max = 2 leaves exactly that as
the second segment's bound: the strict keep test (`nearest > t`) drops the
crossing, as t_max = 1 drops the first.
"""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

import test_query_fuzz_gpu as qf
import trace_ref
import transmit_ref

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
F = np.float32


def test_header_declares_the_transmittance_query_and_native_exports_it():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\bint\s+zrt_context_transmittance\s*\(\s*zrt_context\s*\*\s*\w*\s*,"
                     r"\s*const\s+zrt_transmittance_batch\s*\*", hdr)
    assert re.search(r"typedef\s+struct\s+zrt_transmittance_batch\s*\{", hdr)
    assert "stage3.zig:207-212" in hdr
    assert "zrt_context_transmittance" in native.EXPORTS
    assert hasattr(native.lib(), "zrt_context_transmittance")
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and native.lib().zrt_abi_version() == 2


def test_transmittance_batch_layout():
    tb = native.TransmittanceBatch
    assert C.sizeof(tb) == 56
    assert [tb.num_rays.offset, tb.rays.offset, tb.t_max.offset, tb.transmittance.offset, tb.crossings.offset,
            tb.on_device.offset, tb.flags.offset, tb.t_max_all.offset, tb.max_crossings.offset] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52]
    hdr = open(f"{ROOT}/include/zrt.h").read()
    body = re.search(r"typedef\s+struct\s+zrt_transmittance_batch\s*\{(.*?)\}\s*zrt_transmittance_batch\s*;", hdr,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]
    assert names == [n for n, _ in tb._fields_]


def test_transmittance_rejects_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included),
    and the outputs stay as they were."""
    L = native.lib()
    assert L.zrt_context_transmittance(None, None, None) == -1
    rays = np.zeros(6, np.float32)
    T = np.full(1, 0xABABABAB, np.uint32)
    cr = np.full(1, 0xCDCDCDCD, np.uint32)
    r, t, c = rays.ctypes.data, T.ctypes.data, cr.ctypes.data
    inf = float("inf")
    TB = native.TransmittanceBatch
    for batch in (TB(0, None, None, None, None, 0, 0, inf, 16),
                  TB(1, r, None, t, c, 0, 0, inf, 16),                                  # a valid batch
                  TB(1, None, None, t, c, 0, 0, inf, 16),                               # null rays
                  TB(1, r, None, None, c, 0, 0, inf, 16),                               # null transmittance
                  TB(1, r, None, t, None, 0, native.FLAG_ONE_SET, inf, 16),             # a render-only flag
                  TB(1, r, None, t, None, 0, native.SEGMENT_ANY, inf, 16),              # another call's flags
                  TB(1, r, None, t, None, 0, native.RADIANCE_PER_SAMPLE, inf, 16),
                  TB(1, r, None, t, None, 0, 0x4, inf, 16),                             # a reserved render bit
                  TB(1, r, None, t, c, 2, 0, inf, 16),                                  # on_device > 1
                  TB(1, r, None, t, c, 0, 0, inf, 0),                                   # max_crossings 0
                  TB(1, r, None, t, c, 0, 0, inf, 257)):                                # ... above 256
        assert L.zrt_context_transmittance(None, C.byref(batch), None) == -1
    assert (T == 0xABABABAB).all() and (cr == 0xCDCDCDCD).all()


# ------------------------------------------------------- the hand-derived stack
def stack_soup():
    """Three quads at z = 1, 2, 3 with 1x1 alphas 1/4, 1/2, 1 (this file's docstring)."""
    s = scenes.get_scene("sphere")
    pos, mat = [], []
    for k, z in enumerate((1.0, 2.0, 3.0)):
        a, b, c, d = (-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)
        pos += [a + c + b, a + d + c]              # front faces towards -z: Moller-Trumbore culls det < 1e-8
        mat += [k, k]
    desc = np.zeros((3, 3, 7), np.int32)
    texels = []

    def push(vals):
        off = len(texels)
        texels.extend(vals)
        return (off, 1, 1, 0, 0, 0, 0)

    for k, alpha in enumerate((0.25, 0.5, 1.0)):
        desc[k, 0] = push([0.5, 0.5, 0.5])
        desc[k, 1] = push([0.0, 0.0, 0.0])
        desc[k, 2] = push([alpha])
    n = len(pos)
    return dataclasses.replace(
        s, name="alpha_stack", pos=np.asarray(pos, np.float32),
        nrm=np.tile(np.asarray([0, 0, 1] * 3, np.float32), (n, 1)), uv=np.zeros((n, 6), np.float32),
        mat=np.asarray(mat, s.mat.dtype), materials=[scenes.Material() for _ in range(3)], textures=[],
        tex_desc=desc, texels=np.asarray(texels, np.float32))


STACK_O, STACK_D = [0.25, 0.5, 0.0], [0.0, 0.0, 1.0]


@pytest.fixture(scope="module")
def stack(oracle_mod):
    soup = stack_soup()
    return trace_ref.RayRef(oracle_mod, soup, (2, 2, 2)), soup


def _stack(stack, t_max, cap):
    ref, soup = stack
    T, n, segs, _, _, end = transmit_ref.chain(ref, soup, STACK_O, STACK_D, t_max, cap).cut(cap)
    return float(T), n, segs, end


def test_hand_derived_stack(stack):
    ref, soup = stack
    full = transmit_ref.chain(ref, soup, STACK_O, STACK_D, np.inf, 16)
    assert [float(x) for x in full.T_after] == [0.75, 0.375, 0.0] and full.end == "blocked"
    assert full.at[0] == 1.0
    # as the bound moves past each quad
    assert _stack(stack, 0.5, 16) == (1.0, 0, 1, "miss")
    assert _stack(stack, 1.5, 16) == (0.75, 1, 2, "miss")
    assert _stack(stack, 2.5, 16) == (0.375, 2, 3, "miss")
    assert _stack(stack, 3.5, 16) == (0.0, 3, 3, "blocked")
    assert _stack(stack, np.inf, 16) == (0.0, 3, 3, "blocked")
    # a bound equal to a crossing's t does not count that crossing
    assert _stack(stack, 1.0, 16) == (1.0, 0, 1, "miss")
    assert _stack(stack, np.nextafter(F(1.0), F(2.0)), 16) == (0.75, 1, 2, "miss")
    assert _stack(stack, 2.0, 16) == (0.75, 1, 2, "miss")           # the second segment: t = bound = 1 - 2^-23
    # no ray at all for a bound that is not positive, or NaN
    for t_max in (0.0, -1.0, -np.inf, np.nan):
        assert _stack(stack, t_max, 16) == (1.0, 0, 1, "miss")
    # the cap stops after one and two crossings; the product so far stands
    assert _stack(stack, np.inf, 1) == (0.75, 1, 1, "cap")
    assert _stack(stack, np.inf, 2) == (0.375, 2, 2, "cap")
    assert _stack(stack, np.inf, 3) == (0.0, 3, 3, "blocked")
    # ... and a chain cut from a longer one answers the same
    assert full.cut(1)[:3] == (F(0.75), 1, 1) and full.cut(2)[:3] == (F(0.375), 2, 2)


# ------------------------------------------------ the fuzz rays: what they reach
@pytest.fixture(scope="module")
def case(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed]
    return get


def test_the_fuzz_rays_reach_what_the_chain_has_to_get_right(case):
    """Counted from the reference alone: seeds 0..39, t_max = +inf, cap 16."""
    n = dict.fromkeys(("two_or_more", "between", "cap3_differs", "at_cap", "blocked", "miss"), 0)
    for seed in qf.SEEDS:
        cs = case(seed)
        for c in transmit_ref.cached_chains(cs):
            T, k, _, _, _, end = c.cut(transmit_ref.CAP)
            n["two_or_more"] += k >= 2
            n["between"] += bool(0 < T < 1)
            n["cap3_differs"] += (F(c.cut(3)[0]).view(np.uint32), c.cut(3)[1]) != (F(T).view(np.uint32), k)
            n["at_cap"] += k == transmit_ref.CAP
            n["blocked"] += end == "blocked"
            n["miss"] += end == "miss"
    print(n)
    assert n["two_or_more"] >= 200 and n["between"] >= 200 and n["cap3_differs"] >= 50 and n["at_cap"] >= 1, n
    assert n["blocked"] >= 1 and n["miss"] >= 1, n
