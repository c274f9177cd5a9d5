"""Light-probe queries (zrt_context_light_probes), the part that runs without a
GPU: the C ABI's declaration, constants and exports, the batch's layout, the
argument errors that come back before any device work, the per-probe reference
(light_probe_ref.py) against an analytic answer, and counts of what the GPU
cases (test_light_probes_gpu.py) reach.

The analytic answer: edge_scenes.one_triangle() on a 4^3 grid, one probe 50
above the triangle's centroid, S = 1, max_bounce = 1.  A path of one segment
returns the sky where it misses -- L = a + b y per channel with a = (1 + c) / 2,
b = (c - 1) / 2, c = (0.5, 0.7, 1.0) (stage3.zig:196-199: the blend of white
and c by (y + 1) / 2) -- and black where it hits.  With the real orthonormal
basis Y_0 = sqrt(1 / 4 pi), Y_1 = sqrt(3 / 4 pi) y the projection of a + b y
over the sphere is sh[0] = a sqrt(4 pi), sh[1] = b sqrt(4 pi / 3), the rest 0.
The estimate (4 pi / D) sum L_j Y_k(d_j) over D uniform directions has the
standard error se = std(4 pi L_j Y_k(d_j)) / sqrt(D), taken from the terms
themselves in float64.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native

import edge_scenes
import light_probe_ref as lpr
import test_light_probes_gpu as lpg

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
F = np.float32


def _fields(hdr, name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*(\[\d+\])?\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]


def test_header_declares_the_light_probe_query_and_native_exports_it():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\bint\s+zrt_context_light_probes\s*\(\s*zrt_context\s*\*\s*\w*\s*,"
                     r"\s*const\s+zrt_light_probe_batch\s*\*", hdr)
    assert "light-probe queries (ABI 2, added)" in hdr
    assert hdr.index("direct-light queries (ABI 2, added)") < hdr.index("light-probe queries (ABI 2, added)") < \
        hdr.index("typedef struct zrt_group zrt_group")
    for name, lit in (("C0", "0x1.20dd76p-2f"), ("C1", "0x1.f45438p-2f"), ("C2", "0x1.17b142p+0f"),
                      ("C3", "0x1.42f602p-2f"), ("C4", "0x1.17b142p-1f"), ("FOUR_PI", "0x1.921fb6p+3f")):
        pattern = "0x%08X" % lpr.SH_BITS[name]
        assert lit in hdr and pattern in hdr, name
        assert F(float.fromhex(lit[:-1])).view(np.uint32) == lpr.SH_BITS[name], name     # the two spellings agree
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and native.lib().zrt_abi_version() == 2
    assert "zrt_context_light_probes" in native.EXPORTS
    assert hasattr(native.lib(), "zrt_context_light_probes")
    for name in ("light_probes_raw", "light_probes"):
        assert callable(getattr(native.Context, name))
    from zig_raytracing_contest_amd import RenderScene
    assert callable(RenderScene.light_probes)


def test_the_constants_are_the_real_sh_normalisations():
    pi = math.pi
    for got, want in ((lpr.C0, 0.5 * math.sqrt(1 / pi)), (lpr.C1, math.sqrt(3 / (4 * pi))),
                      (lpr.C2, 0.5 * math.sqrt(15 / pi)), (lpr.C3, 0.25 * math.sqrt(5 / pi)),
                      (lpr.C4, 0.25 * math.sqrt(15 / pi)), (lpr.FOUR_PI, 4 * pi)):
        assert got == F(want), (got, want)
    assert [int(c.view(np.uint32)) for c in (lpr.C0, lpr.C1, lpr.C2, lpr.C3, lpr.C4, lpr.FOUR_PI)] == \
        [lpr.SH_BITS[k] for k in ("C0", "C1", "C2", "C3", "C4", "FOUR_PI")]


def test_batch_layout():
    lb = native.LightProbeBatch
    assert C.sizeof(lb) == 96
    names = [n for n, _ in lb._fields_]
    assert [getattr(lb, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80, 88]
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert _fields(hdr, "zrt_light_probe_batch") == names


def test_light_probes_reject_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included),
    and the outputs stay as they were."""
    L = native.lib()
    assert L.zrt_context_light_probes(None, None, None) == -1
    pos = np.zeros(3, F)
    outs = [np.full(32, 0xA0A0A0A0 + i, np.uint32) for i in range(5)]
    x = pos.ctypes.data
    s, d, h, w, r = (o.ctypes.data for o in outs)
    LB = native.LightProbeBatch
    for batch in (LB(0, None, None, None, None, None, None, 0, 0, 4, 1, 1, 0, 0, 0),
                  LB(1, x, s, d, h, w, r, 0, 0, 4, 1, 1, 0, 0, 0),                     # a valid batch
                  LB(1, None, s, d, h, w, r, 0, 0, 4, 1, 1, 0, 0, 0),                  # null positions
                  LB(1, x, None, None, None, None, None, 0, 0, 4, 1, 1, 0, 0, 0),      # no output at all
                  LB(1, x, s, d, h, w, r, 2, 0, 4, 1, 1, 0, 0, 0),                     # on_device > 1
                  LB(1, x, s, d, h, w, r, 0, 0, 4, 1, 1, 1, 0, 0),                     # _reserved
                  LB(1, x, s, d, h, w, r, 0, 0, 0, 1, 1, 0, 0, 0),                     # num_directions 0
                  LB(1, x, s, d, h, w, r, 0, 0, 65536, 1, 1, 0, 0, 0),                 # ... above 65535
                  LB(1, x, s, d, h, w, r, 0, 0, 4, 0, 1, 0, 0, 0),                     # num_samples 0
                  LB(1, x, s, d, h, w, r, 0, 0, 4, 65536, 1, 0, 0, 0),                 # ... above 65535
                  LB((1 << 47) + 1, x, s, d, h, w, r, 0, 0, 4, 1, 1, 0, 0, 0),         # num_probes above 2^47
                  LB(1, x, s, d, h, w, r, 0, 0, 4, 1, 0, 0, 0, 0),                     # max_bounce 0
                  LB(1, x, s, d, h, w, r, 0, 0, 4, 1, 33, 0, 0, 0),                    # (unsupported with a context)
                  LB(1, x, s, d, h, w, r, 0, native.RADIANCE_PER_SAMPLE, 4, 1, 1, 0, 0, 0),
                  LB(1, x, s, d, h, w, r, 0, native.FLAG_COUNT_STATS, 4, 1, 1, 0, 0, 0),
                  LB(1, x, s, d, h, w, r, 0, native.FLAG_ONE_SET, 4, 1, 1, 0, 0, 0),   # a render-only flag
                  LB(1, x, s, d, h, w, r, 0, native.SEGMENT_ANY, 4, 1, 1, 0, 0, 0),    # another call's flags
                  LB(1, x, s, d, h, w, r, 0, native.DIRECT_UNSHADOWED, 4, 1, 1, 0, 0, 0),
                  LB(1, x, s, d, h, w, r, 0, 0x4, 4, 1, 1, 0, 0, 0),                   # a reserved render bit
                  LB(1, x, s, d, h, w, r, 0, native.TRACE_PARK, 4, 1, 1, 0, 0, 0)):    # (valid: an accepted flag)
        assert L.zrt_context_light_probes(None, C.byref(batch), None) == -1
    for i, o in enumerate(outs):
        assert (o == 0xA0A0A0A0 + i).all()


# ----------------------------------------------------------- the analytic answer
def test_the_reference_projects_the_sky_onto_the_real_basis(oracle_mod):
    soup = edge_scenes.one_triangle()
    ref = lpr.LightProbeRef(oracle_mod, soup, (4, 4, 4))
    centroid = soup.pos.reshape(-1, 3).astype(np.float64).mean(0)
    D = 4096
    got = ref.probes([centroid + [0, 0, 50]], D, 1, 1, seed=9)
    L = got["radiance"][0].astype(np.float64)
    d = got["directions"][0].astype(np.float64)
    assert (L > 0).all(), "no ray is black"
    c = np.array([0.5, 0.7, 1.0])
    a, b = (1 + c) / 2, (c - 1) / 2
    assert np.abs(L - (a + b * d[:, 1:2])).max() < 1e-5                    # every ray sees the sky
    exact = np.zeros((9, 3))
    exact[0], exact[1] = a * math.sqrt(4 * math.pi), b * math.sqrt(4 * math.pi / 3)
    Y = np.array([lpr.basis(v) for v in got["directions"][0]], np.float64)  # (D, 9)
    terms = 4 * math.pi * L[:, None, :] * Y[:, :, None]                     # (D, 9, 3)
    se = terms.std(axis=0, ddof=1) / math.sqrt(D)
    dev = np.abs(got["sh"][0].astype(np.float64) - exact)
    print("largest deviation in se:", (dev / np.maximum(se, 1e-12))[se > 1e-9].max())
    assert (dev <= 6 * se + 1e-4).all(), (dev, se)
    # the restatement adds what it says it adds: float64 and float32 sums agree to rounding
    assert np.abs(terms.mean(axis=0) - got["sh"][0]).max() < 1e-3


def test_the_vector_fold_is_the_scalar_fold():
    rng = np.random.default_rng(5)
    n, D = 7, 33
    d = rng.normal(size=(n, D, 3)).astype(F)
    d /= np.linalg.norm(d, axis=2, keepdims=True).astype(F)
    lin = rng.random((n, D, 3)).astype(F)
    t = np.where(rng.random((n, D)) < 0.3, np.inf, rng.random((n, D)) * 9).astype(F)
    t[0] = np.inf
    lin[1, 3, 1] = np.nan
    sh, dist, hits = lpr.fold_batch(d, lin, t)
    assert sh.dtype == F and dist.dtype == F
    for p in range(n):
        a, b, c = lpr.fold(d[p], lin[p], t[p])
        assert np.array_equal(a.view(np.uint32), sh[p].view(np.uint32)) and c == hits[p]
        assert np.array_equal(b.view(np.uint32), dist[p].view(np.uint32))
    assert hits[0] == 0 and not dist[0].any() and 0 < hits[1:].min() and hits.max() < D
    assert np.isnan(sh[1, :, 1]).all() and not np.isnan(sh[1, :, 0]).any()


# ------------------------------------------------- what the GPU cases reach
@pytest.mark.parametrize("name", list(lpg.CASES))
def test_the_gpu_cases_are_not_degenerate(name, oracle_mod):
    cs = lpg.get_case(oracle_mod, name)
    assert cs.pos.shape == (lpg.N_IN + lpg.N_OUT, 3)
    w65 = cs.want(65, 1, 1)
    assert (w65["hits"] > 0).all(), w65["hits"]
    assert (w65["hits"] < 65).any(), w65["hits"]
    print(name, "hits at D = 65:", w65["hits"].tolist())
    w16 = cs.want(16, 3, 4)
    rows = {r.tobytes() for r in w16["sh"].reshape(len(cs.pos), -1)}
    assert len(rows) == len(cs.pos), "all sh rows are distinct"
    assert np.isfinite(w16["sh"]).all()
    assert w16["segments"] > w16["samples"] > 0
