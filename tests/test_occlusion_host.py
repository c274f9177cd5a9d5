"""Occlusion queries (zrt_context_occlusion), the part that runs without a
GPU: the C ABI's declarations and exports, the batch's layout, the argument
errors that come back before any device work, and the per-ray reference
(occlusion_ref.py) -- on a hand-derived corner and counted for what the fuzz
rays reach.

The hand-derived corner: a floor quad in the plane z = 0 over [-4, 4]^2, facing
up, and a wall quad in the plane x = 1 over y in [-4, 4], z in [0, 4], facing
-x; every vertex normal is its quad's.  The ray o = (1/4, 1/2, 2), d = (0, 0, -1)
meets the floor at t = 2 and its position is (1/4, 1/2, 0) -- 2 + 2^-23 rounds
to 2 -- in the floor's own plane, which a direction with d.z >= 0 leaves without
a hit (t = 0 is not kept, and Moller-Trumbore culls the face from behind), so
only the wall can occlude.  A sample direction d_s = normalize((0, 0, 1) + unit
vector) has d_s.z >= 0 and meets the plane x = 1 at t = (3/4) / d_s.x when
d_s.x > 0, at y = 1/2 + t d_s.y and z = t d_s.z: occluded iff that point lies
on the wall and t is below the radius.
"""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

import occlusion_ref
import test_query_fuzz_gpu as qf
import trace_ref

ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
F = np.float32


def test_header_declares_the_occlusion_query_and_native_exports_it():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\bint\s+zrt_context_occlusion\s*\(\s*zrt_context\s*\*\s*\w*\s*,"
                     r"\s*const\s+zrt_occlusion_batch\s*\*", hdr)
    assert re.search(r"typedef\s+struct\s+zrt_occlusion_batch\s*\{", hdr)
    assert "stage3.zig:214" in hdr and "linalg.zig:140-148" in hdr and "cosine-weighted" in hdr
    assert "zrt_context_occlusion" in native.EXPORTS
    assert hasattr(native.lib(), "zrt_context_occlusion")
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and native.lib().zrt_abi_version() == 2
    for name in ("occlusion_raw", "occlusion"):
        assert callable(getattr(native.Context, name))
    from zig_raytracing_contest_amd import RenderScene
    assert callable(RenderScene.occlusion)


def test_occlusion_batch_layout():
    ob = native.OcclusionBatch
    assert C.sizeof(ob) == 80
    assert [ob.num_rays.offset, ob.rays.offset, ob.radius.offset, ob.visibility.offset, ob.occluded.offset,
            ob.hits.offset, ob.on_device.offset, ob.flags.offset, ob.radius_all.offset, ob.num_samples.offset,
            ob.seed.offset, ob.index_base.offset] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 72]
    hdr = open(f"{ROOT}/include/zrt.h").read()
    body = re.search(r"typedef\s+struct\s+zrt_occlusion_batch\s*\{(.*?)\}\s*zrt_occlusion_batch\s*;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]
    assert names == [n for n, _ in ob._fields_]


def test_occlusion_rejects_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included),
    and the outputs stay as they were."""
    L = native.lib()
    assert L.zrt_context_occlusion(None, None, None) == -1
    rays = np.zeros(6, np.float32)
    vis = np.full(1, 0xABABABAB, np.uint32)
    occ = np.full(1, 0xCDCDCDCD, np.uint32)
    hit = np.full(4, 0xEFEFEFEF, np.uint32)
    r, v, o, h = rays.ctypes.data, vis.ctypes.data, occ.ctypes.data, hit.ctypes.data
    inf = float("inf")
    OB = native.OcclusionBatch
    for batch in (OB(0, None, None, None, None, None, 0, 0, inf, 4, 0, 0),
                  OB(1, r, None, v, o, h, 0, 0, inf, 4, 0, 0),                                  # a valid batch
                  OB(1, None, None, v, o, h, 0, 0, inf, 4, 0, 0),                               # null rays
                  OB(1, r, None, None, None, h, 0, 0, inf, 4, 0, 0),                            # no output at all
                  OB(1, r, None, v, o, None, 0, native.FLAG_ONE_SET, inf, 4, 0, 0),             # a render-only flag
                  OB(1, r, None, v, o, None, 0, native.SEGMENT_ANY, inf, 4, 0, 0),              # another call's flags
                  OB(1, r, None, v, o, None, 0, native.RADIANCE_PER_SAMPLE, inf, 4, 0, 0),
                  OB(1, r, None, v, o, None, 0, 0x4, inf, 4, 0, 0),                             # a reserved render bit
                  OB(1, r, None, v, o, h, 2, 0, inf, 4, 0, 0),                                  # on_device > 1
                  OB(1, r, None, v, o, h, 0, 0, inf, 0, 0, 0),                                  # num_samples 0
                  OB(1, r, None, v, o, h, 0, 0, inf, 65536, 0, 0)):                             # ... above 65535
        assert L.zrt_context_occlusion(None, C.byref(batch), None) == -1
    assert (vis == 0xABABABAB).all() and (occ == 0xCDCDCDCD).all() and (hit == 0xEFEFEFEF).all()


# ------------------------------------------------------- the hand-derived corner
def corner_soup():
    """The floor and the wall of this file's docstring."""
    s = scenes.get_scene("sphere")
    fa, fb, fc, fd = (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)            # (b - a) x (c - a) = +z
    wa, wb, wc, wd = (1, -4, 0), (1, 4, 0), (1, 4, 4), (1, -4, 4)              # (c - a) x (b - a) = -x
    pos = [fa + fb + fc, fa + fc + fd, wa + wc + wb, wa + wd + wc]
    nrm = [[0, 0, 1] * 3] * 2 + [[-1, 0, 0] * 3] * 2
    desc = np.zeros((1, 3, 7), np.int32)
    desc[0, 0] = (0, 1, 1, 0, 0, 0, 0)
    desc[0, 1] = (3, 1, 1, 0, 0, 0, 0)
    desc[0, 2] = (6, 1, 1, 0, 0, 0, 0)
    return dataclasses.replace(
        s, name="corner", pos=np.asarray(pos, np.float32), nrm=np.asarray(nrm, np.float32),
        uv=np.zeros((4, 6), np.float32), mat=np.zeros(4, s.mat.dtype), materials=[scenes.Material()], textures=[],
        tex_desc=desc, texels=np.asarray([0.5, 0.5, 0.5, 0, 0, 0, 1.0], np.float32))


CORNER_O, CORNER_D, CORNER_S, CORNER_SEED, CORNER_KEY = [0.25, 0.5, 2.0], [0.0, 0.0, -1.0], 16, 11, 5


def corner_by_hand(orc, radius):
    """The occluded samples of the corner's ray, from the geometry: float64
    on the directions the reference draws; a sample within 1e-4 of an edge of
    the wall or of the radius would make the derivation doubtful: none is."""
    out = []
    for s in range(CORNER_S):
        d = occlusion_ref.direction(orc, [0, 0, 1], CORNER_SEED, CORNER_KEY, s).astype(np.float64)
        assert d[2] >= 0 and abs(float(np.linalg.norm(d)) - 1) < 1e-6
        if d[0] <= 0:
            out.append(False)
            continue
        t = 0.75 / d[0]
        y, z = 0.5 + t * d[1], t * d[2]
        assert min(abs(abs(y) - 4), abs(z), abs(z - 4), abs(t - radius)) > 1e-4, (s, t, y, z)
        out.append(bool(abs(y) < 4 and 0 < z < 4 and t < radius))
    return out


@pytest.fixture(scope="module")
def corner(oracle_mod):
    soup = corner_soup()
    return trace_ref.RayRef(oracle_mod, soup, (4, 4, 4)), soup


def test_hand_derived_corner(corner, oracle_mod):
    ref, soup = corner
    (t, u, v), r, _, _ = ref.trace(CORNER_O, CORNER_D)
    assert t == 2.0 and r != trace_ref.MISS
    bits = np.append(np.array([t, u, v], F).view(np.uint32), np.uint32(r))
    smp = occlusion_ref.ray_samples(ref, soup, CORNER_O, CORNER_D, bits, CORNER_SEED, CORNER_KEY, CORNER_S)
    assert len(smp) == CORNER_S and all(x.traced for x in smp)
    assert [float(x) for x in smp[0].pos] == [0.25, 0.5, 0.0]
    got = {}
    for radius in (1.5, np.inf):
        want = corner_by_hand(oracle_mod, radius)
        got[radius] = [x.occluded(ref, radius) for x in smp]
        assert got[radius] == want, (radius, got[radius], want)
    # the two radii tell samples apart, and neither is all or nothing
    assert 0 < sum(got[1.5]) < sum(got[np.inf]) < CORNER_S, got
    occ, vis, traced, _ = occlusion_ref.occlusion_batch(ref, [smp], 1.5, CORNER_S)
    assert occ[0] == sum(got[1.5]) and traced == CORNER_S
    assert vis.view(F)[0] == F(CORNER_S - int(occ[0])) / F(CORNER_S)
    # prefixes: the counts at fewer samples are the first samples'
    assert occlusion_ref.occlusion_batch(ref, [smp], np.inf, 3)[0][0] == sum(got[np.inf][:3])
    # never occluded: a radius that is not positive, or NaN; exactly a sample's t is not a hit, the next float is
    for radius in (0.0, -1.0, -np.inf, np.nan):
        assert not any(x.occluded(ref, radius) for x in smp)
    k = got[np.inf].index(True)
    t_k = smp[k].closest(ref, np.inf)[0][0]
    assert not smp[k].occluded(ref, t_k) and smp[k].occluded(ref, np.nextafter(t_k, F(np.inf)))


def test_untraced_samples_and_the_visibility_division():
    # a huge normal: the squared length overflows, the direction is +0; NaN and inf normals: NaN
    assert not occlusion_ref.is_traced(np.zeros(3, F), occlusion_ref.normalize([3e38, 0, 0]))
    assert (occlusion_ref.normalize([3e38, 1, 1]) == 0).all()
    assert np.isnan(occlusion_ref.normalize([np.inf, 0, 0])).any() and np.isnan(occlusion_ref.normalize([np.nan, 0, 0])).all()
    assert not occlusion_ref.is_traced(np.array([np.inf, 0, 0], F), np.array([0, 0, 1], F))
    # (S - 0) / S is exactly 1 for every S; S * (1 / S) is not
    S = np.arange(1, 65536, dtype=np.uint32)
    assert (occlusion_ref.visibility(np.zeros(1, np.uint32), 49) == 1).all()
    assert (S.astype(F) / S.astype(F) == 1).all()
    assert (S.astype(F) * (F(1) / S.astype(F)) != 1).any()


# ------------------------------------------------ the fuzz rays: what they reach
@pytest.fixture(scope="module")
def case(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed]
    return get


def test_the_fuzz_rays_reach_what_the_call_has_to_get_right(case):
    """Counted from the reference alone: seeds 0..39, all 128 rays, 5 samples,
    key = the ray's index, radius = 0.25 x the soup's diagonal."""
    S = occlusion_ref.S_MAX
    n = dict.fromkeys(("hits", "partly", "fully", "open", "untraced"), 0)
    for seed in qf.SEEDS:
        cs = case(seed)
        smp = occlusion_ref.cached_samples(cs)
        occ, _, traced, _ = occlusion_ref.occlusion_batch(cs.ref, smp, occlusion_ref.fuzz_radius(cs.soup), S)
        hit = np.array([len(x) > 0 for x in smp])
        n["hits"] += int(hit.sum())
        n["partly"] += int(((occ > 0) & (occ < S)).sum())
        n["fully"] += int((occ == S).sum())
        n["open"] += int((hit & (occ == 0)).sum())
        n["untraced"] += S * int(hit.sum()) - traced
    print(n)
    # counted: 1783 first hits, 704 partly occluded, 264 fully occluded, 815 open, no untraced sample;
    # the floors are half of that
    assert n["hits"] >= 891 and n["partly"] >= 352 and n["fully"] >= 132 and n["open"] >= 407, n
    assert n["hits"] == n["partly"] + n["fully"] + n["open"] and n["untraced"] == 0, n
