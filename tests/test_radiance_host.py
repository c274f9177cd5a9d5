"""Radiance queries (zrt_context_radiance), the part that runs without a GPU:
the C ABI's declarations and exports, the batch's layout, the argument errors
that come back before any device work, and the per-ray reference
(radiance_ref.py) on two hand cases.

Hand case 1: a ray that misses every triangle ends in
traceRayRecursive's `return env_color(ray)` at its first segment
(stage3.zig:195-197) for every sample, so the pixel is the sum of spp equal
values v times 1 / spp.  For spp = 1 that is v itself (1 / 1 = 1), for
spp = 2 it is (v + v) * 0.5 = v exactly (a doubling and a halving), for any
spp it is the same f32 chain the test restates.
Hand case 2: max_bounce = 0 returns 0 from the depth test before any
traceRay call: zero radiance, RGB 0, no segment counted.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import native, scenes

import radiance_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_radiance_query_and_native_exports_it():
    hdr = open(f"{ROOT}/include/zrt.h").read()
    assert re.search(r"\bint\s+zrt_context_radiance\s*\(\s*zrt_context\s*\*", hdr)
    assert re.search(r"typedef\s+struct\s+zrt_radiance_batch\s*\{", hdr)
    assert "stage3.zig:188-220" in hdr and "stage3.zig:27-35" in hdr
    assert "zrt_context_radiance" in native.EXPORTS
    assert hasattr(native.lib(), "zrt_context_radiance")
    m = re.search(r"#define\s+ZRT_RADIANCE_PER_SAMPLE\s+(0x[0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == native.RADIANCE_PER_SAMPLE
    # a single bit that no render flag and not ZRT_TRACE_PARK uses
    bit = native.RADIANCE_PER_SAMPLE
    assert bit and bit & (bit - 1) == 0
    flags = [int(v, 16) for v in re.findall(r"#define ZRT_FLAG_[A-Z_]+\s+(0x[0-9a-fA-F]+)u", hdr)]
    assert len(flags) >= 10 and all(bit & f == 0 for f in flags)
    park = re.search(r"#define\s+ZRT_TRACE_PARK\s+(0x[0-9a-fA-F]+)u", hdr)
    assert park and int(park.group(1), 16) & bit == 0


def test_radiance_batch_layout_matches_the_header():
    rb = native.RadianceBatch
    assert C.sizeof(rb) == 64
    names = ["num_rays", "rays", "radiance", "rgb", "on_device", "flags", "num_samples", "max_bounce", "seed",
             "index_base"]
    assert [f for f, _ in rb._fields_] == names
    assert [getattr(rb, f).offset for f in names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 56]
    # the header's fields in the same order
    hdr = open(f"{ROOT}/include/zrt.h").read()
    body = re.search(r"typedef\s+struct\s+zrt_radiance_batch\s*\{(.*?)\}\s*zrt_radiance_batch\s*;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == names


def _batch(num_rays=1, rays=True, radiance=True, flags=0, spp=1, max_bounce=1):
    keep = [np.zeros(6, np.float32), np.zeros(3, np.float32)]
    b = native.RadianceBatch(num_rays, keep[0].ctypes.data if rays else None,
                             keep[1].ctypes.data if radiance else None, None, 0, flags, spp, max_bounce, 0, 0)
    return b, keep


@pytest.mark.parametrize("kw", [dict(rays=False), dict(radiance=False), dict(flags=native.FLAG_COUNT_STATS),
                                dict(flags=0x4), dict(flags=native.FLAG_ONE_SET), dict(flags=0x40000), dict(spp=0),
                                dict()])
def test_radiance_rejects_bad_batches_before_any_gpu_work(kw):
    """Argument errors come back without a device (a null context included)."""
    L = native.lib()
    assert L.zrt_context_radiance(None, None, None) == -1
    b, keep = _batch(**kw)
    assert L.zrt_context_radiance(None, C.byref(b), None) == -1
    assert not keep[1].any()


@pytest.fixture(scope="module")
def sphere(oracle_mod):
    return radiance_ref.RadianceRef(oracle_mod, scenes.get_scene("sphere"), (8, 8, 8))


def _mean_of_equal(v, spp):
    """renderWorker's pixel for spp samples that all equal v: the sum in sample order times the f32 1 / spp."""
    px = np.zeros(3, np.float32)
    for _ in range(spp):
        px = (px + v).astype(np.float32)
    return (px * (np.float32(1.0) / np.float32(spp))).astype(np.float32)


@pytest.mark.parametrize("spp", [1, 2, 3, 7])
def test_reference_ray_that_misses_everything_is_the_environment(sphere, oracle_mod, spp):
    xyz = scenes.get_scene("sphere").pos.reshape(-1, 3)
    far = xyz.max(0) + np.float32(10.0)
    d = np.array([[1.0, 2.0, 0.5], [0.0, 4.0, -0.0]], np.float32)      # pointing away from the mesh
    o = np.stack([far, far]).astype(np.float32)
    lin, rgb, ctr = sphere.radiance(o, d, spp, 4, seed=3, index_base=5)
    for i in range(2):
        nd = scenes.f32_normalize((d[i] + np.float32(0.0)).astype(np.float32))
        want = _mean_of_equal(oracle_mod.env_color(nd), spp)
        assert np.array_equal(lin[i].view(np.uint32), want.view(np.uint32)), (i, lin[i], want)
        assert np.array_equal(rgb[i], oracle_mod.to_rgb(want))
    assert int(ctr[0]) == 2 * spp and int(ctr[3]) == 0 and int(ctr[4]) == 2 * spp
    # no draw decides anything on such a path: the seed and the index change nothing
    lin2, _, _ = sphere.radiance(o, d, spp, 4, seed=9, index_base=0)
    assert np.array_equal(lin.view(np.uint32), lin2.view(np.uint32))


def test_reference_max_bounce_zero_is_black(sphere):
    o = np.array([[0.0, 0.0, 3.0], [5.0, 5.0, 5.0]], np.float32)
    d = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], np.float32)
    lin, rgb, ctr = sphere.radiance(o, d, 4, 0)
    assert not lin.view(np.uint32).any() and not rgb.any()             # +0, not -0
    assert [int(x) for x in ctr[:4]] == [0, 0, 0, 0] and int(ctr[4]) == 8


def test_reference_depends_on_the_index_and_the_seed(sphere):
    """A ray that hits the sphere scatters by its stream's draws."""
    soup = scenes.get_scene("sphere")
    c = soup.pos.reshape(-1, 3).mean(0)
    o = np.tile((c + np.array([0.0, 0.0, 4.0])).astype(np.float32), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (4, 1))
    a, _, ctr = sphere.radiance(o, d, 2, 4, seed=1)
    assert int(ctr[3]) >= 4, "the rays hit the scene"
    assert len({a[i].tobytes() for i in range(4)}) > 1, "equal rays, different indices"
    b, _, _ = sphere.radiance(o, d, 2, 4, seed=2)
    assert a.tobytes() != b.tobytes()
    shifted, _, _ = sphere.radiance(o[1:], d[1:], 2, 4, seed=1, index_base=1)
    assert np.array_equal(shifted.view(np.uint32), a[1:].view(np.uint32))
