"""Feature planes on the GPU (zrt_context_features, Context.features), bit for
bit as uint32 patterns against two references:

  feature_ref.PixelRecords   the per-pixel contract on the CPU (the trace and
                             surface references, checked against the oracle's
                             own path tracer in test_features_host.py), at up
                             to 64 pixels of a frame;
  feature_ref.device_composition
                             what a caller had to do before: the reference's
                             numpy camera rays through Context.surface with
                             hits, summed in numpy in sample order, at every
                             pixel of a frame.

The fuzz seeds (test_query_fuzz_gpu.py's scenes and contexts: host-built for
even seeds, device-built for odd ones) run their own camera, size, sample count
and render seed.  The fixed shapes use fuzz seed 33's soup (90 triangles, two
textures, emissive and BLEND materials), whose small frames hold pixels with
every sample hit, none hit and some hit.
"""
import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native

import edge_scenes
import feature_ref
import test_query_fuzz_gpu as qf
import trace_ref
from test_features_host import HAND_PLANES, hand_camera
from test_surface_host import hand_soup

pytestmark = pytest.mark.gpu

PLANES = feature_ref.PLANES
WIDTH = dict(native.FEATURE_PLANES)
SENTINEL = 0xABABABAB
FIXED_SEED = 33


def _same(got, want, what, keys=PLANES):
    for k in keys:
        g = np.ascontiguousarray(got[k]).reshape(len(want[k]), -1).view(np.uint32)
        w = np.ascontiguousarray(want[k]).reshape(len(want[k]), -1).view(np.uint32)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, (f"{what}, {k}: {bad.size} pixels differ, first at packed index {bad[0]}: got "
                               f"{[hex(int(x)) for x in g[bad[0]]]}, reference {[hex(int(x)) for x in w[bad[0]]]}")


def _packed_index(cam, tile=64, rank=0, num_ranks=1):
    """(pix, pos): the packed pixel order and each image index's place in it."""
    pix = native.tile_pixels(cam.w, cam.h, tile, rank, num_ranks)
    pos = np.full(cam.w * cam.h, -1, np.int64)
    pos[pix] = np.arange(len(pix))
    return pix, pos


def _sentinels(n, device=None):
    """A sentinel-filled buffer per plane for n pixels: numpy, or torch on `device`."""
    if device is None:
        return {k: np.full(max(n, 4) * WIDTH[k], SENTINEL, np.uint32) for k in PLANES}
    return {k: torch.full((max(n, 4) * WIDTH[k],), -0x54545455, dtype=torch.int32, device=device) for k in PLANES}


def _raw(ctx, cam, spp, bufs, ask=PLANES, **kw):
    """features_raw into `bufs` (numpy or torch), asking for the planes `ask`."""
    dev = not isinstance(next(iter(bufs.values())), np.ndarray)
    ptr = {k: (bufs[k].data_ptr() if dev else bufs[k].ctypes.data) for k in ask}
    return ctx.features_raw(cam, spp, ptr, dev, **kw)


def _planes_of(bufs, n):
    """The first n pixels of sentinel buffers as a planes dict of numpy arrays."""
    out = {}
    for k in PLANES:
        a = bufs[k] if isinstance(bufs[k], np.ndarray) else bufs[k].cpu().numpy().view(np.uint32)
        a = a[:n * WIDTH[k]]
        out[k] = a.reshape(n, 3) if WIDTH[k] == 3 else a
    return out


# ------------------------------------------------------------ the fuzz frames
@pytest.fixture(scope="module")
def frame(oracle_mod):
    def get(seed):
        if seed not in qf._CASES:                  # one set of references for every module that needs them
            qf._CASES[seed] = qf.SeedCase(oracle_mod, seed)
        return qf._CASES[seed], feature_ref.seed_frame(oracle_mod, qf._CASES[seed])
    return get


@pytest.fixture(scope="module")
def fuzz_context(frame):
    """The seed's context; one at a time."""
    made = {}

    def get(seed):
        if seed not in made:
            for rs in made.values():
                rs.close()
            made.clear()
            cs, _ = frame(seed)
            made[seed] = RenderScene(cs.soup, cs.res, device=0, device_build=cs.device_build)
        return made[seed]
    yield get
    for rs in made.values():
        rs.close()


@pytest.mark.parametrize("seed", qf.SEEDS)
def test_fuzz_frames_match_both_references(seed, frame, fuzz_context, oracle_mod):
    """Seeds 0, 1, 4, 5, ... through host pointers, 2, 3, 6, 7, ... through
    device pointers: both kinds meet both builds."""
    (cs, fr), rs = frame(seed), fuzz_context(seed)
    what = f"seed {seed}, {cs.soup.num_triangles} triangles, grid {cs.res}, {fr.w}x{fr.h} at {fr.spp} spp"
    pix, pos = _packed_index(fr.cam)
    n = len(pix)
    if (seed // 2) % 2:
        if torch is None or not torch.cuda.is_available():
            pytest.skip("torch sees no device")
        bufs = _sentinels(n, torch.device("cuda", 0))
        torch.cuda.current_stream().synchronize()
        st = _raw(rs.context, fr.cam, fr.spp, bufs, seed=cs.rseed)
        got = _planes_of(bufs, n)
    else:
        got = rs.context.features(fr.cam, fr.spp, seed=cs.rseed)
        st = got["stats"]
        for k in PLANES:                           # the images are the packed planes scattered through tile_pixels
            assert np.array_equal(got["images"][k].reshape(n, -1)[pix].view(np.uint32),
                                  got[k].reshape(n, -1).view(np.uint32)), (what, k)
    want = fr.rec.planes(fr.spp)
    at = pos[fr.pixels]
    _same({k: np.asarray(got[k])[at] for k in PLANES}, want, what + " vs the CPU reference")
    comp = feature_ref.device_composition(rs.context, oracle_mod, fr.cam, cs.rseed, pix, fr.spp)
    _same(got, comp, what + " vs the device composition")
    hits = int(np.asarray(got["hits"]).view(np.uint32).sum(dtype=np.int64))
    assert (st["segments"], st["samples"], st["hits"]) == (n * fr.spp, n * fr.spp, hits), what


# ------------------------------------------------------------ the fixed shapes
@pytest.fixture(scope="module")
def fixed(frame):
    cs, _ = frame(FIXED_SEED)
    rs = RenderScene(cs.soup, cs.res, device=0)
    yield cs, rs
    rs.close()


@pytest.fixture(scope="module")
def composed(fixed, oracle_mod):
    """device_composition of a (w, h, spp, seed) frame of the fixed scene, computed once."""
    cs, rs = fixed
    made = {}

    def get(w, h, spp, seed):
        if (w, h, spp, seed) not in made:
            cam = camera_for(cs.soup, None, w, h)
            pix = native.tile_pixels(w, h)
            made[(w, h, spp, seed)] = feature_ref.device_composition(rs.context, oracle_mod, cam, seed, pix, spp)
        return made[(w, h, spp, seed)]
    return get


@pytest.mark.parametrize("spp", [1, 16, 17, 33])
def test_sample_counts_on_a_frame_below_one_wave(spp, fixed, composed):
    """9 x 7: 63 pixels, below one wave and one resolve block; 16 is the
    resolve's chunk, 17 and 33 one past one and two chunks.  At 33 spp any
    samples_per_pass gives the same bits."""
    cs, rs = fixed
    cam = camera_for(cs.soup, None, 9, 7)
    want = composed(9, 7, spp, 5)
    assert (want["hits"] == spp).any() and (want["hits"] == 0).any()
    assert spp == 1 or ((want["hits"] > 0) & (want["hits"] < spp)).any()
    got = rs.context.features(cam, spp, seed=5)
    _same(got, want, f"9x7 at {spp} spp")
    assert got["stats"]["trace_launches"] == 2
    if spp == 33:
        for per_pass in (1, 5, 33):
            again = rs.context.features(cam, spp, seed=5, samples_per_pass=per_pass)
            _same(again, got, f"9x7 at 33 spp, {per_pass} samples per pass")
            assert again["stats"]["trace_launches"] == 2 * ((33 + per_pass - 1) // per_pass)


def test_ranks_own_their_tiles(fixed, composed):
    """20 x 13 in tiles of 8 (3 x 2 tiles) over 3 ranks: each rank's packed
    planes are the one-rank call's at its tile_pixels; with 7 ranks the last
    owns no tile, returns OK and leaves the sentinels."""
    cs, rs = fixed
    cam = camera_for(cs.soup, None, 20, 13)
    _, pos = _packed_index(cam, 8)
    whole = rs.context.features(cam, 3, seed=9, tile_size=8)
    assert len(whole["hits"]) == 260
    want = composed(20, 13, 3, 9)                      # (tile 64 order: through the image indices)
    pix64, _ = _packed_index(cam)
    _same({k: np.asarray(whole[k])[pos[pix64]] for k in PLANES}, want, "20x13 one rank")
    seen = 0
    for rank in range(3):
        part = rs.context.features(cam, 3, seed=9, tile_size=8, rank=rank, num_ranks=3)
        mine = native.tile_pixels(20, 13, 8, rank, 3)
        assert "images" not in part and len(part["hits"]) == len(mine) > 0
        _same(part, {k: np.asarray(whole[k])[pos[mine]] for k in PLANES}, f"rank {rank} of 3")
        assert part["stats"]["segments"] == 3 * len(mine)
        seen += len(mine)
    assert seen == 260
    assert native.tile_pixels(20, 13, 8, 6, 7).size == 0
    bufs = _sentinels(4)
    st = _raw(rs.context, cam, 3, bufs, seed=9, tile_size=8, rank=6, num_ranks=7)
    assert all((b == SENTINEL).all() for b in bufs.values())
    assert (st["segments"], st["samples"], st["hits"], st["trace_launches"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("ask", [("depth",), ("hits",), ("base_color", "emissive", "depth", "transparency", "hits")],
                         ids=["depth", "hits", "all-but-normal"])
def test_plane_subsets_leave_the_others_alone(ask, fixed, composed):
    cs, rs = fixed
    cam = camera_for(cs.soup, None, 9, 7)
    want = composed(9, 7, 3, 5)
    bufs = _sentinels(63 + 2)                          # two guard pixels behind every plane
    _raw(rs.context, cam, 3, bufs, ask=ask, seed=5)
    got = _planes_of(bufs, 63)
    _same(got, want, f"planes {ask}", keys=ask)
    for k in PLANES:
        if k in ask:
            assert (bufs[k][63 * WIDTH[k]:] == SENTINEL).all(), k
        else:
            assert (bufs[k] == SENTINEL).all(), k
    part = rs.context.features(cam, 3, seed=5, planes=ask)
    assert sorted(k for k in part if k in PLANES) == sorted(ask) and sorted(part["images"]) == sorted(ask)
    _same(part, want, f"Context.features planes {ask}", keys=ask)


def test_kernel_selection_flags_give_the_same_planes(fixed, composed):
    cs, rs = fixed
    cam = camera_for(cs.soup, None, 20, 13)
    want = composed(20, 13, 3, 9)
    for name in ("FLAG_MT_EXACT", "FLAG_LANE_WALK", "FLAG_FRUSTUM", "FLAG_NO_FRUSTUM"):
        got = rs.context.features(cam, 3, seed=9, flags=getattr(native, name))
        _same(got, want, name)
        # the frustum bounds are one more launch, where the flag asks for them
        assert got["stats"]["trace_launches"] == (3 if name == "FLAG_FRUSTUM" else 2), name
    # the bounce launches' flags do nothing here
    got = rs.context.features(cam, 3, seed=9, flags=native.FLAG_ESCAPE | native.FLAG_BFCULL | native.FLAG_ONE_SET |
                              native.FLAG_KERNEL_TIMES | native.FLAG_NO_HOP | native.FLAG_RELEASE)
    _same(got, want, "bounce flags")


def test_the_benchmark_grid_with_and_without_the_frustum_bounds(oracle_mod):
    """The Cornell box on the benchmark's grid (config.json: brick-major packed
    words) at 64 x 48, two resolve blocks: the walk a benchmark frame takes."""
    import os
    from zig_raytracing_contest_amd import Config, scenes
    soup = scenes.get_scene("cornell")
    res = Config.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config.json"))
    cam = camera_for(soup, None, 64, 48)
    rs = RenderScene(soup, res.grid_resolution, device=0)
    try:
        pix = native.tile_pixels(64, 48)
        want = feature_ref.device_composition(rs.context, oracle_mod, cam, 3, pix, 2)
        for flags, launches in ((native.FLAG_FRUSTUM, 3), (0, 2), (native.FLAG_NO_FRUSTUM, 2)):
            got = rs.context.features(cam, 2, seed=3, flags=flags)
            _same(got, want, f"cornell, flags {flags:#x}")
            assert got["stats"]["trace_launches"] == launches
        assert got["stats"]["hits"] == int(want["hits"].sum()) > 0
    finally:
        rs.close()


def test_a_far_scene_runs_the_exact_kernels_by_itself(oracle_mod):
    """edge_scenes.FAR's floor at 2^62: the context takes the IEEE-division
    walk unasked (zrt_context::mt_exact); the floor is seen."""
    kind, scale, exact = edge_scenes.FAR[7]
    assert (kind, scale, exact) == ("floor", 2.0 ** 62, True)
    soup = edge_scenes.far_scene(kind, scale)
    cam = camera_for(soup, None, 40, 32)
    rs = RenderScene(soup, (16, 16, 16), device=0)
    try:
        pix = native.tile_pixels(40, 32)
        want = feature_ref.device_composition(rs.context, oracle_mod, cam, 0, pix, 2)
        got = rs.context.features(cam, 2)
        _same(got, want, "far floor at 2^62")
        assert 0 < got["stats"]["hits"] == int(want["hits"].sum())
    finally:
        rs.close()


@pytest.mark.parametrize("w,h,spp", [(20, 13, 3), (9, 7, 17)])
def test_counters_are_the_oracles_at_one_bounce(w, h, spp, fixed, oracle_mod):
    """A counting render at max_bounce = 1 traces exactly these segments."""
    cs, rs = fixed
    cam = camera_for(cs.soup, None, w, h)
    c = cs.soup.camera()
    ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, w, h)
    _, _, ctr = cs.ref.scene.render(ocam, spp, 1, oracle_mod.RNG_PATH, 21, 8)
    counted = rs.context.features(cam, spp, seed=21, stats=True)
    st = counted["stats"]
    assert [st["segments"], st["cells_visited"], st["triangle_tests"], st["hits"]] == [int(x) for x in ctr[:4]]
    assert st["samples"] == w * h * spp
    plain = rs.context.features(cam, spp, seed=21)
    _same(counted, plain, "the counting instantiation")
    st = plain["stats"]
    assert [st["segments"], st["hits"]] == [int(ctr[0]), int(ctr[3])]
    assert st["hits"] == int(plain["hits"].sum())


def test_features_alternate_with_renders_and_queries(fixed):
    """render, features, render, trace, features on one context: equal images,
    equal planes, and the profile of the last render stays."""
    cs, rs = fixed
    cam = camera_for(cs.soup, None, 20, 13)
    img0, _ = rs.render(cam, num_samples=3, max_bounce=4, seed=9, flags=native.FLAG_KERNEL_TIMES)
    before = rs.context.profile()
    first = rs.context.features(cam, 3, seed=9)
    assert rs.context.profile() == before and before["kernels"]
    img1, _ = rs.render(cam, num_samples=3, max_bounce=4, seed=9)
    assert np.array_equal(img0, img1)
    res = rs.trace(cs.o, cs.d)
    assert np.array_equal(trace_ref.hit_bits(res), cs.bits)
    last = rs.context.features(cam, 3, seed=9)
    _same(last, first, "features after render and trace")
    assert first["stats"]["hits"] > 0


def test_bad_arguments_raise_on_a_live_context(fixed):
    cs, rs = fixed
    cam = camera_for(cs.soup, None, 9, 7)
    bufs = _sentinels(63)
    ptr = {k: bufs[k].ctypes.data for k in PLANES}
    for spp, pointers, kw in ((3, {}, {}), (0, ptr, {}), (65536, ptr, {}), (3, ptr, dict(reserved=1)),
                              (3, ptr, dict(rank=1, num_ranks=1)), (3, ptr, dict(tile_size=12))):
        with pytest.raises(native.ZrtError) as e:
            rs.context.features_raw(cam, spp, pointers, False, **kw)
        assert e.value.status == -1
    assert all((b == SENTINEL).all() for b in bufs.values())
    rs.context.features_raw(cam, 3, ptr, False)                # the control: the valid call runs
    assert not (bufs["hits"][:63] == SENTINEL).any()


def test_hand_derived_planes_on_the_gpu():
    """test_features_host.py's case: four equal exact samples, times 1 / 4."""
    soup = hand_soup()
    for build in (False, True):
        rs = RenderScene(soup, (2, 2, 2), device=0, device_build=build)
        for flags in (0, native.FLAG_MT_EXACT, native.FLAG_COUNT_STATS):
            got = rs.context.features(hand_camera(), 4, seed=123, flags=flags)
            for k in PLANES:
                want = np.array(HAND_PLANES[k], np.uint32 if k == "hits" else np.float32)
                assert np.array_equal(got[k].reshape(-1).view(np.uint32), want.view(np.uint32)), (build, flags, k, got[k])
            assert got["stats"]["hits"] == 4
        rs.close()
