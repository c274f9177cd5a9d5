"""Reprojection (zrt_context_reproject), the part that runs without a GPU: the
C ABI's declaration, flag, export and binding, the batch's layout against the
header's own comment, the argument errors that come back before any device
work, properties of the numpy reference (reproject_ref.py) that hold whatever
the GPU does, and the quality condition of the wrapper's default tolerances.

The quality condition: Cornell and the textured fuzz scene of test_tall_gpu.py
at 33 x 31, grid 16^3, max_bounce 4, under four camera moves.  The previous
frame is the oracle's 64-sample frame at camera A with history length 16, the
current frame its 4-sample frame at camera B; the guides are feature_ref.py's
planes of the 4 camera samples per pixel at A and at B; depth_tolerance 0.05,
normal_tolerance 0.5, max_history 32.  The error is the mean absolute linear
error against the oracle's 256-sample frame at B.  Each row asserts that the
blended frame is closer than the raw one and that at least half of the pixels
have history (a condition, not a measurement: it keeps a run without history
from passing).  The translations are 0.04, 0.02 and 0.02 of the scene's largest
absolute vertex coordinate (5.0 for cornell, 2.997 for the fuzz scene); yaw
turns lower_left_corner, right and up about the world y axis.  Seen with this
reference (pixels with history, raw -> blended, ratio):
  cornell  identical                            0.935  0.155396 -> 0.043227  0.278
  cornell  origin + (0.2, 0.1, 0)               0.855  0.143742 -> 0.094247  0.656
  cornell  yaw 0.05                             0.840  0.144709 -> 0.063060  0.436
  cornell  origin + (0.2, 0.1, 0.1), yaw 0.05   0.841  0.138706 -> 0.101666  0.733
  fuzz     identical                            1.000  0.018472 -> 0.004054  0.219
  fuzz     origin + (0.12, 0.06, 0)             0.710  0.014481 -> 0.009755  0.674
  fuzz     yaw 0.05                             0.898  0.018794 -> 0.006594  0.351
  fuzz     origin + (0.12, 0.06, 0.06), yaw 0.05  0.658  0.012762 -> 0.007938  0.622
No row needed its translation halved.
"""
import ctypes as C
import re

import numpy as np
import pytest

from zig_raytracing_contest_amd import camera_for, native

import feature_ref
import refine_cases as rc
import reproject_ref as rr
from test_denoise_host import _header, _struct

F = np.float32
INF = float("inf")
NAN = float("nan")


def to_native(c):
    """A native.Camera of a reproject_ref.Cam (or of any camera)."""
    c = rr.cam_of(c)
    cam = native.Camera()
    cam.w, cam.h = c.w, c.h
    for name, v in (("origin", c.origin), ("lower_left_corner", c.llc), ("right", c.right), ("up", c.up)):
        getattr(cam, name)[:] = [float(x) for x in v]
    return cam


def pinhole(w, h, origin=(0.25, -0.5, 6.0), fov=0.8):
    """A camera looking down -z: `up` points world-down, row 0 is the top row."""
    s = 2.0 * np.tan(fov / 2) / h
    return rr.Cam(w, h, np.array(origin, F), np.array([-w / 2 * s, h / 2 * s, -1.0], F), np.array([s, 0, 0], F),
                  np.array([0, -s, 0], F))


def test_header_declares_reproject_and_native_exports_and_binds_it():
    hdr = _header()
    assert re.search(r"\bint\s+zrt_context_reproject\s*\(\s*zrt_context\s*\*\s*\w*\s*,\s*const\s+zrt_reproject_batch\s*\*"
                     r"\s*\w*\s*,\s*zrt_stats\s*\*", hdr)
    sec = "reproject: carry a frame's history across a camera change (ABI 2, added)"
    assert hdr.index("denoise: edge-avoiding a-trous filter (ABI 2, added)") < hdr.index(sec) < \
        hdr.index("typedef struct zrt_group zrt_group")
    # the next free bit after ZRT_DENOISE_ROW_MAJOR
    assert re.search(r"#define\s+ZRT_DENOISE_ROW_MAJOR\s+0x100000u", hdr)
    assert re.search(r"#define\s+ZRT_REPROJECT_ROW_MAJOR\s+0x200000u", hdr) and native.REPROJECT_ROW_MAJOR == 0x200000
    assert re.search(r"#define\s+ZRT_ABI_VERSION\s+2\b", hdr) and native.lib().zrt_abi_version() == 2
    assert "zrt_context_reproject" in native.EXPORTS
    assert hasattr(native.lib(), "zrt_context_reproject")        # (dlsym: libzrt.so exports it)
    for name in ("reproject_raw", "reproject"):
        assert callable(getattr(native.Context, name))
    assert callable(native.Film.reproject) and callable(native.History.update)
    assert native.REPROJECT_DEFAULTS == (32, 0.05, 0.5)


def test_batch_layout_is_the_headers():
    rb = native.ReprojectBatch
    names, tail = _struct(_header(), "zrt_reproject_batch")
    assert names == [n for n, _ in rb._fields_]
    m = re.search(r"(\d+)\s*B;\s*offsets((?:\s+\d+)+)", tail)
    assert m, tail
    assert C.sizeof(rb) == int(m.group(1)) == 136
    assert [getattr(rb, n).offset for n in names] == [int(x) for x in m.group(2).split()]


# ------------------------------------------------------------------ refusals
W8 = H8 = 8
CAMS = {"cur": to_native(pinhole(W8, H8)), "prev": to_native(rr.moved(pinhole(W8, H8), (0.05, 0.0, 0.0))),
        "w0": to_native(pinhole(W8, H8)), "h0": to_native(pinhole(W8, H8)), "other": to_native(pinhole(H8, 2 * W8)),
        "big": to_native(pinhole(W8, H8)), "huge": to_native(pinhole(W8, H8))}
CAMS["w0"].w = 0
CAMS["h0"].h = 0
CAMS["big"].w, CAMS["big"].h = 1 << 16, 1 << 15                    # P = 2^31
CAMS["huge"].w, CAMS["huge"].h = 1 << 16, (1 << 15) + 1


def cam_ptr(name):
    return C.addressof(CAMS[name])


def host_planes(P=W8 * H8):
    """The inputs of a valid 8 x 8 call: colour, depth, normal, previous colour, depth, normal, length."""
    z = np.full(P, 6.0, F)
    n = np.zeros((P, 3), F)
    n[:, 2] = 1
    return [np.full((P, 3), 0.5, F), z, n, np.full((P, 3), 0.25, F), z.copy(), n.copy(), np.full(P, 3, np.uint32)]


def guarded_outputs(P=W8 * H8):
    return [np.full(3 * P, 0xA0A0A0A0, np.uint32), np.full(P, 0xB1B1B1B1, np.uint32), np.full(2 * P, 0xC2C2C2C2, np.uint32)]


def untouched(outs):
    return (outs[0] == 0xA0A0A0A0).all() and (outs[1] == 0xB1B1B1B1).all() and (outs[2] == 0xC2C2C2C2).all()


def _valid(x, outs):
    """A batch that passes every check that needs no device: 8 x 8, normals and lengths, host pointers."""
    c, z, n, pc, pz, pn, pl = (p.ctypes.data for p in x)
    return dict(tile_size=8, max_history=32, depth_tolerance=0.05, normal_tolerance=0.5, on_device=0, flags=0,
                camera=cam_ptr("cur"), prev_camera=cam_ptr("prev"), color=c, film=None, depth=z, normal=n,
                prev_color=pc, prev_depth=pz, prev_normal=pn, prev_length=pl, color_out=outs[0].ctypes.data,
                length_out=outs[1].ctypes.data, motion=outs[2].ctypes.data, _reserved=0)


REFUSALS = {
    "no camera": dict(camera=None), "no previous camera": dict(prev_camera=None),
    "w 0": dict(camera=cam_ptr("w0"), prev_camera=cam_ptr("w0")),
    "h 0": dict(camera=cam_ptr("h0"), prev_camera=cam_ptr("h0")),
    "P above 2^31": dict(camera=cam_ptr("huge"), prev_camera=cam_ptr("huge")),
    "a previous camera of another size": dict(prev_camera=cam_ptr("other")),
    "tile not a multiple of 8": dict(tile_size=12),
    "max_history 0": dict(max_history=0), "max_history 65536": dict(max_history=65536),
    "depth_tolerance NaN": dict(depth_tolerance=NAN), "depth_tolerance negative": dict(depth_tolerance=-0.05),
    "depth_tolerance -inf": dict(depth_tolerance=-INF),
    "normal_tolerance NaN": dict(normal_tolerance=NAN), "normal_tolerance negative": dict(normal_tolerance=-1.0),
    "no colour source": dict(color=None),
    "color and film": dict(film=0x1000),
    "film with row major": dict(color=None, film=0x1000, flags=native.REPROJECT_ROW_MAJOR),
    "no depth": dict(depth=None), "no previous colour": dict(prev_color=None),
    "no previous depth": dict(prev_depth=None), "no colour output": dict(color_out=None),
    "on_device 2": dict(on_device=2),
    "_reserved": dict(_reserved=1), "_reserved high word": dict(_reserved=1 << 32),
    "the denoiser's flag": dict(flags=native.DENOISE_ROW_MAJOR),
    "a render flag": dict(flags=native.FLAG_COUNT_STATS),
    "a flag beside the valid one": dict(flags=native.REPROJECT_ROW_MAJOR | 0x400000),
}
# what the same fields may hold: these batches are valid (refused below only for the null context)
ALLOWED = {
    "tolerances +inf": dict(depth_tolerance=INF, normal_tolerance=INF),
    "tolerances 0": dict(depth_tolerance=0.0, normal_tolerance=0.0),
    "no normal: its tolerance is not read": dict(normal=None, normal_tolerance=NAN),
    "no previous normal: its tolerance is not read": dict(prev_normal=None, normal_tolerance=-1.0),
    "P = 2^31": dict(camera=cam_ptr("big"), prev_camera=cam_ptr("big")),
    "row major ignores tile_size": dict(flags=native.REPROJECT_ROW_MAJOR, tile_size=12),
    "max_history 1": dict(max_history=1), "max_history 65535": dict(max_history=65535),
    "no lengths in": dict(prev_length=None), "no lengths out": dict(length_out=None), "no motion": dict(motion=None),
}


def test_reproject_rejects_bad_batches_before_any_gpu_work():
    """Argument errors come back without a device (a null context included),
    and the outputs stay as they were."""
    L = native.lib()
    assert L.zrt_context_reproject(None, None, None) == -1
    x, outs = host_planes(), guarded_outputs()
    st = native.Stats()
    for change in [{}] + list(REFUSALS.values()) + list(ALLOWED.values()):
        batch = native.ReprojectBatch(**{**_valid(x, outs), **change})
        assert L.zrt_context_reproject(None, C.byref(batch), C.byref(st)) == -1
    assert untouched(outs)
    assert st.samples == 0 and st.trace_launches == 0


def test_denoise_still_refuses_the_reprojection_flag():
    import test_denoise_host as dh
    assert dh.REFUSALS["a flag beside the valid one"] == dict(flags=native.DENOISE_ROW_MAJOR | native.REPROJECT_ROW_MAJOR)


# --------------------------------------------------- properties of the reference
def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


W, H = 33, 31


def _frame(seed=5, depth=4.0):
    """A current colour, a depth plane with a depth-0 sky band on top, and a previous colour."""
    rng = np.random.default_rng(seed)
    c = rng.random((H, W, 3)).astype(F)
    pc = rng.random((H, W, 3)).astype(F)
    z = np.full((H, W), depth, F)
    z[:4] = 0.0
    return c, z, pc


def test_an_identical_camera_moves_nothing_and_finds_history_wherever_there_is_depth():
    cam = pinhole(W, H)
    c, z, pc = _frame()
    r = rr.reproject(cam, cam, c, z, pc, np.full((H, W), 4.0, F))
    has = z > 0
    print("identical camera: largest |motion| %.3g px" % np.abs(r["motion"][has]).max())
    assert np.abs(r["motion"][has]).max() < 1e-4
    assert np.array_equal(r["has"], has) and r["hits"] == int(has.sum())
    assert (_bits(r["motion"][~has]) == 0x7FC00000).all()
    assert (r["length"][has] == 2).all() and (r["length"][~has] == 1).all()
    assert np.array_equal(_bits(r["color"][~has]), _bits(c[~has]))
    # N = 2: half history, half colour; the history is the previous colour up to the bilinear weights' rounding
    assert np.abs(r["color"][has].astype(np.float64) - (0.5 * pc[has] + 0.5 * c[has])).max() < 1e-3


def test_a_previous_camera_turned_away_sees_nothing():
    cam = pinhole(W, H)
    c, z, pc = _frame()
    r = rr.reproject(cam, rr.moved(cam, yaw=np.pi), c, z, pc, np.full((H, W), 4.0, F), prev_length=np.full((H, W), 7, np.uint32))
    assert r["hits"] == 0 and not r["has"].any() and (r["length"] == 1).all()
    assert np.array_equal(_bits(r["color"]), _bits(c))
    assert (_bits(r["motion"]) == 0x7FC00000).all()               # behind the previous camera: g <= 0, no projection


def test_a_mirrored_previous_camera_gives_the_mirrored_coordinates():
    """right negated: D < 0, so A, B and Cv change sign, which leaves g and b
    the same bits and turns a into -a."""
    cam = pinhole(W, H)
    prev = rr.moved(cam, (0.3, 0.1, 0.2), yaw=0.1)
    mirrored = prev._replace(right=-prev.right)
    assert rr.constants(prev)[3] and rr.constants(mirrored)[3]
    assert rr._dot(prev.llc, rr._cross(prev.right, prev.up)) > 0 > rr._dot(mirrored.llc, rr._cross(mirrored.right, mirrored.up))
    z = _frame()[1]
    d0, a0, b0, zq0, _, _ = rr.project(cam, prev, z)
    d1, a1, b1, zq1, _, _ = rr.project(cam, mirrored, z)
    assert np.array_equal(d0, d1) and d0.any()
    assert np.array_equal(_bits(a1[d0]), _bits(-a0[d0])) and np.array_equal(_bits(b1[d0]), _bits(b0[d0]))
    assert np.array_equal(_bits(zq1), _bits(zq0))


def test_a_degenerate_previous_camera_has_no_projection():
    cam = pinhole(W, H)
    flat = cam._replace(right=np.zeros(3, F))                      # D = 0
    assert not rr.constants(flat)[3]
    c, z, pc = _frame()
    r = rr.reproject(cam, flat, c, z, pc, np.full((H, W), 4.0, F))
    assert r["hits"] == 0 and (r["length"] == 1).all() and np.array_equal(_bits(r["color"]), _bits(c))
    assert (_bits(r["motion"]) == 0x7FC00000).all()
    nan = cam._replace(up=np.array([NAN, 0, 0], F))                # D = NaN
    assert rr.reproject(cam, nan, c, z, pc, np.full((H, W), 4.0, F))["hits"] == 0


def test_lengths_follow_the_least_tap_and_max_history():
    cam = pinhole(W, H)
    c, z, pc = _frame()
    c[5, 6] = -0.0                                                 # N == 1 keeps a -0's sign: the colour's bits
    has = z > 0
    pz = np.full((H, W), 4.0, F)
    for lp in (1, 5, 31, 32, 65535, 0xFFFFFFFF):
        for mx in (1, 2, 32, 65535):
            r = rr.reproject(cam, cam, c, z, pc, pz, prev_length=np.full((H, W), lp, np.uint32), max_history=mx)
            assert (r["length"][has] == min(lp, mx - 1) + 1).all() and (r["length"][~has] == 1).all(), (lp, mx)
            assert r["hits"] == int(has.sum())                     # W > 0, whatever N is
            if mx == 1:
                assert np.array_equal(_bits(r["color"]), _bits(c))
    r = rr.reproject(cam, cam, c, z, pc, pz, prev_length=np.zeros((H, W), np.uint32))
    assert r["hits"] == 0 and np.array_equal(_bits(r["color"]), _bits(c))        # length 0: no tap counts
    # one short tap lowers its neighbours' N and nobody else's
    lens = np.full((H, W), 9, np.uint32)
    lens[10, 10] = 2
    r = rr.reproject(cam, cam, c, z, pc, pz, prev_length=lens)
    assert r["length"][10, 10] == 3 and set(np.unique(r["length"][has])) == {3, 10}
    assert (r["length"][has] == 3).sum() <= 4 and (r["length"][12:, 12:] == 10).all()


def test_guides_reject_taps():
    cam = pinhole(W, H)
    c, z, pc = _frame()
    has = z > 0
    far = np.full((H, W), 4.5, F)                                  # 12.5 % off: outside 0.05, inside 0.25
    assert rr.reproject(cam, cam, c, z, pc, far)["hits"] == 0
    assert rr.reproject(cam, cam, c, z, pc, far, depth_tolerance=0.25)["hits"] == int(has.sum())
    assert rr.reproject(cam, cam, c, z, pc, far, depth_tolerance=INF)["hits"] == int(has.sum())
    n = np.zeros((H, W, 3), F)
    n[..., 2] = 1
    pn = n.copy()
    pn[:, W // 2:] = (1, 0, 0)                                     # |dn|^2 = 2 on the right half
    pz = np.full((H, W), 4.0, F)
    r = rr.reproject(cam, cam, c, z, pc, pz, normal=n, prev_normal=pn)
    assert r["has"][:, :W // 2 - 1][has[:, :W // 2 - 1]].all() and not r["has"][:, W // 2 + 1:].any()
    assert rr.reproject(cam, cam, c, z, pc, pz, normal=n, prev_normal=pn, normal_tolerance=1.5)["hits"] == int(has.sum())
    assert rr.reproject(cam, cam, c, z, pc, pz, normal=n)["hits"] == int(has.sum())   # one normal plane: no guide
    bad = pc.copy()
    bad[20, 20, 1] = np.inf
    bad[22, 8, 0] = np.nan
    r = rr.reproject(cam, cam, c, z, bad, pz)
    assert np.isfinite(r["color"]).all()                           # such a tap is skipped: nothing spreads


def test_row_major_and_packed_are_one_function():
    w, h = 13, 5
    cam = pinhole(w, h)
    prev = rr.moved(cam, (0.2, 0.0, 0.1), yaw=0.03)
    rng = np.random.default_rng(13)
    c, pc = rng.random((h, w, 3)).astype(F), rng.random((h, w, 3)).astype(F)
    z = (F(4.0) + rng.random((h, w)).astype(F) * F(0.05)).astype(F)
    pl = rng.integers(1, 40, (h, w)).astype(np.uint32)
    pix = native.tile_pixels(w, h, 8)
    want = rr.reproject(cam, prev, c, z, pc, z, prev_length=pl)
    got = rr.reproject_packed(pix, cam, prev, c.reshape(-1, 3)[pix], z.reshape(-1)[pix], pc.reshape(-1, 3)[pix],
                              z.reshape(-1)[pix], prev_length=pl.reshape(-1)[pix])
    assert want["hits"] == got["hits"] > w * h // 2
    assert np.array_equal(_bits(got["color"]), _bits(want["color"].reshape(-1, 3)[pix]))
    assert np.array_equal(got["length"], want["length"].reshape(-1)[pix])
    assert np.array_equal(_bits(got["motion"]), _bits(want["motion"].reshape(-1, 2)[pix]))


# ----------------------------------------------------------- the quality condition
QUALITY = (33, 31, 4, 64, 256, 16)      # w, h, the current frame's samples, the previous frame's, the converged one's, its length
MOVES = {
    "cornell": {"identical": ((0.0, 0.0, 0.0), 0.0), "translated": ((0.2, 0.1, 0.0), 0.0), "yawed": ((0.0, 0.0, 0.0), 0.05),
                "both": ((0.2, 0.1, 0.1), 0.05)},
    "fuzz": {"identical": ((0.0, 0.0, 0.0), 0.0), "translated": ((0.12, 0.06, 0.0), 0.0), "yawed": ((0.0, 0.0, 0.0), 0.05),
             "both": ((0.12, 0.06, 0.06), 0.05)},
}
_AT = {}


def scene_frames(orc, name, move):
    """The oracle frames and reference guide planes of scene `name` at camera
    A (move "identical") or B: {"cam", "lin": {spp: (P, 3) float32}, "planes"},
    row-major, computed once."""
    key = (name, move)
    if key in _AT:
        return _AT[key]
    w, h, spp = QUALITY[:3]
    t = rc.tall_scene(orc, name)
    base = camera_for(t.soup, None, w, h)
    if move == "identical":
        cam = rr.cam_of(base)
        lin = lambda n: t.frame(w, h, n, rc.MB)[1].view(F).reshape(-1, 3)
    else:
        cam = rr.moved(base, *MOVES[name][move])
        ocam = orc.camera_from_dict(dict(w=w, h=h, origin=cam.origin, llc=cam.llc, right=cam.right, up=cam.up))
        lin = lambda n: t.oracle.render(ocam, n, rc.MB, orc.RNG_PATH, t.seed, rc.THREADS)[1].reshape(-1, 3).copy()
    rec = feature_ref.PixelRecords(orc, t.ray_ref, t.soup, to_native(cam), t.seed, np.arange(w * h), spp)
    out = {"cam": cam, "lin": {}, "planes": rec.planes(spp), "_lin": lin}
    _AT[key] = out
    return out


def frame_of(at, spp):
    if spp not in at["lin"]:
        at["lin"][spp] = at["_lin"](spp)
        at["lin"][spp].setflags(write=False)
    return at["lin"][spp]


@pytest.mark.parametrize("move", ("identical", "translated", "yawed", "both"))
@pytest.mark.parametrize("name", rc.SCENES)
def test_history_brings_a_4_sample_frame_closer_to_the_converged_one(name, move, oracle_mod):
    w, h, spp, before, many, length = QUALITY
    A, B = scene_frames(oracle_mod, name, "identical"), scene_frames(oracle_mod, name, move)
    noisy = frame_of(B, spp).reshape(h, w, 3)
    truth = frame_of(B, many).reshape(h, w, 3).astype(np.float64)
    mx, dt, nt = native.REPROJECT_DEFAULTS
    r = rr.reproject(B["cam"], A["cam"], noisy, B["planes"]["depth"], frame_of(A, before), A["planes"]["depth"],
                     B["planes"]["normal"], A["planes"]["normal"], np.full((h, w), length, np.uint32), mx, dt, nt)
    raw = float(np.abs(noisy - truth).mean())
    blended = float(np.abs(r["color"] - truth).mean())
    share = r["hits"] / (w * h)
    print(f"{name} {move}: pixels with history {share:.3f}, mean absolute error against {many} samples: "
          f"raw {raw:.6f} -> blended {blended:.6f} (ratio {blended / raw:.3f})")
    assert blended < raw
    assert share >= 0.5
