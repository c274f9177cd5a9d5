"""The hand-made edge scenes shared by the GPU tests (test_gpu_edges.py,
test_bfcull_gpu.py, test_trace_gpu.py, test_radiance_gpu.py,
test_grid_build_fuzz.py); not a test module itself."""
import dataclasses
import math

import numpy as np

from zig_raytracing_contest_amd import scenes

HAND_RES = (8, 8, 8)


def with_camera(soup, eye, target, yfov_deg=50.0):
    cam = scenes.CameraDef("Edge", scenes.look_at(eye, target), math.radians(yfov_deg), None)
    return dataclasses.replace(soup, cameras=[cam])


def degenerate_sphere():
    s = scenes.get_scene("sphere")
    v = np.array([[0.2, 0.1, 0.9], [0.2, 0.1, 0.9], [0.2, 0.1, 0.9],      # one point
                  [-0.5, 0.0, 1.1], [0.0, 0.0, 1.1], [0.5, 0.0, 1.1],    # collinear
                  [0.3, -0.4, 1.05], [0.3, -0.4, 1.05], [0.6, 0.2, 1.05],  # two equal vertices
                  [-0.2, 0.3, 1.2], [0.1, 0.3, 1.2], [-0.2, 0.6, 1.2]],  # a proper one on top
                 np.float32).reshape(4, 9)
    n = np.tile(np.array([0, 0, 1], np.float32), (4, 3))
    uv = np.zeros((4, 6), np.float32)
    return dataclasses.replace(s, name="sphere_degenerate", pos=np.concatenate([s.pos, v]),
                               nrm=np.concatenate([s.nrm, n]), uv=np.concatenate([s.uv, uv]),
                               mat=np.concatenate([s.mat, np.zeros(4, s.mat.dtype)]))


def one_triangle():
    s = scenes.get_scene("sphere")
    pos = np.array([[-1, -1, 0, 1, -1, 0, 0, 1, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (1, 3))
    return dataclasses.replace(s, name="one_triangle", pos=pos, nrm=nrm,
                               uv=np.zeros((1, 6), np.float32), mat=np.zeros(1, s.mat.dtype))


def cornell_inside():
    s = scenes.get_scene("cornell")
    lo = s.pos.reshape(-1, 3).min(0)
    hi = s.pos.reshape(-1, 3).max(0)
    mid = (lo + hi) / 2
    eye = mid + (hi - lo) * np.array([0.1, 0.15, 0.2])
    return with_camera(s, tuple(float(x) for x in eye), tuple(float(x) for x in lo), 70.0)


def far_vertex(scale):
    """The sphere with one vertex moved to (scale, scale, scale): the
    triangles around it get edge components near `scale` (Moller-Trumbore
    dets up to ~scale^2, past the short reciprocal's 2^126 from 2^62 on)."""
    s = scenes.get_scene("sphere")
    pos = s.pos.astype(np.float32).copy()
    pos[0, 0:3] = np.float32(scale)
    return dataclasses.replace(s, name=f"far_vertex_{scale}", pos=pos)


def far_floor(scale):
    """The sphere over a floor triangle with edges of 2 * scale, facing up
    (y = -1.5): Moller-Trumbore's det for a ray down onto it is
    4 scale^2 |d.y|, so from scale 2^62 on the bounce rays that hit it have
    dets of 2^124 .. 2^128 and past (the short reciprocal's 2^126 limit, the
    subnormal reciprocals, the overflow to inf)."""
    s = scenes.get_scene("sphere")
    S = np.float32(scale)
    tri = np.array([[-S, -1.5, -S, 0, -1.5, S, S, -1.5, -S]], np.float32)
    n = np.tile(np.array([0, 1, 0], np.float32), (1, 3))
    return dataclasses.replace(s, name=f"far_floor_{scale}", pos=np.concatenate([s.pos, tri]),
                               nrm=np.concatenate([s.nrm, n]), uv=np.concatenate([s.uv, np.zeros((1, 6), np.float32)]),
                               mat=np.concatenate([s.mat, np.zeros(1, s.mat.dtype)]))


# (scene, scale, needs the IEEE-division kernels)
FAR = [("vertex", 2.0 ** 40, False), ("vertex", 2.0 ** 62, True), ("vertex", 2.0 ** 64, True),
       ("vertex", 2.0 ** 100, True), ("vertex", float("inf"), True), ("vertex", float("nan"), False),
       ("floor", 2.0 ** 40, False), ("floor", 2.0 ** 62, True), ("floor", 2.0 ** 63, True),
       ("floor", 2.0 ** 64, True)]
FAR_IDS = [f"{k}-2^{int(np.log2(s))}" if np.isfinite(s) else f"{k}-{s}" for k, s, _ in FAR]


def far_scene(kind, scale):
    return far_vertex(scale) if kind == "vertex" else far_floor(scale)


def hand_scene():
    """An 8^3-cell box [0, 8]^3: axis-aligned floor (y = 0) and back wall
    (z = 0), a corner triangle pinning the bbox, 32 small triangles inside
    cell (2, 3, 2) and 33 inside cell (5, 3, 5) (one of them zero-area), and a
    coincident pair of opposite-facing triangles."""
    s = scenes.get_scene("cornell")
    tris = []
    quad = lambda a, b, c, d: [a + b + c, a + c + d]
    tris += quad([0, 0, 0], [0, 0, 8], [8, 0, 8], [8, 0, 0])            # floor, normal +y
    tris += quad([0, 0, 0], [8, 0, 0], [8, 8, 0], [0, 8, 0])            # back wall, normal +z
    tris += [[8, 8, 8, 7.5, 8, 8, 8, 8, 7.5]]                            # bbox corner
    rng = np.random.default_rng(5)

    def cluster(cell, n):
        out = []
        c = np.array(cell, np.float64) + 0.5
        for _ in range(n):
            p = c + rng.uniform(-0.25, 0.25, 3)
            out.append(list(np.concatenate([p, p + rng.uniform(-0.15, 0.15, 3), p + rng.uniform(-0.15, 0.15, 3)])))
        return out
    tris += cluster((2, 3, 2), 32)
    c33 = cluster((5, 3, 5), 33)
    c33[7][3:6] = c33[7][0:3]                                           # zero area: v1 = v0
    tris += c33
    pair = [3.2, 2.2, 6.3, 4.7, 2.4, 6.4, 3.9, 3.6, 6.2]
    tris += [pair, pair[0:3] + pair[6:9] + pair[3:6]]                   # the same triangle, both windings
    pos = np.array(tris, np.float32).reshape(-1, 9)
    n = len(pos)
    e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
    nr = np.cross(e1, e2)
    ln = np.linalg.norm(nr, axis=1, keepdims=True)
    nr = np.where(ln > 0, nr / np.maximum(ln, 1e-30), np.array([0, 1, 0])).astype(np.float32)
    cam = scenes.CameraDef("Hand", scenes.look_at((4.0, 4.0, 14.0), (4.0, 4.0, 0.0)), math.radians(45.0), None)
    return dataclasses.replace(s, name="bfcull_hand", pos=pos, nrm=np.tile(nr, (1, 3)).astype(np.float32),
                               uv=np.zeros((n, 6), np.float32),
                               mat=(np.arange(n) % s.num_materials).astype(s.mat.dtype), cameras=[cam])
