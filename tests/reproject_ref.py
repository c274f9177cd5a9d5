"""The contract of zrt_context_reproject (include/zrt.h) in numpy float32,
operation by operation, left to right as the header writes it.  numpy's
elementwise float32 + - * /, np.sqrt, np.floor and np.abs are the IEEE
operations and never fuse, so the result is the bits the header specifies.  The
four taps are a Python loop; each tap is whole-image array arithmetic, a
skipped tap a mask.

Nothing here depends on anything but numpy.  It is the reference of
test_reproject_host.py and test_reproject_gpu.py and is never checked against a
GPU result of this tree as truth.
"""
import collections

import numpy as np

F = np.float32
ONE, ZERO, HALF = F(1.0), F(0.0), F(0.5)
INF = F(np.inf)
NAN = np.array([0x7FC00000], np.uint32).view(F)[0]

Cam = collections.namedtuple("Cam", "w h origin llc right up")


def cam_of(c):
    """A Cam (float32 vectors) of a native.Camera, an oracle camera or a Cam."""
    llc = c.lower_left_corner if hasattr(c, "lower_left_corner") else c.llc
    return Cam(int(c.w), int(c.h), *(np.array(list(v), F) for v in (c.origin, llc, c.right, c.up)))


def moved(c, translate=(0.0, 0.0, 0.0), yaw=0.0):
    """The camera `c` with its origin moved by `translate` and its frame turned
    by `yaw` radians about the world y axis (float32 results of float64
    arithmetic: a camera is an input, not part of the contract)."""
    c = cam_of(c)
    cs, sn = np.cos(yaw), np.sin(yaw)
    rot = np.array([[cs, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, cs]])
    turn = lambda v: (rot @ v.astype(np.float64)).astype(F)
    return Cam(c.w, c.h, (c.origin.astype(np.float64) + np.array(translate, np.float64)).astype(F), turn(c.llc),
               turn(c.right), turn(c.up))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def constants(prev):
    """(A, B, Cv, usable) of the previous camera."""
    with np.errstate(all="ignore"):
        A, B, Cv = _cross(prev.up, prev.llc), _cross(prev.llc, prev.right), _cross(prev.right, prev.up)
        D = _dot(prev.llc, Cv)
        if D < ZERO:
            A, B, Cv = -A, -B, -Cv
    assert A.dtype == F and D.dtype == F
    return A, B, Cv, bool(D < ZERO or D > ZERO)


def project(cam, prev, depth):
    """(defined (h, w) bool, a, b, zq (h, w) float32, px, py) of every pixel."""
    h, w = cam.h, cam.w
    A, B, Cv, usable = constants(prev)
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = xs.astype(F) + HALF, ys.astype(F) + HALF
    z = np.ascontiguousarray(depth, F).reshape(h, w)
    with np.errstate(all="ignore"):
        v = (cam.llc + cam.right * px[..., None]) + cam.up * py[..., None]
        d = v * (ONE / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]))[..., None]
        X = cam.origin + d * z[..., None]
        q = X - prev.origin
        g = _dot(q, Cv)
        a, b = _dot(q, A) / g, _dot(q, B) / g
        zq = np.sqrt(_dot(q, q))
        defined = (z > ZERO) & (z < INF) & (g > ZERO) & usable
    assert all(t.dtype == F for t in (v, d, q, g, a, b, zq))
    return defined, a, b, zq, px, py


def reproject(cam, prev, color, depth, prev_color, prev_depth, normal=None, prev_normal=None, prev_length=None,
              max_history=32, depth_tolerance=0.05, normal_tolerance=0.5):
    """Row-major planes: color, prev_color, normal, prev_normal (h, w, 3),
    depth, prev_depth (h, w) float32, prev_length (h, w) uint32 ->
    {"color" (h, w, 3) float32, "length" (h, w) uint32, "motion" (h, w, 2)
    float32, "has" (h, w) bool: W > 0, "hits": their number}."""
    cam, prev = cam_of(cam), cam_of(prev)
    h, w = cam.h, cam.w
    assert (prev.h, prev.w) == (h, w) and 1 <= max_history <= 65535
    c = np.ascontiguousarray(color, F).reshape(h, w, 3)
    pc = np.ascontiguousarray(prev_color, F).reshape(h, w, 3)
    pd = np.ascontiguousarray(prev_depth, F).reshape(h, w)
    nrm = normal is not None and prev_normal is not None
    if nrm:
        n = np.ascontiguousarray(normal, F).reshape(h, w, 3)
        pn = np.ascontiguousarray(prev_normal, F).reshape(h, w, 3)
        tn2 = F(normal_tolerance) * F(normal_tolerance)
    pl = None if prev_length is None else np.ascontiguousarray(prev_length, np.uint32).reshape(h, w)
    defined, a, b, zq, px, py = project(cam, prev, depth)
    with np.errstate(all="ignore"):
        motion = np.stack([a - px, b - py], axis=-1)
        motion[~defined] = NAN
        fx, fy = a - HALF, b - HALF
        ok = defined & (fx > -ONE) & (fx < F(w)) & (fy > -ONE) & (fy < F(h))
        x0 = np.floor(np.where(ok, fx, ZERO)).astype(np.int64)
        y0 = np.floor(np.where(ok, fy, ZERO)).astype(np.int64)
        tx, ty = fx - x0.astype(F), fy - y0.astype(F)
        S = np.zeros((h, w, 3), F)
        W = np.zeros((h, w), F)
        M = np.full((h, w), 0xFFFFFFFF, np.uint32)
        ztol = F(depth_tolerance) * zq
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                m = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                bw = (tx if i else ONE - tx) * (ty if j else ONE - ty)
                m &= bw > ZERO
                at = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
                zp = pd[at]
                m &= zp > ZERO
                m &= np.abs(zp - zq) <= ztol
                if nrm:
                    dn = n - pn[at]
                    m &= ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) <= tn2
                cp = pc[at]
                m &= np.isfinite(cp).all(axis=-1)
                lp = np.ones((h, w), np.uint32) if pl is None else pl[at]
                m &= lp != 0
                S[m] = (S + cp * bw[..., None])[m]             # a skipped tap leaves S, W and M as they are
                W[m] = (W + bw)[m]
                M[m] = np.minimum(M, lp)[m]
        has = W > ZERO
        N = np.where(has, np.minimum(M, np.uint32(max_history - 1)) + np.uint32(1), np.uint32(1)).astype(np.uint32)
        alpha = ONE / N.astype(F)
        hist = S / np.where(has, W, ONE)[..., None]
        blended = (hist * (ONE - alpha)[..., None]) + (c * alpha[..., None])
        out = c.copy()                                         # no history, or N == 1: the input's bits
        use = has & (N > 1)
        out[use] = blended[use]
    assert out.dtype == F and motion.dtype == F and blended.dtype == F
    return {"color": out, "length": N, "motion": motion, "has": has, "hits": int(has.sum())}


def reproject_packed(pix, cam, prev, color, depth, prev_color, prev_depth, normal=None, prev_normal=None,
                     prev_length=None, **kw):
    """The same over planes in packed order (pix: packed k -> row-major pixel,
    zrt_tile_pixels(w, h, tile, 0, 1)); None: the planes are row-major already.
    Returns "color" (P, 3), "length" (P,), "motion" (P, 2) in the planes' order, and "hits"."""
    cam = cam_of(cam)
    w, h = cam.w, cam.h

    def img(a, ch, dt=F):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt).reshape(w * h, ch)
        if pix is not None:
            full = np.empty_like(a)
            full[pix] = a
            a = full
        return a.reshape((h, w, ch) if ch > 1 else (h, w))

    r = reproject(cam, prev, img(color, 3), img(depth, 1), img(prev_color, 3), img(prev_depth, 1), img(normal, 3),
                  img(prev_normal, 3), img(prev_length, 1, np.uint32), **kw)
    order = slice(None) if pix is None else pix
    return {"color": r["color"].reshape(-1, 3)[order], "length": r["length"].reshape(-1)[order],
            "motion": r["motion"].reshape(-1, 2)[order], "hits": r["hits"]}
