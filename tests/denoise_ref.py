"""The contract of zrt_context_denoise (include/zrt.h) in numpy float32: the
edge-avoiding a-trous filter, operation by operation, left to right as the
header writes it.  numpy's elementwise float32 + - * / are the IEEE operations
and never fuse, np.fmax is C's fmaxf (a NaN operand gives the other operand),
so the result is the bits the header specifies.  The 25 taps are a Python
loop; each tap is whole-image array arithmetic, a skipped tap a mask.

Nothing here depends on anything but numpy.  It is the reference of
test_denoise_host.py and test_denoise_gpu.py and is never checked against a
GPU result of this tree as truth.
"""
import numpy as np

F = np.float32
H = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))      # (1/16, 1/4, 3/8, 1/4, 1/16)
ZMIN = F(2.0 ** -20)                                        # 0x1p-20f
ONE, ZERO = F(1.0), F(0.0)


def _weight(x2, k):
    """fmaxf(1 - x2 * k, 0)^2"""
    w = np.fmax(ONE - x2 * k, ZERO)
    return w * w


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _shifted(plane, dx, dy):
    """(the centre window, the tap window) of `plane` for the tap offset
    (dx, dy): views over the pixels whose tap lies inside the image."""
    h, w = plane.shape[:2]
    x0, x1 = max(0, -dx), min(w, w - dx)
    y0, y1 = max(0, -dy), min(h, h - dy)
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def level(c, step, kc, normal=None, kn=None, depth=None, kz=None, albedo=None, ka=None):
    """One level: c (h, w, 3) float32 -> the next colour frame."""
    h, w = c.shape[:2]
    S = np.zeros((h, w, 3), F)
    W = np.zeros((h, w), F)
    iz = None if depth is None else ONE / np.fmax(depth, ZMIN)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                if abs(ox) >= w or abs(oy) >= h:
                    continue                                 # outside for every pixel
                P, Q = _shifted(c, ox, oy)
                k = H[dx + 2] * H[dy + 2]
                wt = k * _weight(_dist2(c[P], c[Q]), kc)
                if normal is not None:
                    wt = wt * _weight(_dist2(normal[P], normal[Q]), kn)
                if depth is not None:
                    r = (depth[P] - depth[Q]) * iz[P]
                    wt = wt * _weight(r * r, kz)
                if albedo is not None:
                    wt = wt * _weight(_dist2(albedo[P], albedo[Q]), ka)
                keep = wt > ZERO                              # NaN: not kept
                wt = np.where(keep, wt, ZERO)
                add = c[Q] * wt[..., None]
                Sp, Wp = S[P], W[P]
                Sp[keep] = (Sp + add)[keep]                   # a skipped tap leaves S and W as they are
                Wp[keep] = (Wp + wt)[keep]
        some = W > ZERO
        out = c.copy()                                       # W == 0: the input's bits
        out[some] = (S / np.where(some, W, ONE)[..., None])[some]
    return out


def denoise(color, iterations, sigma_color, normal=None, sigma_normal=None, depth=None, sigma_depth=None,
            albedo=None, sigma_albedo=None):
    """color (h, w, 3), normal (h, w, 3), depth (h, w), albedo (h, w, 3), all
    row-major float32 (guides may be None) -> c_iterations (h, w, 3) float32."""
    assert 1 <= iterations <= 8
    c = np.ascontiguousarray(color, F)
    assert c.ndim == 3 and c.shape[2] == 3
    g = {}
    with np.errstate(all="ignore"):
        if normal is not None:
            g["normal"] = np.ascontiguousarray(normal, F).reshape(c.shape)
            g["kn"] = ONE / (F(sigma_normal) * F(sigma_normal))
        if depth is not None:
            g["depth"] = np.ascontiguousarray(depth, F).reshape(c.shape[:2])
            g["kz"] = ONE / (F(sigma_depth) * F(sigma_depth))
        if albedo is not None:
            g["albedo"] = np.ascontiguousarray(albedo, F).reshape(c.shape)
            g["ka"] = ONE / (F(sigma_albedo) * F(sigma_albedo))
        for i in range(iterations):
            s = F(sigma_color) * F(2.0 ** -i)                # exact
            c = level(c, 1 << i, ONE / (s * s), **g)
    return c


def denoise_packed(pix, w, h, color, iterations, sigma_color, normal=None, sigma_normal=None, depth=None,
                   sigma_depth=None, albedo=None, sigma_albedo=None):
    """The same over planes in packed order (pix: packed k -> row-major pixel,
    zrt_tile_pixels(w, h, tile, 0, 1)); None: the planes are row-major already.
    Returns linear (P, 3) in the planes' order."""
    def img(a, ch):
        if a is None:
            return None
        a = np.ascontiguousarray(a, F).reshape(w * h, ch)
        if pix is not None:
            full = np.empty_like(a)
            full[pix] = a
            a = full
        return a.reshape((h, w, ch) if ch == 3 else (h, w))

    out = denoise(img(color, 3), iterations, sigma_color, img(normal, 3), sigma_normal, img(depth, 1), sigma_depth,
                  img(albedo, 3), sigma_albedo).reshape(w * h, 3)
    return out if pix is None else out[pix]


def b3_blur(c):
    """The plain separable 5-tap B3 blur of c (h, w, 3) in float64, taps outside
    the image dropped without renormalising (callers compare interior pixels)."""
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    a = np.asarray(c, np.float64)
    h, w = a.shape[:2]
    t = np.zeros_like(a)
    for d in range(-2, 3):
        x0, x1 = max(0, -d), min(w, w - d)
        t[:, x0:x1] += k[d + 2] * a[:, x0 + d:x1 + d]
    o = np.zeros_like(a)
    for d in range(-2, 3):
        y0, y1 = max(0, -d), min(h, h - d)
        o[y0:y1] += k[d + 2] * t[y0 + d:y1 + d]
    return o
