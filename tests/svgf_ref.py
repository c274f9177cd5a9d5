"""The contracts of zrt_context_illumination and zrt_context_svgf
(include/zrt.h) in numpy float32: albedo demodulation and luminance moments,
the per-pixel variance estimate, and the variance-guided a-trous levels,
operation by operation, left to right as the header writes them.  numpy's
elementwise float32 + - * / and sqrt are the IEEE operations and never fuse,
np.fmax is C's fmaxf (a NaN operand gives the other operand), so the result is
the bits the header specifies.  The taps are a Python loop; each tap is
whole-image array arithmetic, a skipped tap a mask.

Nothing here depends on anything but numpy.  It is the reference of
test_svgf_host.py and test_svgf_gpu.py and is never checked against a GPU
result of this tree as truth.
"""
import numpy as np

F = np.float32
H = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))      # (1/16, 1/4, 3/8, 1/4, 1/16)
KK = ((F(0.0625), F(0.125), F(0.0625)), (F(0.125), F(0.25), F(0.125)), (F(0.0625), F(0.125), F(0.0625)))
ZMIN = F(2.0 ** -20)                                        # 0x1p-20f
AMIN = F(2.0 ** -4)                                         # 0x1p-4f: dmod's floor
EPS = F(2.0 ** -16)                                         # 0x1p-16f
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)
ONE, ZERO, FOUR = F(1.0), F(0.0), F(4.0)
INF = F(np.inf)


def lum(c):
    return (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]


def dmod(a):
    """fmaxf(a, 0x1p-4f) per component: a NaN albedo gives 0x1p-4f."""
    return np.fmax(np.asarray(a, F), AMIN)


def illumination(color, albedo=None):
    """color, albedo (..., 3) float32 in any one order -> (illumination
    (..., 3), moments (..., 3) = (l, l * l, +0))."""
    c = np.ascontiguousarray(color, F)
    with np.errstate(all="ignore"):
        I = c.copy() if albedo is None else c / dmod(albedo).reshape(c.shape)
        l = lum(I)
        m = np.zeros(c.shape, F)
        m[..., 0] = l
        m[..., 1] = l * l
    return I, m


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


def _guides(P, Q, normal, kn, depth, kz, iz):
    """wn * wz of the taps Q of the centres P; None with both guides absent."""
    wt = None
    if normal is not None:
        wt = _weight(_dist2(normal[P], normal[Q]), kn)
    if depth is not None:
        r = (depth[P] - depth[Q]) * iz[P]
        wz = _weight(r * r, kz)
        wt = wz if wt is None else wt * wz
    return wt


def variance0(c, moments=None, length=None, normal=None, kn=None, depth=None, kz=None):
    """The variance estimate: (v_0 (h, w) float32, temporal (h, w) bool: the
    pixels whose v_0 came from the moments)."""
    h, w = c.shape[:2]
    N = np.ones((h, w), np.uint32) if length is None else np.ascontiguousarray(length, np.uint32).reshape(h, w)
    temporal = (N >= 4) if moments is not None else np.zeros((h, w), bool)
    iz = None if depth is None else ONE / np.fmax(depth, ZMIN)
    S1, S2, W = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    l = lum(c)
    with np.errstate(all="ignore"):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                if abs(dx) >= w or abs(dy) >= h:
                    continue                                 # outside for every pixel
                P, Q = _shifted(c, dx, dy)
                wt = _guides(P, Q, normal, kn, depth, kz, iz)
                lq = l[Q]
                if wt is None:
                    wt = np.ones(lq.shape, F)
                keep = (wt > ZERO) & (np.abs(lq) < INF)       # NaN: not kept
                wt = np.where(keep, wt, ZERO)
                lq = np.where(keep, lq, ZERO)
                for acc, add in ((S1, lq * wt), (S2, (lq * lq) * wt), (W, wt)):
                    a = acc[P]
                    a[keep] = (a + add)[keep]                # a skipped tap leaves the sums as they are
        some = W > ZERO
        Ws = np.where(some, W, ONE)
        m1, m2 = S1 / Ws, S2 / Ws
        scale = FOUR / np.minimum(np.maximum(N, 1), 4).astype(F)
        spatial = np.where(some, np.fmax(m2 - m1 * m1, ZERO) * scale, ZERO)
        v = spatial
        if moments is not None:
            m = np.ascontiguousarray(moments, F).reshape(h, w, 3)
            v = np.where(temporal, np.fmax(m[..., 1] - m[..., 0] * m[..., 0], ZERO), spatial)
    return v.astype(F), temporal


def gauss3(v):
    """The 3 x 3 Gaussian of v at step 1, taps outside the image skipped."""
    h, w = v.shape
    Sg, Wg = np.zeros((h, w), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                if abs(dx) >= w or abs(dy) >= h:
                    continue
                P, Q = _shifted(v, dx, dy)
                kk = KK[dy + 1][dx + 1]
                Sg[P] = Sg[P] + v[Q] * kk
                Wg[P] = Wg[P] + kk
        return Sg / Wg


def level(c, v, step, sigma_luminance, normal=None, kn=None, depth=None, kz=None):
    """One level: c (h, w, 3), v (h, w) float32 -> (the next colour frame, the
    next variance plane)."""
    h, w = c.shape[:2]
    S = np.zeros((h, w, 3), F)
    W = np.zeros((h, w), F)
    V = np.zeros((h, w), F)
    iz = None if depth is None else ONE / np.fmax(depth, ZMIN)
    with np.errstate(all="ignore"):
        den = F(sigma_luminance) * np.sqrt(gauss3(v)) + EPS
        kl = ONE / (den * den)
        l = lum(c)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                if abs(ox) >= w or abs(oy) >= h:
                    continue                                 # outside for every pixel
                P, Q = _shifted(c, ox, oy)
                k = H[dx + 2] * H[dy + 2]
                dl = l[P] - l[Q]
                wt = k * _weight(dl * dl, kl[P])
                if normal is not None:                        # ((k * wl) * wn) * wz, in this order
                    wt = wt * _weight(_dist2(normal[P], normal[Q]), kn)
                if depth is not None:
                    r = (depth[P] - depth[Q]) * iz[P]
                    wt = wt * _weight(r * r, kz)
                keep = wt > ZERO                              # NaN: not kept
                wt = np.where(keep, wt, ZERO)
                Sp, Wp, Vp = S[P], W[P], V[P]
                Sp[keep] = (Sp + c[Q] * wt[..., None])[keep]
                Wp[keep] = (Wp + wt)[keep]
                Vp[keep] = (Vp + v[Q] * (wt * wt))[keep]
        some = W > ZERO
        Ws = np.where(some, W, ONE)
        oc, ov = c.copy(), v.copy()                          # W == 0: the input's bits
        oc[some] = (S / Ws[..., None])[some]
        ov[some] = (V / (Ws * Ws))[some]
    return oc, ov


def svgf(color, iterations, sigma_luminance, moments=None, length=None, normal=None, sigma_normal=None, depth=None,
         sigma_depth=None, albedo=None):
    """color, moments, normal, albedo (h, w, 3), depth (h, w) float32, length
    (h, w) uint32, all row-major (all but color may be None) -> {"linear"
    (h, w, 3), "variance" (h, w), "v0" (h, w), "temporal" (h, w) bool, "hits"}."""
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
        v0, temporal = variance0(c, moments, length, **g)
        v = v0
        for i in range(iterations):
            c, v = level(c, v, 1 << i, sigma_luminance, **g)
        if albedo is not None:
            c = c * dmod(albedo).reshape(c.shape)
    return {"linear": c, "variance": v, "v0": v0, "temporal": temporal, "hits": int(temporal.sum())}


def _image(a, pix, w, h, ch, dt=F):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dt).reshape(w * h, ch)
    if pix is not None:
        full = np.empty_like(a)
        full[pix] = a
        a = full
    return a.reshape((h, w, ch) if ch == 3 else (h, w))


def svgf_packed(pix, w, h, color, iterations, sigma_luminance, moments=None, length=None, normal=None,
                sigma_normal=None, depth=None, sigma_depth=None, albedo=None):
    """The same over planes in packed order (pix: packed k -> row-major pixel,
    zrt_tile_pixels(w, h, tile, 0, 1)); None: the planes are row-major already.
    Returns {"linear" (P, 3), "variance" (P,), "hits"} in the planes' order."""
    r = svgf(_image(color, pix, w, h, 3), iterations, sigma_luminance, _image(moments, pix, w, h, 3),
             _image(length, pix, w, h, 1, np.uint32), _image(normal, pix, w, h, 3), sigma_normal,
             _image(depth, pix, w, h, 1), sigma_depth, _image(albedo, pix, w, h, 3))
    lin, var = r["linear"].reshape(w * h, 3), r["variance"].reshape(w * h)
    if pix is not None:
        lin, var = lin[pix], var[pix]
    return {"linear": lin, "variance": var, "hits": r["hits"]}
