"""The contract of zrt_context_sky_light (include/zrt.h) -- the reference of
the sky-light tests (test_sky_light_host.py, test_sky_light_gpu.py); not a
test module itself.

In numpy float32 scalars, in the contract's order, composed from what the suite
already trusts:

    trace_ref.RayRef.trace          the first hit h of the ray
    surface_ref.surface_ref         the zrt_surface r of (ray, h)
    oracle.path_norm                the three floatNorm draws of a sample's stream
    direct_ref.normalize_rn, dot    N and d_s = normalize_rn(N + normalize_rn(draws))
    env_color (below)               getEnvColor, operation by operation; the host
                                    test holds it to oracle.env_color as bits
    transmit_ref.chain              the chain of (r.position, d_s, +inf)

An item keeps its chain, so a further cap, the unshadowed call and the counting
call of the same item walk nothing again.
"""
import numpy as np

import surface_ref
import transmit_ref
from direct_ref import normalize_rn
from trace_ref import MISS

F = np.float32
CAP = 16
PI = F(np.uint32(0x40490FDB).view(F))          # 0x1.921fb6p+1f
MAX64 = 2 ** 64 - 1
SKY_C = (F(0.5), F(0.7), F(1.0))


def env_color(d):
    """stage3.zig:144-150: t = 0.5f * (d.y + 1.0f); L.k = (1.0f - t) + c_k * t."""
    with np.errstate(all="ignore"):
        t = F(F(0.5) * F(F(d[1]) + F(1.0)))
        return np.array([F(F(F(1.0) - t) + F(c * t)) for c in SKY_C], F)


class Item:
    """One (ray, sample) item: d_s, whether it is traced, L_s, and its chain
    once walked."""

    def __init__(self, orc, pos, N, seed, key, s):
        draws = orc.path_norm(int(seed) & MAX64, int(key) & 0xFFFFFFFF, int(s), 3)
        with np.errstate(all="ignore"):
            u = normalize_rn(draws)
            self.d = normalize_rn([F(N[k] + u[k]) for k in range(3)])
        self.traced = bool(np.isfinite(self.d).all() and (self.d != 0).any())
        self.L = env_color(self.d)
        self.pos = pos
        self._chain = None

    def chain(self, ref, soup):
        if self._chain is None:
            self._chain = transmit_ref.chain(ref, soup, self.pos, self.d, np.inf, CAP)
        return self._chain


class Ray:
    """One ray: its surface words (None: a miss), whether it is shaded, and its
    items in sample order ([] unless shaded)."""

    def __init__(self, orc, ref, soup, o, d, hit_bits, spp, seed, key):
        self.items, self.shaded, self.words = [], False, None
        if int(hit_bits[3]) == MISS:
            return
        self.words = surface_ref.surface_ref(ref, soup, o, d, hit_bits)
        f = self.words.view(F)
        pos = f[0:3].copy()
        with np.errstate(all="ignore"):
            N = normalize_rn(f[4:7])
        self.N = N
        self.shaded = bool(np.isfinite(pos).all() and np.isfinite(N).all())
        if self.shaded:
            self.items = [Item(orc, pos, N, seed, key, s) for s in range(spp)]


def make_rays(orc, ref, soup, origins, dirs, bits, spp, seed=0, index_base=0):
    return [Ray(orc, ref, soup, origins[i], dirs[i], bits[i], spp, seed, index_base + i) for i in range(len(origins))]


def sky_batch(ref, soup, rays, spp, cap=CAP, unshadowed=False, counts=False):
    """(irradiance bits (n, 3) uint32, radiance bits (n, 3) uint32, visibility
    bits (n,) uint32, totals) of `rays` (Ray objects made with `spp` samples);
    the hit records are the ones the rays were made from.  totals =
    {"segments" (without the rays' own), "samples", "hits", "cells", "tests"},
    the last two the chains' counting walks (None without `counts`)."""
    n = len(rays)
    E = np.zeros((n, 3), F)
    R = np.zeros((n, 3), F)
    V = np.zeros(n, F)
    tot = dict(segments=0, samples=0, hits=0, cells=0 if counts else None, tests=0 if counts else None)
    fs = F(spp)
    with np.errstate(all="ignore"):
        for i, ray in enumerate(rays):
            if ray.words is None:
                continue
            a, v = [F(0), F(0), F(0)], F(0)
            for it in ray.items:
                if not it.traced:
                    continue
                tot["samples"] += 1
                T = F(1)
                if not unshadowed:
                    T, nx, segs, cells, tests, _ = it.chain(ref, soup).cut(cap)
                    T = F(T)
                    tot["segments"] += segs
                    tot["hits"] += nx
                    if counts:
                        tot["cells"] += cells
                        tot["tests"] += tests
                a = [F(a[k] + F(it.L[k] * T)) for k in range(3)]
                v = F(v + T)
            mean = [F(a[k] / fs) for k in range(3)]
            V[i] = F(v / fs)
            E[i] = [F(mean[k] * PI) for k in range(3)]
            f = ray.words.view(F)
            R[i] = [F(f[12 + k] + F(f[8 + k] * mean[k])) for k in range(3)] if ray.shaded else f[12:15]
    return E.view(np.uint32).copy(), R.view(np.uint32).copy(), V.view(np.uint32).copy(), tot
