"""The per-ray contract of zrt_context_occlusion (include/zrt.h) -- the
reference of the occlusion tests (test_occlusion_host.py,
test_occlusion_gpu.py); not a test module itself.

Composed from what the suite already trusts, in numpy float32 scalars in the
contract's order:

    trace_ref.RayRef.trace          the first hit h of the ray
    surface_ref.surface_ref         the zrt_surface r of (ray, h): the normal as
                                    interpolated (words 4:7), the position
                                    (words 0:3)
    oracle.path_norm(seed, key, s, 3)   the first three floatNorm draws of the
                                    stream (seed, key, s)
    normalize(x) = x * (1 / sqrt((x0 x0 + x1 x1) + x2 x2))
    d_s = normalize(r.normal + normalize(draws))
    segment_ref.segment             the closest-mode segment (r.position, d_s,
                                    radius): occluded iff it is a hit

A sample is traced iff r.position and d_s are finite and d_s is not all zero;
one that is not traced is unoccluded and costs nothing.  The samples of a ray
are kept with their segment caches (the walk and the triangle answers), so a
further radius or the any-hit counting walk of the same sample asks the oracle
nothing new, and the counts at S' < S samples are prefixes.
"""
import numpy as np

import segment_ref
import surface_ref
from trace_ref import MISS

F = np.float32
S_MAX = 5                      # samples the fuzz cases keep per ray


def normalize(x):
    """x * (1.0f / sqrt((x.x*x.x + x.y*x.y) + x.z*x.z)), float32 throughout."""
    x = [F(v) for v in x]
    with np.errstate(all="ignore"):
        n2 = F(F(F(x[0] * x[0]) + F(x[1] * x[1])) + F(x[2] * x[2]))
        inv = F(F(1.0) / np.sqrt(n2, dtype=F))
        return np.array([F(v * inv) for v in x], F)


def direction(orc, normal, seed, key, s):
    """d_s of the contract for the interpolated normal `normal` (3 float32)."""
    draws = orc.path_norm(int(seed) & 0xFFFFFFFFFFFFFFFF, int(key) & 0xFFFFFFFF, int(s), 3)
    with np.errstate(all="ignore"):
        u = normalize(draws)
        return normalize([F(F(normal[k]) + u[k]) for k in range(3)])


def is_traced(pos, d):
    return bool(np.isfinite(pos).all() and np.isfinite(d).all() and (np.asarray(d) != 0).any())


class Sample:
    """One (ray, sample) item: its segment's origin and direction, whether it
    is traced, and the cache segment_ref.segment keeps for it."""

    def __init__(self, pos, d):
        self.pos, self.d = pos, d
        self.traced = is_traced(pos, d)
        self.cache = {}

    def closest(self, ref, radius):
        """((t, u, v), ref) of the closest-mode segment under `radius`."""
        best, r, _, _ = segment_ref.segment(ref, self.pos, self.d, radius, False, self.cache)
        return best, r

    def occluded(self, ref, radius):
        return self.traced and self.closest(ref, radius)[1] != MISS

    def any_counts(self, ref, radius):
        """(cells, tests) of the counting any-hit segment call's walk."""
        _, _, nc, nt = segment_ref.segment(ref, self.pos, self.d, radius, True, self.cache)
        return nc, nt


def ray_samples(ref, soup, o, d, hit_bits, seed, key, S):
    """The S samples of one ray whose trace record is `hit_bits` ((t, u, v, ref)
    patterns); [] for a miss."""
    if int(hit_bits[3]) == MISS:
        return []
    words = surface_ref.surface_ref(ref, soup, o, d, hit_bits)
    f = words.view(F)
    pos, nrm = f[0:3].copy(), f[4:7].copy()
    return [Sample(pos, direction(ref.orc, nrm, seed, key, s)) for s in range(S)]


def visibility(occluded, S):
    """(float)(S - occluded) / (float)S by the IEEE division, as float32."""
    occluded = np.asarray(occluded, np.uint32)
    return ((np.uint32(S) - occluded).astype(F) / F(S)).astype(F)


def cached_samples(cs):
    """The samples of a fuzz seed's rays -- S_MAX per ray, key = the ray's
    index, seed = cs.rseed -- computed once and kept on the case."""
    if not hasattr(cs, "_occlusion_samples"):
        cs._occlusion_samples = [ray_samples(cs.ref, cs.soup, cs.o[i], cs.d[i], cs.bits[i], cs.rseed, i, S_MAX)
                                 for i in range(len(cs.o))]
    return cs._occlusion_samples


def fuzz_radius(soup):
    """The radius of the fuzz cases: f32(0.25 x the soup's bounding-box diagonal)."""
    p = np.asarray(soup.pos, np.float64).reshape(-1, 3)
    return F(0.25 * float(np.linalg.norm(p.max(0) - p.min(0))))


def occlusion_batch(ref, samples, radius, S, counts=False):
    """(occluded (n,) uint32, visibility bits (n,) uint32, traced samples,
    (cells, tests) of the samples' counting any-hit walks or None) for the
    first S samples of every ray of `samples` (ray_samples' lists); radius a
    scalar or (n,)."""
    n = len(samples)
    rad = np.broadcast_to(np.asarray(radius, F), (n,))
    occ = np.zeros(n, np.uint32)
    traced = cells = tests = 0
    for i, smp in enumerate(samples):
        for x in smp[:S]:
            if not x.traced:
                continue
            traced += 1
            occ[i] += x.occluded(ref, rad[i])
            if counts:
                nc, nt = x.any_counts(ref, rad[i])
                cells += nc
                tests += nt
    return occ, visibility(occ, S).view(np.uint32).copy(), traced, ((cells, tests) if counts else None)
