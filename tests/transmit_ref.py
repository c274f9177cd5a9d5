"""The pass-through chain of zrt_context_transmittance (include/zrt.h) -- the
reference of the transmittance tests (test_transmit_host.py,
test_transmit_gpu.py); not a test module itself.

Composed from the two references the suite already has, with numpy float32
scalars in the contract's order: segment_ref.segment (Scene.traceRay with
nearest starting at the bound, closest mode) finds each crossing,
surface_ref.surface_ref gives its transparency and the origin the reference
continues from (ray.at(t + eps)), and

    p = 1 - a;  !(p > 0): T = +0, stop;  T = T * min(p, 1);  n == cap: stop;
    b = b - (t + eps)

folds it in.  A chain records what every prefix of it answers, so the result
for a smaller cap is read off the chain of a larger one (cut).
"""
import numpy as np

import segment_ref
import surface_ref
from trace_ref import MISS

F = np.float32
EPS = surface_ref.EPS


class Chain:
    """One ray's chain under one bound and cap: T after each crossing, the
    cells and tests of each segment, the crossings' parameters along the
    ORIGINAL ray (float64 sums, for building bounds), and how it ended:
    "miss", "blocked" or "cap"."""

    def __init__(self):
        self.T_after, self.cells, self.tests, self.at = [], [], [], []
        self.end = None

    def cut(self, cap):
        """(T float32, n, segments, cells, tests, end) of this chain under the smaller cap `cap`."""
        n = len(self.T_after)
        if n >= cap:                                   # stopped at crossing `cap` (blocked there or cut)
            end = self.end if n == cap else "cap"
            return self.T_after[cap - 1], cap, cap, sum(self.cells[:cap]), sum(self.tests[:cap]), end
        T = self.T_after[-1] if n else F(1)
        return T, n, len(self.cells), sum(self.cells), sum(self.tests), self.end


def chain(ref, soup, o, d, t_max, cap):
    """The Chain of ray (o, d) bounded by t_max with at most `cap` crossings."""
    o_k = np.ascontiguousarray(o, F).copy()
    d = np.ascontiguousarray(d, F)
    b = F(t_max)
    T = F(1)
    c = Chain()
    base = 0.0
    with np.errstate(all="ignore"):
        while True:
            (t, u, v), r, nc, nt = segment_ref.segment(ref, o_k, d, b)
            c.cells.append(nc)
            c.tests.append(nt)
            if r == MISS:
                c.end = "miss"
                return c
            bits = np.array([F(t), F(u), F(v)], F).view(np.uint32)
            words = surface_ref.surface_ref(ref, soup, o_k, d, np.append(bits, np.uint32(r)))
            a = words.view(F)[7]
            c.at.append(base + float(t))
            p = F(1) - a
            if not (p > 0):
                c.T_after.append(F(0))
                c.end = "blocked"
                return c
            T = F(T * min(p, F(1)))
            c.T_after.append(T)
            if len(c.T_after) == cap:
                c.end = "cap"
                return c
            s = F(F(t) + EPS)
            base += float(s)
            o_k = words[0:3].view(F).copy()            # zrt_surface.position: o_k + d * s
            b = F(b - s)


CAP = 16


def cached_chains(cs):
    """The chains of a fuzz seed's rays (t_max = +inf, cap CAP), computed once
    and kept on the case."""
    if not hasattr(cs, "_transmit_chains"):
        cs._transmit_chains = [chain(cs.ref, cs.soup, cs.o[i], cs.d[i], np.inf, CAP) for i in range(len(cs.o))]
    return cs._transmit_chains


def transmit_batch(ref, soup, origins, dirs, t_max, cap, chains=None):
    """(T bits (n,) uint32, crossings (n,) uint32, (segments, cells, tests,
    hits) totals, the chains); t_max a scalar or (n,).  `chains`: those of a
    larger cap under the same bounds, cut instead of walked again."""
    n = len(origins)
    tm = np.broadcast_to(np.asarray(t_max, F), (n,))
    if chains is None:
        chains = [chain(ref, soup, origins[i], dirs[i], tm[i], cap) for i in range(n)]
    T = np.zeros(n, F)
    cr = np.zeros(n, np.uint32)
    tot = [0, 0, 0, 0]
    for i, c in enumerate(chains):
        T[i], cr[i], segs, cells, tests, _ = c.cut(cap)
        tot[0] += segs
        tot[1] += cells
        tot[2] += tests
        tot[3] += int(cr[i])
    return T.view(np.uint32).copy(), cr, tuple(tot), chains
