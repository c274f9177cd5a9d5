"""Scene.traceRay (stage3.zig:152-186) for one ray, composed from the CPU
oracle's unit entry points -- the reference of the ray-query tests
(test_trace_host.py, test_trace_gpu.py); not a test module itself.

    OracleScene(soup, res).baked()   cells and Geometry.indices
    oracle.grid_trace                the first cell, then the cell and the
                                     crossing t of every Iterator.next()
    oracle.tri_intersect             Moller-Trumbore on the SOURCE triangle
                                     soup.pos[indices[ref]]

with the reference's rules: the cells in walk order, a cell's refs begin ->
end, a hit kept if `t < nearest and t > 0`, the walk stopped once
`nearest <= t_next`.  Also counts the cells visited and the refs tested, as
the oracle's render counts them (zrt_oracle.c trace(): one per cell entered,
one per ref tried).
"""
import numpy as np

MISS = 0xFFFFFFFF
INF = np.float32(np.inf)


class RayRef:
    """The baked scene of (soup, res) and trace(o, d) against it."""

    def __init__(self, orc, soup, res):
        self.orc = orc
        self.res = tuple(int(r) for r in res)
        self.scene = orc.OracleScene(soup, self.res)
        gb, cs, cells, idx = self.scene.baked()
        self.bmin, self.bmax, self.cs = gb[:3].copy(), gb[3:].copy(), cs
        self.cells, self.indices = cells, idx
        self.pos = np.ascontiguousarray(soup.pos, np.float32).reshape(-1, 9)
        self.max_steps = sum(self.res) + 1

    def trace(self, o, d):
        """((t, u, v) float32, ref, cells visited, refs tested); a miss is
        ((+inf, 0, 0), MISS, ...)."""
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        walk = self.orc.grid_trace(self.bmin, self.bmax, self.res, o, d, self.max_steps)
        best = (INF, np.float32(0), np.float32(0))
        ref = MISS
        if walk is None:                                   # the ray misses the grid's bbox
            return best, ref, 0, 0
        first, nxt, ts = walk
        assert len(ts) < self.max_steps and ts[-1] == INF, "max_steps reached"
        rx, ry, _ = self.res
        n_cells = n_tests = 0
        cell = first
        asked = {}       # source triangle -> the oracle's answer for this ray (a triangle sits in many cells)
        for k in range(len(ts)):
            b, e = self.cells[(int(cell[2]) * ry + int(cell[1])) * rx + int(cell[0])]
            n_cells += 1
            for r in range(int(b), int(e)):
                n_tests += 1
                src = int(self.indices[r])
                if src not in asked:
                    tri = self.pos[src]
                    asked[src] = self.orc.tri_intersect(tri[0:3], tri[3:6], tri[6:9], o, d)
                hit, tuv = asked[src]
                if hit and tuv[0] < best[0] and tuv[0] > 0:    # stage3.zig:172: strict, the first ref wins a tie
                    best = (tuv[0], tuv[1], tuv[2])
                    ref = r
            if best[0] <= ts[k]:                           # stage3.zig:179-182
                break
            cell = nxt[k]
        return best, ref, n_cells, n_tests

    def trace_batch(self, origins, dirs):
        """A (n, 4) uint32 array of the bit patterns (t, u, v, ref) and the
        batch's (cells visited, refs tested, hits)."""
        out = np.zeros((len(origins), 4), np.uint32)
        cells = tests = hits = 0
        for i, (o, d) in enumerate(zip(origins, dirs)):
            (t, u, v), ref, nc, nt = self.trace(o, d)
            out[i, :3] = np.array([t, u, v], np.float32).view(np.uint32)
            out[i, 3] = ref
            cells += nc
            tests += nt
            hits += ref != MISS
        return out, (cells, tests, hits)


def hit_bits(res):
    """Context.trace's numpy result as the (n, 4) uint32 array of trace_batch."""
    return np.stack([res["t"].view(np.uint32), res["u"].view(np.uint32), res["v"].view(np.uint32),
                     res["triangle"]], axis=1)
