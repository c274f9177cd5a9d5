"""Scene.traceRay (stage3.zig:152-186) with nearest_hit.t initialised to a
bound t_max instead of +inf (stage3.zig:154) -- the reference of the segment
query tests (test_segments_host.py, test_segments_gpu.py); not a test module
itself.

Built on a trace_ref.RayRef: the same composed loop over the oracle's unit
entry points (grid_trace, tri_intersect), with `best` starting at
np.float32(t_max) and, in any-hit form, the walk left after the first cell in
which a ref was kept.  Nothing else changes: a ref is kept if `t < nearest and
t > 0` (so t == t_max is not), the first cell is always tested, the walk stops
once `nearest <= t_next` and in any case at the grid's exit (a NaN bound makes
no comparison true).  A miss is normalised to ((+inf, 0, 0), MISS) whatever the
bound was.
"""
import numpy as np

from trace_ref import INF, MISS


def segment(ref, o, d, t_max, any_hit=False, cache=None):
    """((t, u, v) float32, ref, cells visited, refs tested) of ray (o, d)
    bounded by t_max against the RayRef `ref`.  `cache`: a dict of this ray's
    own, which keeps the oracle's answers (the walk, the triangle tests) for
    further bounds of the same ray."""
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    miss = (INF, np.float32(0), np.float32(0))
    cache = {} if cache is None else cache
    if "walk" not in cache:
        cache["walk"] = ref.orc.grid_trace(ref.bmin, ref.bmax, ref.res, o, d, ref.max_steps)
        cache["asked"] = {}
    walk = cache["walk"]
    if walk is None:                                       # the ray misses the grid's bbox
        return miss, MISS, 0, 0
    first, nxt, ts = walk
    assert len(ts) < ref.max_steps and ts[-1] == INF, "max_steps reached"
    rx, ry, _ = ref.res
    nearest = np.float32(t_max)
    best, kept = miss, MISS
    n_cells = n_tests = 0
    cell = first
    asked = cache["asked"]     # source triangle -> the oracle's answer for this ray
    for k in range(len(ts)):
        b, e = ref.cells[(int(cell[2]) * ry + int(cell[1])) * rx + int(cell[0])]
        n_cells += 1
        kept_here = False
        for r in range(int(b), int(e)):
            n_tests += 1
            src = int(ref.indices[r])
            if src not in asked:
                tri = ref.pos[src]
                asked[src] = ref.orc.tri_intersect(tri[0:3], tri[3:6], tri[6:9], o, d)
            hit, tuv = asked[src]
            if hit and tuv[0] < nearest and tuv[0] > 0:    # stage3.zig:172: strict
                nearest = np.float32(tuv[0])
                best = (tuv[0], tuv[1], tuv[2])
                kept = r
                kept_here = True
        if nearest <= ts[k]:                               # stage3.zig:179-182
            break
        if any_hit and kept_here:                          # any mode: the answer is known
            break
        cell = nxt[k]
    return best, kept, n_cells, n_tests


def segment_batch(ref, origins, dirs, t_max, any_hit=False, caches=None):
    """A (n, 4) uint32 array of the bit patterns (t, u, v, ref), the batch's
    (cells visited, refs tested, hits) and the cells visited per ray; t_max a
    scalar or (n,).  `caches`: a list of n dicts (see segment)."""
    n = len(origins)
    caches = [None] * n if caches is None else caches
    tm = np.broadcast_to(np.asarray(t_max, np.float32), (n,))
    out = np.zeros((n, 4), np.uint32)
    per_ray_cells = np.zeros(n, np.int64)
    cells = tests = hits = 0
    for i, (o, d) in enumerate(zip(origins, dirs)):
        (t, u, v), r, nc, nt = segment(ref, o, d, tm[i], any_hit, caches[i])
        out[i, :3] = np.array([t, u, v], np.float32).view(np.uint32)
        out[i, 3] = r
        per_ray_cells[i] = nc
        cells += nc
        tests += nt
        hits += r != MISS
    return out, (cells, tests, int(hits)), per_ray_cells
