"""The per-probe contract of zrt_context_light_probes (include/zrt.h) -- the
reference of the light-probe tests (test_light_probes_host.py,
test_light_probes_gpu.py); not a test module itself.

Composed from what the suite already trusts, in numpy float32 scalars in the
contract's order.  For probe p at x_p and direction j of D:

    key = (index_base + p * D + j) mod 2^32
    oracle.path_norm(seed, key, 65535, 3)   the first three floatNorm draws of
                                            the stream (seed, key, 65535)
    occlusion_ref.normalize                 d_j = normalize(draws)
    radiance_ref.RadianceRef.radiance       L_j of the ray (x_p, d_j) with
                                            index_base = key
    trace_ref.RayRef.trace                  h_j of (x_p, normalize((d_j + 0) + 0))
    the basis on d_j, the sums in direction order, the scales
"""
import numpy as np

import occlusion_ref
import radiance_ref
import trace_ref

F = np.float32
DIR_SAMPLE = 65535
C0, C1, C2, C3, C4 = (F(float.fromhex(h)) for h in ("0x1.20dd76p-2", "0x1.f45438p-2", "0x1.17b142p+0",
                                                     "0x1.42f602p-2", "0x1.17b142p-1"))
FOUR_PI = F(float.fromhex("0x1.921fb6p+3"))
SH_BITS = {"C0": 0x3E906EBB, "C1": 0x3EFA2A1C, "C2": 0x3F8BD8A1, "C3": 0x3EA17B01, "C4": 0x3F0BD8A1,
           "FOUR_PI": 0x41490FDB}


def basis(d):
    """Y_0 .. Y_8 of the contract on d = (x, y, z), nine float32."""
    x, y, z = (F(v) for v in d)
    with np.errstate(all="ignore"):
        return np.array([C0,
                         F(C1 * y),
                         F(C1 * z),
                         F(C1 * x),
                         F(F(C2 * x) * y),
                         F(F(C2 * y) * z),
                         F(C3 * F(F(F(3.0) * F(z * z)) - F(1.0))),
                         F(F(C2 * x) * z),
                         F(C4 * F(F(x * x) - F(y * y)))], F)


def direction(orc, seed, key):
    """d_j of stream key `key`."""
    draws = orc.path_norm(int(seed) & 0xFFFFFFFFFFFFFFFF, int(key) & 0xFFFFFFFF, DIR_SAMPLE, 3)
    with np.errstate(all="ignore"):
        return occlusion_ref.normalize(draws)


def directions(orc, seed, keys):
    """(len(keys), 3) float32: d_j of every key."""
    return np.array([direction(orc, seed, k) for k in keys], F).reshape(-1, 3)


def traced_direction(d):
    """u_j: what the radiance call traces for d_j -- +0 added twice, normalised again."""
    with np.errstate(all="ignore"):
        return occlusion_ref.normalize([F(F(F(v) + F(0.0)) + F(0.0)) for v in d])


def fold(dirs, lin, t):
    """The sums of one probe over its D directions in order and their scaling:
    (sh (9, 3), distance (2,), hits) from d_j (D, 3), L_j (D, 3) and the first
    hits' t (D,), all float32."""
    D = len(dirs)
    A = np.zeros((9, 3), F)
    T1 = T2 = F(0.0)
    n = 0
    with np.errstate(all="ignore"):
        for j in range(D):
            Y = basis(dirs[j])
            for k in range(9):
                for c in range(3):
                    A[k, c] = F(A[k, c] + F(F(lin[j, c]) * Y[k]))
            tj = F(t[j])
            if tj != trace_ref.INF:
                T1 = F(T1 + tj)
                T2 = F(T2 + F(tj * tj))
                n += 1
        w = F(FOUR_PI / F(D))
        r = F(F(1.0) / F(D))
        return (A * w).astype(F), np.array([F(T1 * r), F(T2 * r)], F), n


def fold_batch(dirs, lin, t):
    """fold() for n probes at once -- (n, D, 3), (n, D, 3), (n, D) float32 ->
    (sh (n, 9, 3), distance (n, 2), hits (n,) uint32) -- one numpy float32
    operation per operation of the contract, the directions in order."""
    dirs, lin, t = (np.ascontiguousarray(a, F) for a in (dirs, lin, t))
    n, D = t.shape
    A = np.zeros((n, 9, 3), F)
    T1, T2 = np.zeros(n, F), np.zeros(n, F)
    cnt = np.zeros(n, np.uint32)
    one, three = F(1.0), F(3.0)
    with np.errstate(all="ignore"):
        for j in range(D):
            x, y, z = dirs[:, j, 0], dirs[:, j, 1], dirs[:, j, 2]
            Y = np.stack([np.full(n, C0, F), C1 * y, C1 * z, C1 * x, (C2 * x) * y, (C2 * y) * z,
                          C3 * ((three * (z * z)) - one), (C2 * x) * z, C4 * ((x * x) - (y * y))], axis=1)
            A = A + lin[:, j, None, :] * Y[:, :, None]
            tj = t[:, j]
            hit = tj != trace_ref.INF
            T1 = np.where(hit, T1 + tj, T1)
            T2 = np.where(hit, T2 + tj * tj, T2)
            cnt += hit
        w = F(FOUR_PI / F(D))
        r = F(one / F(D))
        assert A.dtype == F and T1.dtype == F and Y.dtype == F
        return A * w, np.stack([T1 * r, T2 * r], axis=1), cnt


class LightProbeRef:
    """The oracle's scene of (soup, res) and probes(positions, ...) against it."""

    def __init__(self, orc, soup, res):
        self.orc = orc
        self.rad = radiance_ref.RadianceRef(orc, soup, res)
        self.ray = trace_ref.RayRef(orc, soup, res)

    def probes(self, positions, D, spp, max_bounce, seed=0, index_base=0):
        """{"sh": (n, 9, 3), "distance": (n, 2), "hits": (n,) uint32,
        "directions", "radiance": (n, D, 3), "segments", "samples",
        "hits_total"}; the float arrays float32."""
        pos = np.ascontiguousarray(positions, F).reshape(-1, 3)
        n = len(pos)
        out = {"sh": np.zeros((n, 9, 3), F), "distance": np.zeros((n, 2), F), "hits": np.zeros(n, np.uint32),
               "directions": np.zeros((n, D, 3), F), "radiance": np.zeros((n, D, 3), F)}
        segments = 0
        for p in range(n):
            t = np.zeros(D, F)
            for j in range(D):
                key = (int(index_base) + p * D + j) & 0xFFFFFFFF
                d = direction(self.orc, seed, key)
                lin, _, ctr = self.rad.radiance(pos[p:p + 1], d[None, :], spp, max_bounce, seed=seed, index_base=key)
                segments += int(ctr[0])
                out["directions"][p, j] = d
                out["radiance"][p, j] = lin[0]
                t[j] = self.ray.trace(pos[p], traced_direction(d))[0][0]
            out["sh"][p], out["distance"][p], out["hits"][p] = fold(out["directions"][p], out["radiance"][p], t)
        out["segments"] = segments
        out["samples"] = n * D * spp
        out["hits_total"] = int(out["hits"].sum())
        return out
