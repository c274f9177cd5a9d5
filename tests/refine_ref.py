"""zrt_context_refine's contract (include/zrt.h) in numpy f32, from oracle
frames alone: `lin(N)` gives the oracle's linear frame at N samples in the
film's packed order, (P, 3) float32.  Returns per call (b, active mask traced
by the call, counts after it)."""
import numpy as np

F = np.float32


def error(cur, p, b, c):
    d = (np.abs(cur[:, 0] - p[:, 0]) + np.abs(cur[:, 1] - p[:, 1])) + np.abs(cur[:, 2] - p[:, 2])
    m = (cur[:, 0] + cur[:, 1]) + cur[:, 2]
    k = F(b) / F(b - c)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d * k) / np.sqrt(np.fmax(m, F(2.0 ** -10)))


def simulate(lin, P, schedule, threshold, min_samples):
    frozen, n = np.zeros(P, bool), np.zeros(P, np.uint32)
    cp, b, c, calls = np.zeros((P, 3), F), 0, 0, []
    for spp in schedule:
        cur = lin(b) if b else None
        if c and b >= min_samples:
            with np.errstate(invalid="ignore"):
                stop = ~frozen & ~(error(cur, cp, b, c) > F(threshold))
            n[stop], frozen = b, frozen | stop
        active = ~frozen
        if active.any():
            if b:
                cp[active] = cur[active]
            c, b0, b = b, b, b + spp
        else:
            b0 = b
        calls.append((b0, active.copy(), np.where(frozen, n, np.uint32(b)).astype(np.uint32)))
    return calls
