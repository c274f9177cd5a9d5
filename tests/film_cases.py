"""The cases of the film tests (zrt_context_accumulate), shared by
test_film_gpu.py and test_film_host.py: frames, splits of a sample count over
calls, and the oracle frames they are compared with.

The scenes, the grid and the oracle cache are test_tall_gpu's (Cornell and the
fuzz draw 65 at (16, 16, 16)): an oracle frame either file asks for is computed
once per session, whichever test asks first.
"""
from test_tall_gpu import RENDER_MODES, RES, SCENES, THREADS, TWO_SETS, Tall, _TALL, _scatters  # noqa: F401

FRAMES = ((1, 1), (3, 3), (13, 5))       # 9 pixels: more than 8 queue regions; 65: crosses the 64-pixel resolve block
# splits of 64 cross the 16-sample resolve chunk inside calls and between them
SPLITS = {
    64: ((64,), (1, 63), (63, 1), (16, 16, 16, 16), (15, 17, 32), (1,) * 64),
    4096: ((4095, 1), (1, 4095)),
    65535: ((65534, 1), (1, 65534)),       # the last sample index the stream key holds
}
# (w, h, total, max_bounce): every split of `total`, in every mode
PARITY = ([(w, h, total, 4) for w, h in FRAMES for total in (64, 4096)] + [(1, 1, 65535, 4)] +
          [(1, 1, total, mb) for mb in (0, 1) for total in (64, 4096, 65535)])

PREFIX = (3, 3, (15, 17, 32), 4)           # every intermediate call against the oracle at its prefix
PASSES = (3, 3, (1000, 3096), 4, 1000)     # the second call: base 1000, samples_per_pass 1000, a last pass of 96
SETS = (13, 10, (1, 65534), 4)             # the second call alone is 2^23 samples or more: two pass sets, base 1
RANKS = (64, 33, (2, 3), 4, 32, 3)         # tile 32: 4 tiles over 3 ranks
CHECKPOINT = (13, 5, (17, 47), 4)
ISOLATION = (3, 3, (15, 49), 4)
ISOLATION_RENDER = (13, 5, 64, 4, 16)      # a render of 4 passes (d_acc) between the film's calls
BIG = 1 << 23

assert TWO_SETS == (SETS[0], SETS[1], sum(SETS[2]), SETS[3])


def prefixes(counts):
    out, s = [], 0
    for n in counts:
        s += n
        out.append(s)
    return out


def oracle_frames():
    """Every (w, h, spp, max_bounce) the GPU tests compare with."""
    fr = list(PARITY)
    for w, h, counts, mb in (PREFIX, PASSES[:4], SETS, RANKS[:4], CHECKPOINT, ISOLATION):
        fr += [(w, h, s, mb) for s in prefixes(counts)]
    fr.append(ISOLATION_RENDER[:4])
    # the one-sample prefix of the two-set frame is no case of its own (no output is asked there)
    fr.remove((SETS[0], SETS[1], 1, SETS[3]))
    return sorted(set(fr))


def tall_scene(orc, name):
    if name not in _TALL:
        _TALL[name] = Tall(orc, name)
    return _TALL[name]
