"""One context, all ten entry points: seeded histories of renders, ray,
radiance, segment, surface, transmittance, feature, occlusion, direct-light and
light-probe calls (and calls the library refuses) on the same zrt_context,
every result against the CPU references, bit for bit.

test_context_history_gpu.py draws orders of render, trace and radiance.  The
seven calls merged after it stage through the same grow-only buffers, each in
a layout of its own (render.hip: query_rays, zrt_context_transmittance,
zrt_context_occlusion, zrt_context_direct, zrt_context_light_probes carve
d_rays and d_hits; zrt_context_features reuses pass set 0's queue and keeps
d_facc / d_fout; the probes go through d_lin / d_rgb), size their chunk from
what earlier calls left allocated, and promise in zrt.h to alternate freely.
A fresh context per test cannot show a word read before this call wrote it, an
offset only right at a fresh capacity, a split that depends on the calls
before, or a profile record a query clobbered.

history(seed) names one list of about OPS ops for good, on scene
SCENE_NAMES[seed % 3]: Cornell at 16^3 (opaque, the park kernel available),
the textured fuzz draw FUZZ_SEED (BLEND / MASK: chains and transparency are
real; built on the device) and WIDE_SEED (an axis above 1024: ZRT_TRACE_PARK
silently takes the lane walk).  A history opens with sequences that are
constructed (the host-only test below says which and asserts them from the op
lists alone) and goes on with ops dealt from the scene's pool, so every pool
op runs somewhere; NEW closes the context and makes another.  After every op:

1. the result equals the CPU reference's bits, and every stats field zrt.h
   specifies for the call (segments, samples, hits; the cell and test counters
   of a counting call) equals the reference's;
2. trace_launches equals the same op's on a context that ran nothing else
   (recorded once per distinct op; that run is checked against the reference
   too, so every op is also a context's first call);
3. the PAD guard rows behind every host output keep their sentinel, feature
   planes that were not asked for are not written, tensors sit between the
   guard tensors of test_context_history_gpu._on_device, the caller's inputs
   come back unchanged; a refused call raises and leaves every output alone;
4. for features, occlusion, direct and probes zrt_context_profile's record
   equals the one before the call.

A reference is computed once per distinct op and left unchanged; ops share the
per-batch work below them (a batch's first hits, its segment caches, its
surface records, a frame's pixel records at the most samples).
"""
import collections
import functools

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, native, scenes

import direct_ref
import feature_ref
import fuzz_scenes
import light_probe_ref
import occlusion_ref
import radiance_ref
import segment_ref
import surface_ref
import trace_ref
import transmit_ref
import test_context_history_gpu as hist
import test_direct_gpu
import test_light_probes_gpu
import test_occlusion_gpu
import test_surface_gpu
import test_trace_gpu
import test_transmit_gpu
from test_context_history_gpu import (FRAMES, FUZZ_SEED, SENTINEL, WIDE_SEED, Big, Radiance, Render, Trace, World,
                                      _on_device, owns_pixels, rays)
from test_query_fuzz_gpu import RADIANCE_MODES, TRACE_MODES

F = np.float32
MISS = trace_ref.MISS
SCENE_NAMES = ("cornell", "fuzz", "wide")
HISTORIES = 8            # per scene
SEEDS = list(range(HISTORIES * len(SCENE_NAMES)))
OPS = 30
PAD = 3                  # guard rows behind every host output
SMALL_FRAMES = FRAMES[:3]            # a feature reference walks every pixel's samples in Python
RAY_N, ITEM_N = (1, 100, 3000), (1, 33, 200)
# the rays of a batch are rays(soup, n, rayseed); few seeds per size, so that ops share a batch's first hits
RAYSEEDS = {1: (11, 12, 13), 100: (21, 22), 3000: (31,), 33: (41, 42), 200: (51,)}

Segments = collections.namedtuple("Segments", "n rayseed torch flags stats any_hit per_ray bseed")
Surface = collections.namedtuple("Surface", "n rayseed torch flags stats hits")
Transmit = collections.namedtuple("Transmit", "n rayseed torch flags stats per_ray bseed cap crossings")
Features = collections.namedtuple("Features", "w h spp spp_pass seed rank nranks tile flags stats planes device")
Occlusion = collections.namedtuple("Occlusion", "n rayseed torch flags stats S radius seed base outputs")
Direct = collections.namedtuple("Direct", "n rayseed torch flags stats lights unshadowed cap outputs")
Probes = collections.namedtuple("Probes", "n posseed torch flags D spp mb seed base outputs")
Refused = collections.namedtuple("Refused", "call why")
New = collections.namedtuple("New", "")
NEW = New()              # not an op: the context is closed and another one made

KIND = {Render: "render", Trace: "trace", Radiance: "radiance", Segments: "segments", Surface: "surface",
        Transmit: "transmit", Features: "features", Occlusion: "occlusion", Direct: "direct", Probes: "probes",
        Refused: "refused", Big: "big"}
KINDS = tuple(k for k in KIND.values() if k != "big")
STAGING = ("trace", "segments", "surface", "transmit", "occlusion", "direct", "probes")     # through d_rays / d_hits
PARK_KINDS = ("trace", "radiance", "segments", "surface", "transmit", "occlusion", "direct", "probes")
COUNTING = ("render", "trace", "segments", "surface", "transmit", "features", "occlusion", "direct")
PROFILE_KEPT = ("features", "occlusion", "direct", "probes")

LANE, PARK, MT = native.FLAG_LANE_WALK, native.TRACE_PARK, native.FLAG_MT_EXACT
# per kind: the lane walk as the call's own table names it, the park kernel, the exact walk
PATHS = {"trace": (TRACE_MODES["lane"], TRACE_MODES["park"], TRACE_MODES["mt_exact"]),
         "radiance": (RADIANCE_MODES["lane"], RADIANCE_MODES["park"], RADIANCE_MODES["mt_exact"]),
         "segments": (test_trace_gpu.MODES["lane"], test_trace_gpu.MODES["park"], test_trace_gpu.MODES["mt_exact"]),
         "surface": (test_surface_gpu.PATHS["lane"], test_surface_gpu.PATHS["park"],
                     test_surface_gpu.FUZZ_MODES["mt_exact"]),
         "transmit": tuple(test_transmit_gpu.MODES[k] for k in ("lane", "park", "mt_exact")),
         "features": (LANE, MT, 0),                              # (no park kernel in a primary walk)
         "occlusion": tuple(test_occlusion_gpu.MODES[k] for k in ("lane", "park", "mt_exact")),
         "direct": tuple(test_direct_gpu.MODES[k] for k in ("lane", "park", "mt_exact")),
         "probes": tuple(test_light_probes_gpu.MODES[k] for k in ("lane", "park", "mt_exact"))}

PLANES = feature_ref.PLANES
WIDTH = dict(native.FEATURE_PLANES)
PLANE_SETS = (PLANES, ("depth",), ("hits",), ("base_color", "normal"), ("emissive", "transparency", "hits"),
              ("base_color", "emissive", "depth", "transparency", "hits"))
OCC_OUTPUTS = (("visibility",), ("occluded",), ("visibility", "occluded"), ("visibility", "hits"),
               ("visibility", "occluded", "hits"))
DIR_OUTPUTS = (("irradiance",), ("radiance",), ("irradiance", "radiance"), ("irradiance", "hits"),
               ("irradiance", "radiance", "hits"))
PROBE_ALL = ("sh", "distance", "hits", "directions", "radiance")
PROBE_OUTPUTS = (("sh",), ("directions", "radiance"), ("sh", "distance", "hits"), PROBE_ALL, ("distance",),
                 ("hits", "radiance"))
RADII = ("fuzz", "inf", "nonpos", "per_ray")
# one invalid call per name, from the ZRT_ERR_INVALID_ARG list of its entry point in zrt.h
REFUSALS = (("trace", "unknown flag"), ("trace", "null hits"),
            ("radiance", "counting flag"), ("radiance", "no samples"),
            ("segments", "reserved"), ("segments", "any with hits"), ("segments", "no output"),
            ("surface", "null surfaces"), ("surface", "unknown flag"),
            ("transmit", "no crossings allowed"), ("transmit", "257 crossings"),
            ("features", "no samples"), ("features", "tile 12"), ("features", "reserved"), ("features", "no plane"),
            ("occlusion", "no samples"), ("occlusion", "no output"),
            ("direct", "no crossings allowed"), ("direct", "no lights"), ("direct", "no output"),
            ("probes", "no bounce"), ("probes", "no directions"), ("probes", "counting flag"), ("probes", "reserved"))


def kind(op):
    return KIND[type(op)]


def on_host(op):
    """A call that stages its batch through d_rays / d_hits: a staging kind with host pointers."""
    return kind(op) in STAGING and not op.torch


def counting(op):
    return bool(getattr(op, "stats", False))


def parked(op):
    return kind(op) in PARK_KINDS and not counting(op) and bool(op.flags & PARK)


# ----------------------------------------------------------------- the draws
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _batch(rng, what, sizes):
    """(n, rayseed, torch, flags, stats) of a ray kind."""
    n = _pick(rng, sizes)
    on_torch = bool(rng.random() < 0.4)
    stats = bool(rng.random() < 0.25)
    return n, _pick(rng, RAYSEEDS[n]), on_torch, 0 if stats else _pick(rng, PATHS[what]), stats


def _draw_render(rng, **fixed):
    return hist._draw_render(rng, **fixed)


def _draw_trace(rng, **fixed):
    op = hist._draw_trace(rng)
    return op._replace(rayseed=_pick(rng, RAYSEEDS[op.n]))._replace(**fixed)


def _draw_radiance(rng, **fixed):
    op = hist._draw_radiance(rng)
    return op._replace(rayseed=_pick(rng, RAYSEEDS[op.n]), seed=_pick(rng, (4, 8)))._replace(**fixed)


def _draw_segments(rng, **fixed):
    op = Segments(*_batch(rng, "segments", RAY_N), bool(rng.random() < 0.5), bool(rng.random() < 0.6),
                  int(rng.integers(0, 3)))
    return op._replace(**fixed)


def _draw_surface(rng, **fixed):
    return Surface(*_batch(rng, "surface", RAY_N), bool(rng.random() < 0.5))._replace(**fixed)


def _draw_transmit(rng, **fixed):
    op = Transmit(*_batch(rng, "transmit", RAY_N), bool(rng.random() < 0.6), int(rng.integers(0, 3)),
                  _pick(rng, (1, 2, 16)), bool(rng.random() < 0.5))
    return op._replace(**fixed)


def _draw_features(rng, **fixed):
    w, h = _pick(rng, SMALL_FRAMES)
    spp = int(rng.integers(1, 6))
    spp_pass = 0 if rng.random() < 0.5 else int(rng.integers(1, 4))
    rank, nranks, tile = hist._draw_split(rng, w, h)
    stats = bool(rng.random() < 0.25)
    op = Features(w, h, spp, spp_pass, _pick(rng, (3, 9)), rank, nranks, tile, 0 if stats else _pick(rng, PATHS["features"]),
                  stats, _pick(rng, PLANE_SETS), bool(rng.random() < 0.4))
    return op._replace(**fixed)


def _draw_occlusion(rng, **fixed):
    op = Occlusion(*_batch(rng, "occlusion", ITEM_N), int(rng.integers(1, 7)), _pick(rng, RADII), _pick(rng, (5, 77)),
                   _pick(rng, (0, 1000, 2 ** 32 - 17)), _pick(rng, OCC_OUTPUTS))
    return op._replace(**fixed)


def _draw_direct(rng, **fixed):
    lights = ("fuzz", int(rng.integers(1, 5)), 0) if rng.random() < 0.5 else \
        ("box", int(rng.integers(1, 6)), int(rng.integers(1, 3)))
    op = Direct(*_batch(rng, "direct", ITEM_N), lights, bool(rng.random() < 0.3), _pick(rng, (1, 2, 16)),
                _pick(rng, DIR_OUTPUTS))
    return op._replace(**fixed)


def _draw_probes(rng, **fixed):
    op = Probes(int(rng.integers(1, 7)), _pick(rng, (1, 2)), bool(rng.random() < 0.4), _pick(rng, PATHS["probes"]),
                _pick(rng, (1, 5, 65)), int(rng.integers(1, 4)), int(rng.integers(1, 5)), _pick(rng, (4, 8)),
                _pick(rng, (0, 2 ** 32 - 3)), _pick(rng, PROBE_OUTPUTS))
    return op._replace(**fixed)


def _draw_refused(rng, **fixed):
    return Refused(*_pick(rng, REFUSALS))._replace(**fixed)


DRAW = {"render": _draw_render, "trace": _draw_trace, "radiance": _draw_radiance, "segments": _draw_segments,
        "surface": _draw_surface, "transmit": _draw_transmit, "features": _draw_features,
        "occlusion": _draw_occlusion, "direct": _draw_direct, "probes": _draw_probes, "refused": _draw_refused}
ITEM_KINDS = ("occlusion", "direct", "probes")       # a ray becomes S, L or D items: the dearest references
# the least and the most of each staging kind (see staging_need)
LEAST = {"occlusion": dict(S=1, outputs=("occluded",)), "direct": dict(lights=("fuzz", 1, 0), outputs=("irradiance",)),
         "probes": dict(D=1, outputs=("hits",))}
MOST = {"occlusion": dict(S=6, outputs=OCC_OUTPUTS[-1]), "direct": dict(lights=("box", 5, 1), outputs=DIR_OUTPUTS[-1]),
        "probes": dict(D=65, outputs=PROBE_ALL)}


def draw(k, rng, **fixed):
    """A draw of kind k with the fields `fixed` that the kind has."""
    op = DRAW[k](rng)
    return op._replace(**{f: v for f, v in fixed.items() if f in op._fields})


@functools.lru_cache(maxsize=None)
def pool(name):
    """(ops, roles, bigs): the scene's distinct ops, those of them the
    constructed sequences name, and the big renders of the existing file's
    pool.  The least and the most op of a staging kind take its lane and its
    exact walk, so every path of every kind runs.  The drawn part holds every
    kind, the item kinds once on the wide grid (a sample there walks up to
    1100 cells in the Python reference) and twice elsewhere."""
    rng = np.random.default_rng(8000 + SCENE_NAMES.index(name))
    timed = dict(torch=False, stats=False)
    whole = dict(rank=0, nranks=1, tile=64)
    r = {"lane": _draw_render(rng, flags=LANE, stats=False),
         "times": _draw_render(rng, flags=native.FLAG_KERNEL_TIMES, stats=False),
         "pixel": _draw_render(rng, w=1, h=1, **whole),
         "split": _draw_render(rng, w=40, h=7, rank=1, nranks=5, tile=8, stats=False),
         "split_features": _draw_features(rng, w=40, h=7, rank=2, nranks=5, tile=8, stats=False, flags=LANE),
         "passes": _draw_features(rng, w=24, h=24, spp=5, spp_pass=2, stats=False, flags=MT, **whole),
         "device_surface": _draw_surface(rng, n=3000, rayseed=31, torch=True, stats=False, flags=0, hits=False)}
    for k in PARK_KINDS:
        n = 3 if k == "probes" else 33 if k in ITEM_KINDS else 100
        r["park", k] = draw(k, rng, n=n, rayseed=RAYSEEDS[n][0] if k != "probes" else None, flags=PATHS[k][1], **timed)
    for k in STAGING:
        lo, hi = (1, 6) if k == "probes" else (1, 200) if k in ITEM_KINDS else (1, 3000)
        r["least", k] = draw(k, rng, n=lo, rayseed=RAYSEEDS[1][0], flags=PATHS[k][0], **timed, **LEAST.get(k, {}))
        r["most", k] = draw(k, rng, n=hi, rayseed=RAYSEEDS.get(hi, (0,))[0], flags=PATHS[k][2], **timed, **MOST.get(k, {}))
    for k in COUNTING:
        n = 33 if k in ITEM_KINDS else 100
        r["counting", k] = draw(k, rng, n=n, rayseed=RAYSEEDS[n][0], torch=False, flags=0, stats=True, w=24, h=24, **whole)
    r["timed", "render"], r["timed", "features"] = r["lane"], r["passes"]
    for k in COUNTING:
        r.setdefault(("timed", k), r.get(("park", k)))
    assert all(not counting(r["timed", k]) and counting(r["counting", k]) for k in COUNTING)
    ops = list(dict.fromkeys(r.values()))
    for k in KINDS:
        for _ in range(3 if k == "refused" else 1 if k in ITEM_KINDS and name == "wide" else 2):
            op = DRAW[k](rng)
            while op in ops:
                op = DRAW[k](rng)
            ops.append(op)
    assert len(ops) == len(set(ops))
    return tuple(ops), r, tuple(hist.pool(name)[1])


def _euler(nodes):
    """A closed walk over every ordered pair of distinct `nodes` once (Hierholzer)."""
    nxt = {a: [b for b in nodes if b != a] for a in nodes}
    stack, walk = [nodes[0]], []
    while stack:
        if nxt[stack[-1]]:
            stack.append(nxt[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    assert len(walk) == len(nodes) * (len(nodes) - 1) + 1
    return walk[::-1]


CIRCUIT = _euler(KINDS)
STEP = -(-(len(CIRCUIT) - 1) // len(SEEDS))          # kind pairs of the circuit per history


@functools.lru_cache(maxsize=None)
def scene_histories(name):
    """The scene's HISTORIES op lists.  History h is three contexts:

    - h < 7: the least op of STAGING[h + 1], the most of STAGING[h] (it
      reallocates d_rays and d_hits), the least of STAGING[h + 1] again (below
      the capacity another kind left); h == 7: a device surface batch without
      hits, its records in d_hits, between two host batches of other kinds;
    - the park op of PARK_KINDS[h] as a context's first call (h == 0: then a
      one-pixel render, the probes op whose chunk outgrows d_lin / d_rgb and
      the render again);
    - a lane-walk render, that park op as the second call, and then
      * its STEP + 1 kinds of the closed walk CIRCUIT over every ordered pair
        of kinds, staging kinds with host pointers;
      * h == 1: a one-pixel render, a features op of several passes (d_facc,
        a larger queue than the frame's), the render again; 2: a render of a
        rank, features of another rank of the same frame, the render again
        (the cached pixel list); 3: a render with kernel times before each
        kind that must keep the profile; 4, 5: counting and timed ops of the
        counting kinds in turn;
      * a big render before the kind KINDS[seed % 11];
      * ops dealt from the pool in shuffled rounds, up to OPS entries."""
    ops, r, bigs = pool(name)
    s = SCENE_NAMES.index(name)
    rng = np.random.default_rng(9000 + s)
    by_kind = {k: [o for o in ops if kind(o) == k and (k not in STAGING or not o.torch)] for k in KINDS}
    deal = []
    while len(deal) < HISTORIES * OPS:
        deal += [ops[int(i)] for i in rng.permutation(len(ops))]
    out = []
    for h in range(HISTORIES):
        seed = h * len(SCENE_NAMES) + s
        pk = PARK_KINDS[h]
        if h < 7:
            a, b = STAGING[h], STAGING[(h + 1) % 7]
            ops_h = [r["least", b], r["most", a], r["least", b]]
        else:
            ops_h = [r["most", "occlusion"], r["device_surface"], r["least", "segments"]]
        ops_h += [NEW, r["park", pk]]
        if h == 0:
            ops_h += [r["pixel"], r["most", "probes"], r["pixel"]]
        ops_h += [NEW, r["lane"], r["park", pk]]
        walk = [CIRCUIT[(STEP * seed + i) % (len(CIRCUIT) - 1)] for i in range(STEP + 1)]
        ops_h += [by_kind[k][(seed + i) % len(by_kind[k])] for i, k in enumerate(walk)]
        if h == 1:
            ops_h += [r["pixel"], r["passes"], r["pixel"]]
        elif h == 2:
            ops_h += [r["split"], r["split_features"], r["split"]]
        elif h == 3:
            for k in PROFILE_KEPT:
                ops_h += [r["times"], by_kind[k][seed % len(by_kind[k])]]
        elif h in (4, 5):
            ks = COUNTING[-1:] + COUNTING + COUNTING[:1]
            ops_h += [r["counting" if (i + h) % 2 else "timed", k] for i, k in enumerate(ks)]
        target = KINDS[seed % len(KINDS)]
        ops_h += [bigs[seed % len(bigs)], by_kind[target][(seed // 2) % len(by_kind[target])]]
        while len(ops_h) < OPS:
            ops_h.append(deal.pop())
        out.append(ops_h)
    return out


def history(seed):
    """(scene name, the ops of `seed`, NEW markers among them)."""
    name = SCENE_NAMES[seed % len(SCENE_NAMES)]
    return name, scene_histories(name)[seed // len(SCENE_NAMES)]


# ------------------------------------------------- the op lists alone (CPU)
K_OCC_ITEMS = K_DIR_ITEMS = 1 << 20      # kOccItems, kDirItems (render.hip)


def staging_need(op):
    """(words of d_rays, words of d_hits) a host batch of a staging kind asks
    for -- the formulas of render.hip (query_rays, zrt_context_transmittance,
    zrt_context_occlusion, zrt_context_direct, zrt_context_light_probes) for a
    batch below every chunk limit; both buffers are grow-only."""
    assert on_host(op)
    k = kind(op)
    if k == "probes":
        chunk, n = op.n * op.D, op.n                                   # items; the probes with an item in the chunk
        assert n <= (chunk + op.D - 1) // op.D + 1
        return (6 * chunk + 3 * n,
                chunk + 64 + n * (27 * ("sh" in op.outputs) + 2 * ("distance" in op.outputs) + ("hits" in op.outputs)) +
                3 * chunk * ("directions" in op.outputs))
    c = max(64, op.n)
    if k in ("trace", "surface"):
        return 6 * c, 4 * c
    if k == "segments":
        return 7 * c, 4 * c + (c + 3) // 4
    if k == "transmit":
        return 7 * c, 2 * c
    if k == "occlusion":
        m = min(K_OCC_ITEMS, c * op.S)
        return 7 * c + 8 * m, 5 * c + c * ("visibility" in op.outputs) + (m + 3) // 4
    L = op.lights[1]
    m = min(K_DIR_ITEMS, c * L)
    return 6 * c + 12 * L + 10 * m, 7 * c + 3 * c * ("radiance" in op.outputs)


def rgb_need(op):
    """The elements of d_rgb (and d_lin) a call asks for, as the existing file's."""
    if isinstance(op, Probes):
        return 3 * op.n * op.D
    if isinstance(op, Radiance):
        return 3 * op.n if op.mb else 0
    if isinstance(op, Big):
        return 3 * op.w * op.h
    return 3 * native.tile_pixels(op.w, op.h, op.tile, op.rank, op.nranks).size if isinstance(op, Render) else 0


def contexts(ops):
    """The op lists of a history's contexts (split at NEW)."""
    out = [[]]
    for op in ops:
        if op is NEW:
            out.append([])
        else:
            out[-1].append(op)
    return out


def _passes(op):
    return -(-op.spp // op.spp_pass) if op.spp_pass else 1


def test_histories_contain_the_sequences():
    runs = [(history(s)[0], c) for s in SEEDS for c in contexts(history(s)[1])]
    pairs = [(a, b) for _, c in runs for a, b in zip(c, c[1:])]
    triples = [t for _, c in runs for t in zip(c, c[1:], c[2:])]
    assert all(len(history(s)[1]) == OPS for s in SEEDS)
    assert len(KINDS) == 11 and set(STAGING + PARK_KINDS + COUNTING + PROFILE_KEPT) <= set(KINDS)

    # adjacent kinds: every ordered pair of distinct kinds; every kind right after a big render, one per history
    adjacent = {(kind(a), kind(b)) for a, b in pairs}
    assert all((a, b) in adjacent for a in KINDS for b in KINDS if a != b), \
        [(a, b) for a in KINDS for b in KINDS if a != b and (a, b) not in adjacent]
    assert all(("big", k) in adjacent for k in KINDS)
    assert all(sum(isinstance(o, Big) for o in history(s)[1]) == 1 for s in SEEDS)
    for name in SCENE_NAMES:
        assert {o for n, c in runs if n == name for o in c if isinstance(o, Big)} <= set(hist.pool(name)[1])

    # staging size orders, host pointers: every ordered pair of the seven kinds adjacent ...
    hosted = {(kind(a), kind(b)) for a, b in pairs if on_host(a) and on_host(b)}
    assert all((a, b) in hosted for a in STAGING for b in STAGING if a != b)
    # ... and each kind once needing more words of both buffers than any earlier op of its context (which
    # reallocates them), once fewer than the capacity a different kind left (stale words in another layout)
    grows, fits = set(), set()
    for _, c in runs:
        cap, by = [0, 0], [None, None]
        for o in c:
            if not on_host(o):
                continue
            need = staging_need(o)
            if all(need[i] > cap[i] > 0 for i in (0, 1)):
                grows.add(kind(o))
            if all(need[i] < cap[i] and by[i] != kind(o) for i in (0, 1)):
                fits.add(kind(o))
            for i in (0, 1):
                if need[i] > cap[i]:
                    cap[i], by[i] = need[i], kind(o)
    assert grows == set(STAGING) and fits == set(STAGING), (grows, fits)

    # a device surface batch without hits (its records stay in d_hits) between host batches of other staging kinds
    def own_records(o):
        return isinstance(o, Surface) and o.torch and not o.hits
    assert any(own_records(b) and on_host(a) and on_host(c) and "surface" not in (kind(a), kind(c)) for a, b, c in triples)

    # park first: per scene and kind, the op with the flag is a context's first call, and its second after a
    # lane-walk render -- no hit records grown yet
    for name in SCENE_NAMES:
        for k in PARK_KINDS:
            mine = [c for n, c in runs if n == name]
            assert any(kind(c[0]) == k and parked(c[0]) for c in mine if c), (name, k)
            assert any(len(c) > 1 and isinstance(c[0], Render) and owns_pixels(c[0]) and not c[0].stats and
                       c[0].flags & LANE and kind(c[1]) == k and parked(c[1]) for c in mine), (name, k)

    # d_lin / d_rgb regrown by a probes chunk between two renders of one frame; a features op of several
    # passes (d_facc, a larger queue than the frame's) between two such renders
    regrown = sums = 0
    for _, c in runs:
        cap = 0
        for i, o in enumerate(c):
            between = 0 < i < len(c) - 1 and isinstance(c[i - 1], Render) and owns_pixels(c[i - 1]) and c[i - 1] == c[i + 1]
            regrown += between and isinstance(o, Probes) and rgb_need(o) > cap > 0
            sums += (between and isinstance(o, Features) and _passes(o) > 1 and
                     o.w * o.h * min(o.spp_pass, o.spp) > c[i - 1].w * c[i - 1].h * c[i - 1].spp)
            cap = max(cap, rgb_need(o))
    assert regrown and sums

    # the cached pixel list: render(frame, split A), features(the frame, another rank or tile), render(A)
    assert any(isinstance(a, Render) and owns_pixels(a) and isinstance(b, Features) and a == c and
               (a.w, a.h) == (b.w, b.h) and (a.rank, a.nranks, a.tile) != (b.rank, b.nranks, b.tile)
               for a, b, c in triples)

    # counting next to timed, per counting kind: a counting op right after a timed one of another kind, a timed
    # one right after a counting one
    for k in COUNTING:
        assert any(kind(b) == k and counting(b) and kind(a) not in (k, "refused", "big") and not counting(a)
                   for a, b in pairs), k
        assert any(kind(b) == k and not counting(b) and counting(a) for a, b in pairs), k

    # the profile: a render that recorded kernel times directly before each kind that must keep it
    for k in PROFILE_KEPT:
        assert any(isinstance(a, Render) and owns_pixels(a) and not a.stats and a.flags & native.FLAG_KERNEL_TIMES and
                   kind(b) == k for a, b in pairs), k

    # every draw of the issue occurs: both pointer kinds, counting, every path
    ran = {o for _, c in runs for o in c}
    for k in KINDS[1:-1]:
        mine = [o for o in ran if kind(o) == k]
        assert {bool(o.device if k == "features" else o.torch) for o in mine} == {False, True}, k
        assert k == "radiance" or {f for o in mine for f in PATHS[k] if o.flags == f} == set(PATHS[k]), k
    assert {o.call for o in ran if isinstance(o, Refused)} >= {"segments", "features", "probes"}
    # every pool op and the scene's big ops run somewhere
    for name in SCENE_NAMES:
        ops, _, bigs = pool(name)
        assert set(ops) | set(bigs) == {o for n, c in runs if n == name for o in c}, name


def test_the_scenes_are_what_the_file_says():
    assert test_trace_gpu.CASES["cornell_bm"][1] == _scene("cornell")[1] == (16, 16, 16)
    assert max(_scene("wide")[1]) > 1024 >= max(_scene("fuzz")[1]) and _scene("fuzz")[2]
    for name in ("fuzz", "wide"):                  # the existing file's scene, so the two share a big reference
        theirs = hist._scene(name)
        assert (tuple(theirs[1]), theirs[2]) == _scene(name)[1:]


# ------------------------------------------------------------- the references
def _scene(name):
    """(soup, grid resolution, built on the device)"""
    if name == "cornell":
        return scenes.get_scene("cornell"), (16, 16, 16), False
    soup, res = fuzz_scenes.scene(FUZZ_SEED if name == "fuzz" else WIDE_SEED)[:2]
    return soup, tuple(res), name == "fuzz"


def _frozen(x):
    for a in (x.values() if isinstance(x, dict) else x if isinstance(x, (tuple, list)) else (x,)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


class Batch:
    """rays(soup, n, rayseed): their first hits, the counters of a counting
    trace, a segment cache per ray and, once asked, their surface records."""

    def __init__(self, w, n, rayseed):
        self.o, self.d = rays(w.soup, n, rayseed)
        self.bits, self.counts = w.ray_ref.trace_batch(self.o, self.d)
        self.counts = tuple(int(x) for x in self.counts)
        self.caches = [{} for _ in range(n)]
        self.t = self.bits[:, 0].copy().view(F)
        self.hit = self.bits[:, 3] != MISS
        _frozen((self.o, self.d, self.bits, self.t, self.hit))


class QueryWorld(World):
    """The existing World on this file's scenes, with the references of the seven later entry points."""

    def __init__(self, orc, name):
        self.orc, self.name = orc, name
        self.soup, self.res, self.device_build = _scene(name)
        self.oracle = orc.OracleScene(self.soup, self.res)
        self.ray_ref = trace_ref.RayRef(orc, self.soup, self.res)
        self.rad_ref = radiance_ref.RadianceRef(orc, self.soup, self.res)
        self.probe_ref = light_probe_ref.LightProbeRef.__new__(light_probe_ref.LightProbeRef)
        self.probe_ref.orc, self.probe_ref.rad, self.probe_ref.ray = orc, self.rad_ref, self.ray_ref
        self._want, self._fresh, self._memo = {}, {}, {}
        p = np.asarray(self.soup.pos, np.float64).reshape(-1, 3)
        self.lo, self.ext = p.min(0), p.max(0) - p.min(0)

    def make(self):
        return RenderScene(self.soup, self.res, device=0, device_build=self.device_build)

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = _frozen(fn())
        return self._memo[key]

    def batch(self, n, rayseed):
        return self.memo(("batch", n, rayseed), lambda: Batch(self, n, rayseed))

    def surface_words(self, n, rayseed):
        b = self.batch(n, rayseed)
        return self.memo(("surface", n, rayseed),
                         lambda: surface_ref.surface_batch(self.ray_ref, self.soup, b.o, b.d, b.bits))

    def bounds(self, op):
        """The t_max of a segment or transmittance op: per ray 0.5, 1 or 1.5
        times its own hit distance (a miss: the median hit distance), or one
        bound for all, the median hit distance; both outcomes occur."""
        def make():
            b = self.batch(op.n, op.rayseed)
            rng = np.random.default_rng(100 + op.bseed)
            mid = F(np.median(b.t[b.hit])) if b.hit.any() else F(1)
            if not op.per_ray:
                return F(mid * F((0.5, 1.0, 1.5)[op.bseed % 3])) if op.n == 1 else mid
            f = rng.choice(np.array([0.5, 1.0, 1.5], F), op.n)
            return (np.where(b.hit, b.t, mid) * f).astype(F)
        return self.memo(("bounds", op.n, op.rayseed, op.per_ray, op.bseed), make)

    def radius(self, op):
        fz = occlusion_ref.fuzz_radius(self.soup)
        if op.radius == "per_ray":
            return np.array([(fz, F(np.inf), F(0), F(fz / 4), F(-1))[i % 5] for i in range(op.n)], F)
        return {"fuzz": fz, "inf": F(np.inf), "nonpos": F(0) if op.seed % 2 else F(-1)}[op.radius]

    def lights(self, spec):
        src, L, lseed = spec
        return self.memo(("lights", spec), lambda: direct_ref.fuzz_lights(self.soup)[:L] if src == "fuzz" else
                         test_direct_gpu.box_lights(self.soup, L, 300 + lseed))

    def positions(self, op):
        rng = np.random.default_rng(500 + op.posseed)
        return np.ascontiguousarray(self.lo + (0.1 + 0.8 * rng.random((6, 3))) * self.ext, F)[:op.n]

    def camera(self, op):
        c = self.soup.camera(None)
        return native.camera_from_matrix(c.matrix, c.yfov, None, op.w, op.h)

    def want(self, op):
        """The reference of `op` as a dict of read-only arrays and numbers (the
        existing file's tuple for render, big and radiance ops)."""
        if isinstance(op, (Render, Big, Radiance)):
            # (the fuzz and the wide scene are the existing file's, grid and all: one big reference for both files)
            shared = hist._WORLDS.get(self.name) if self.name != "cornell" else None
            return shared.want(op) if shared is not None else super().want(op)
        k = kind(op)
        if k == "trace":
            b = self.batch(op.n, op.rayseed)
            return b.o, b.d, b.bits, b.counts
        if k == "segments":
            b, tm = self.batch(op.n, op.rayseed), self.bounds(op)

            def make():
                bits, counts, _ = segment_ref.segment_batch(self.ray_ref, b.o, b.d, tm, op.any_hit, b.caches)
                if op.per_ray and op.n >= 100:
                    assert 0 < counts[2] < int(b.hit.sum()), "both outcomes"
                return {"bits": bits, "occluded": bits[:, 3] != MISS, "counts": tuple(int(x) for x in counts)}
            return self.memo(("segments", op.n, op.rayseed, op.per_ray, op.bseed, op.any_hit), make)
        if k == "surface":
            b = self.batch(op.n, op.rayseed)
            return {"words": self.surface_words(op.n, op.rayseed), "bits": b.bits, "counts": b.counts}
        if k == "transmit":
            b, tm = self.batch(op.n, op.rayseed), self.bounds(op)
            chains = self.memo(("chains", op.n, op.rayseed, op.per_ray, op.bseed), lambda: [
                transmit_ref.chain(self.ray_ref, self.soup, b.o[i], b.d[i], np.broadcast_to(tm, (op.n,))[i],
                                   transmit_ref.CAP) for i in range(op.n)])

            def make():
                T, cr, tot, _ = transmit_ref.transmit_batch(self.ray_ref, self.soup, b.o, b.d, tm, op.cap, chains)
                return {"T": T, "crossings": cr, "totals": tuple(int(x) for x in tot)}
            return self.memo(("transmit", op.n, op.rayseed, op.per_ray, op.bseed, op.cap), make)
        if k == "features":
            pix = native.tile_pixels(op.w, op.h, op.tile, op.rank, op.nranks)
            rec = self.memo(("records", op.w, op.h, op.seed, op.rank, op.nranks, op.tile), lambda: feature_ref.PixelRecords(
                self.orc, self.ray_ref, self.soup, self.camera(op), op.seed, pix, 5))
            return self.memo(("features", op.w, op.h, op.seed, op.rank, op.nranks, op.tile, op.spp),
                             lambda: dict(rec.planes(op.spp), pix=pix, counters=tuple(rec.counters(op.spp))))
        if k == "occlusion":
            b = self.batch(op.n, op.rayseed)
            smp = self.memo(("samples", op.n, op.rayseed, op.seed, op.base), lambda: [
                occlusion_ref.ray_samples(self.ray_ref, self.soup, b.o[i], b.d[i], b.bits[i], op.seed, op.base + i, 6)
                for i in range(op.n)])

            def make():
                occ, vis, traced, (cells, tests) = occlusion_ref.occlusion_batch(self.ray_ref, smp, self.radius(op), op.S,
                                                                                 True)
                return {"occluded": occ, "visibility": vis, "bits": b.bits, "traced": traced,
                        "counts": (b.counts[0] + cells, b.counts[1] + tests)}
            return self.memo(("occlusion", op.n, op.rayseed, op.seed, op.base, op.radius, op.S), make)
        if k == "direct":
            b, lights = self.batch(op.n, op.rayseed), self.lights(op.lights)
            made = self.memo(("direct rays", op.n, op.rayseed, op.lights), lambda: [
                direct_ref.Ray(self.ray_ref, self.soup, b.o[i], b.d[i], b.bits[i], lights) for i in range(op.n)])

            def make():
                E, R, tot = direct_ref.direct_batch(self.ray_ref, self.soup, made, lights, op.cap, op.unshadowed, True)
                return {"irradiance": E, "radiance": R, "bits": b.bits, "totals": tot,
                        "counts": (b.counts[0] + tot["cells"], b.counts[1] + tot["tests"])}
            return self.memo(("direct", op.n, op.rayseed, op.lights, op.cap, op.unshadowed), make)
        assert k == "probes"
        return self.memo(("probes", op.n, op.posseed, op.D, op.spp, op.mb, op.seed, op.base), lambda: self.probe_ref.probes(
            self.positions(op), op.D, op.spp, op.mb, seed=op.seed, index_base=op.base))

    def fresh_launches(self, op):
        """trace_launches of `op` on a context that has run nothing else."""
        if op not in self._fresh:
            rs = self.make()
            try:
                self._fresh[op] = run(self, rs, op, "fresh")
            finally:
                rs.close()
        return self._fresh[op]


# ------------------------------------------------------------------- the GPU
def _have_torch():
    return torch is not None and torch.cuda.is_available()


def _buf(rows, width, dtype=np.uint32):
    """rows + PAD rows of `width` elements, every byte the sentinel."""
    a = np.empty((rows + PAD) * width, dtype)
    a.view(np.uint8)[:] = SENTINEL
    return a


def _rows(a, rows, width, what):
    """The first `rows` rows of a _buf as a copy; its guard rows must hold the sentinel."""
    assert (a[rows * width:].view(np.uint8) == SENTINEL).all(), (what, "a guard row behind an output was written")
    out = a[:rows * width].copy()
    return out.reshape(rows, width) if width > 1 else out


def _ptr(a):
    return None if a is None else a.ctypes.data


def _same(got, want, what, name):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    g = (got if got.dtype.itemsize == 1 else got.view(np.uint32)).reshape(len(want), -1)
    w = (want if want.dtype.itemsize == 1 else want.view(np.uint32)).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (what, name, f"{bad.size} rows differ, first {int(bad[0])}", g[bad[0]], w[bad[0]])


def _stats(st, what, segments, samples, hits=None, counts=None):
    assert (st["segments"], st["samples"]) == (segments, samples), (what, st)
    if hits is not None:
        assert st["hits"] == hits, (what, st, hits)
    if counts is not None:
        assert (st["cells_visited"], st["triangle_tests"]) == tuple(counts), (what, st, counts)


def _tensor(a):
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def _per_ray(fn, o, d, values):
    """_on_device with one more per-ray tensor (bounds or radii), which must come back unchanged too."""
    if np.ndim(values) == 0:
        return _on_device(lambda a, b: fn(a, b, float(values)), o, d)
    t = _tensor(values)
    res = _on_device(lambda a, b: fn(a, b, t), o, d)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), np.asarray(values, F).view(np.uint32)), "the caller's bounds"
    return res


def _split(values):
    """(pointer array or None, scalar for all) of a scalar or per-ray float32 argument."""
    if np.ndim(values) == 0:
        return None, float(values)
    return np.array(values, F), float("inf")


def _run_segments(w, ctx, op, what):
    b, want, tm = w.batch(op.n, op.rayseed), w.want(op), w.bounds(op)
    flags = op.flags | (native.SEGMENT_ANY if op.any_hit else 0) | (native.FLAG_COUNT_STATS if op.stats else 0)
    n = op.n
    if op.torch:
        res = _per_ray(lambda o, d, t: ctx.segments(o, d, t, any_hit=op.any_hit, flags=op.flags, stats=op.stats),
                       b.o, b.d, tm)
        hits, occ = None if op.any_hit else res["hits"].view(np.uint32), res["occluded"].view(np.uint8)
    else:
        r = np.ascontiguousarray(np.concatenate([b.o, b.d], axis=1))
        r0, (tma, tm_all) = r.copy(), _split(tm)
        hits, occ = None if op.any_hit else _buf(n, 4), _buf(n, 1, np.uint8)
        st = ctx.segments_raw(n, _ptr(r), _ptr(tma), _ptr(hits), _ptr(occ), False, flags, tm_all)
        res = {"stats": st}
        assert np.array_equal(r, r0) and (tma is None or np.array_equal(tma.view(np.uint32), tm.view(np.uint32))), what
        hits, occ = None if op.any_hit else _rows(hits, n, 4, what), _rows(occ, n, 1, what)
    if not op.any_hit:
        _same(hits, want["bits"], what, "hits")
    _same(occ, want["occluded"].view(np.uint8), what, "occluded")
    cells, tests, nhit = want["counts"]
    _stats(res["stats"], what, n, 0, nhit if op.any_hit or op.stats else None, (cells, tests) if op.stats else None)
    return res["stats"]["trace_launches"]


def _run_surface(w, ctx, op, what):
    b, want, n = w.batch(op.n, op.rayseed), w.want(op), op.n
    if op.torch:
        res = _on_device(lambda o, d: ctx.surface(o, d, flags=op.flags, stats=op.stats, hits=op.hits), b.o, b.d)
        surf, rec = res["surfaces"].view(np.uint32), res["hits"].view(np.uint32) if op.hits else None
    else:
        r = np.ascontiguousarray(np.concatenate([b.o, b.d], axis=1))
        r0, surf, rec = r.copy(), _buf(n, 16), _buf(n, 4) if op.hits else None
        st = ctx.surface_raw(n, _ptr(r), _ptr(surf), _ptr(rec), False,
                             op.flags | (native.FLAG_COUNT_STATS if op.stats else 0))
        res = {"stats": st}
        assert np.array_equal(r, r0), what
        surf, rec = _rows(surf, n, 16, what), _rows(rec, n, 4, what) if op.hits else None
    _same(surf, want["words"], what, "surfaces")
    if op.hits:
        _same(rec, want["bits"], what, "hits")
    _stats(res["stats"], what, n, 0, want["counts"][2] if op.stats else None, want["counts"][:2] if op.stats else None)
    return res["stats"]["trace_launches"]


def _run_transmit(w, ctx, op, what):
    b, want, tm, n = w.batch(op.n, op.rayseed), w.want(op), w.bounds(op), op.n
    if op.torch:
        res = _per_ray(lambda o, d, t: ctx.transmittance(o, d, t, max_crossings=op.cap, flags=op.flags, stats=op.stats,
                                                         crossings=op.crossings), b.o, b.d, tm)
        T, cr = res["transmittance"].view(np.uint32), res["crossings"].astype(np.uint32) if op.crossings else None
    else:
        r = np.ascontiguousarray(np.concatenate([b.o, b.d], axis=1))
        r0, (tma, tm_all) = r.copy(), _split(tm)
        T, cr = _buf(n, 1), _buf(n, 1) if op.crossings else None
        st = ctx.transmittance_raw(n, _ptr(r), _ptr(tma), _ptr(T), _ptr(cr), False,
                                   op.flags | (native.FLAG_COUNT_STATS if op.stats else 0), tm_all, op.cap)
        res = {"stats": st}
        assert np.array_equal(r, r0) and (tma is None or np.array_equal(tma.view(np.uint32), tm.view(np.uint32))), what
        T, cr = _rows(T, n, 1, what), _rows(cr, n, 1, what) if op.crossings else None
    _same(T, want["T"], what, "transmittance")
    if op.crossings:
        _same(cr, want["crossings"], what, "crossings")
    segs, cells, tests, nx = want["totals"]
    _stats(res["stats"], what, segs, 0, nx, (cells, tests) if op.stats else None)
    return res["stats"]["trace_launches"]


def _run_features(w, ctx, op, what):
    want = w.want(op)
    n = len(want["pix"])
    kw = dict(seed=op.seed, rank=op.rank, num_ranks=op.nranks, tile_size=op.tile,
              flags=op.flags | (native.FLAG_COUNT_STATS if op.stats else 0), samples_per_pass=op.spp_pass)
    cam = w.camera(op)
    if op.device:
        dev = torch.device("cuda", 0)
        g0 = torch.arange(4096, dtype=torch.int32, device=dev)
        bufs = {k: torch.full(((n + PAD) * WIDTH[k],), SENTINEL * 0x01010101 - (1 << 32), dtype=torch.int32, device=dev)
                for k in PLANES}
        g1 = torch.full((4096,), 5, dtype=torch.int32, device=dev)
        torch.cuda.current_stream().synchronize()
        st = ctx.features_raw(cam, op.spp, {k: bufs[k].data_ptr() for k in op.planes}, True, **kw)
        assert torch.equal(g0.cpu(), torch.arange(4096, dtype=torch.int32)) and bool((g1 == 5).all()), (what, "guards")
        bufs = {k: v.cpu().numpy().view(np.uint32) for k, v in bufs.items()}
    else:
        bufs = {k: _buf(n, WIDTH[k]) for k in PLANES}
        st = ctx.features_raw(cam, op.spp, {k: bufs[k].ctypes.data for k in op.planes}, False, **kw)
    for k in PLANES:
        if k in op.planes:                        # the owned pixels, packed; nothing behind them
            _same(_rows(bufs[k], n, WIDTH[k], what), want[k], what, k)
        else:
            assert (bufs[k].view(np.uint8) == SENTINEL).all(), (what, k, "a plane that was not asked for")
    segs, cells, tests, nhit = want["counters"]
    assert segs == n * op.spp
    _stats(st, what, segs, segs, nhit, (cells, tests) if op.stats else None)
    if n:
        assert st["trace_launches"] >= 2 * _passes(op), (what, st)
    return st["trace_launches"]


def _run_occlusion(w, ctx, op, what):
    b, want, rad, n = w.batch(op.n, op.rayseed), w.want(op), w.radius(op), op.n
    ask = op.outputs
    if op.torch:
        res = _per_ray(lambda o, d, t: ctx.occlusion(o, d, op.S, t, seed=op.seed, index_base=op.base, flags=op.flags,
                                                     stats=op.stats, hits="hits" in ask), b.o, b.d, rad)
        got = {"visibility": res["visibility"].view(np.uint32), "occluded": res["occluded"].astype(np.uint32)}
        if "hits" in ask:
            got["hits"] = res["hits"].view(np.uint32)
        st = res["stats"]
    else:
        r = np.ascontiguousarray(np.concatenate([b.o, b.d], axis=1))
        r0, (ra, r_all) = r.copy(), _split(rad)
        bufs = {"visibility": _buf(n, 1), "occluded": _buf(n, 1), "hits": _buf(n, 4)}
        st = ctx.occlusion_raw(n, _ptr(r), _ptr(ra), *[_ptr(bufs[k]) if k in ask else None for k in bufs], False, op.S,
                               r_all,
                               op.seed, op.base, op.flags | (native.FLAG_COUNT_STATS if op.stats else 0))
        assert np.array_equal(r, r0) and (ra is None or np.array_equal(ra.view(np.uint32), rad.view(np.uint32))), what
        got = {k: _rows(bufs[k], n, 4 if k == "hits" else 1, what) for k in ask}
        assert all((bufs[k].view(np.uint8) == SENTINEL).all() for k in bufs if k not in ask), what
    for k, v in got.items():
        _same(v, want["bits" if k == "hits" else k], what, k)
    _stats(st, what, n + want["traced"], 0, int(want["occluded"].sum(dtype=np.int64)), want["counts"] if op.stats else None)
    return st["trace_launches"]


def _run_direct(w, ctx, op, what):
    b, want, lights, n = w.batch(op.n, op.rayseed), w.want(op), w.lights(op.lights), op.n
    ask = op.outputs
    if op.torch:
        res = _on_device(lambda o, d: ctx.direct(o, d, lights, max_crossings=op.cap, flags=op.flags,
                                                 unshadowed=op.unshadowed,
                                                 irradiance="irradiance" in ask, radiance="radiance" in ask,
                                                 hits="hits" in ask, stats=op.stats), b.o, b.d)
        got = {k: res[k].view(np.uint32) for k in ask}
        st = res["stats"]
    else:
        r = np.ascontiguousarray(np.concatenate([b.o, b.d], axis=1))
        r0 = r.copy()
        bufs = {"irradiance": _buf(n, 3), "radiance": _buf(n, 3), "hits": _buf(n, 4)}
        st = ctx.direct_raw(n, _ptr(r), lights, *[_ptr(bufs[k]) if k in ask else None for k in bufs], False, op.cap,
                            op.flags | (native.FLAG_COUNT_STATS if op.stats else 0) |
                            (native.DIRECT_UNSHADOWED if op.unshadowed else 0))
        assert np.array_equal(r, r0), what
        got = {k: _rows(bufs[k], n, 4 if k == "hits" else 3, what) for k in ask}
        assert all((bufs[k].view(np.uint8) == SENTINEL).all() for k in bufs if k not in ask), what
    for k, v in got.items():
        _same(v, want["bits" if k == "hits" else k], what, k)
    tot = want["totals"]
    _stats(st, what, n + tot["segments"], tot["samples"], tot["hits"], want["counts"] if op.stats else None)
    return st["trace_launches"]


def _run_probes(w, ctx, op, what):
    want, pos, n, D = w.want(op), w.positions(op), op.n, op.D
    ask = op.outputs
    if op.torch:
        res = _on_device(lambda p, _: ctx.light_probes(p, D, op.spp, op.mb, seed=op.seed, index_base=op.base, flags=op.flags,
                                                       **{k: k in ask for k in PROBE_ALL}), pos, pos)
        got = {k: (res[k].astype(np.uint32) if k == "hits" else res[k].view(np.uint32)) for k in ask}
        st = res["stats"]
    else:
        p0 = pos.copy()
        width = {"sh": 27, "distance": 2, "hits": 1, "directions": 3 * D, "radiance": 3 * D}
        bufs = {k: _buf(n, width[k]) for k in PROBE_ALL}
        st = ctx.light_probes_raw(n, _ptr(pos), *[_ptr(bufs[k]) if k in ask else None for k in PROBE_ALL], False, D, op.spp,
                                  op.mb, op.seed, op.base, op.flags)
        assert np.array_equal(pos, p0), what
        got = {k: _rows(bufs[k], n, width[k], what) for k in ask}
        assert all((bufs[k].view(np.uint8) == SENTINEL).all() for k in bufs if k not in ask), what
    for k, v in got.items():
        _same(v, want[k], what, k)
    _stats(st, what, want["segments"], want["samples"], want["hits_total"])
    return st["trace_launches"]


def _run_refused(w, ctx, op, what):
    """The invalid call raises ZRT_ERR_INVALID_ARG and leaves every output it was given alone."""
    b = w.batch(33, RAYSEEDS[33][0])
    n = 33
    r = np.ascontiguousarray(np.concatenate([b.o, b.d], axis=1))
    out = {k: _buf(n, wd) for k, wd in (("a", 16), ("b", 4), ("c", 4), ("d", 27), ("e", 27))}
    p = {k: v.ctypes.data for k, v in out.items()}
    cam = native.camera_from_matrix(w.soup.camera(None).matrix, w.soup.camera(None).yfov, None, 4, 4)
    planes = {k: _buf(16, WIDTH[k]) for k in PLANES}
    pp = {k: v.ctypes.data for k, v in planes.items()}
    lights = w.lights(("fuzz", 2, 0))
    count = native.FLAG_COUNT_STATS
    calls = {
        ("trace", "unknown flag"): lambda: ctx.trace_raw(n, r.ctypes.data, p["b"], False, 0x40000000),
        ("trace", "null hits"): lambda: ctx.trace_raw(n, r.ctypes.data, None, False),
        ("radiance", "counting flag"): lambda: ctx.radiance_raw(n, r.ctypes.data, p["a"], p["b"], False, 2, 3, flags=count),
        ("radiance", "no samples"): lambda: ctx.radiance_raw(n, r.ctypes.data, p["a"], p["b"], False, 0, 3),
        ("segments", "reserved"): lambda: ctx.segments_raw(n, r.ctypes.data, None, p["a"], p["b"], False, reserved=1),
        ("segments", "any with hits"): lambda: ctx.segments_raw(n, r.ctypes.data, None, p["a"], p["b"], False,
                                                                native.SEGMENT_ANY),
        ("segments", "no output"): lambda: ctx.segments_raw(n, r.ctypes.data, None, None, None, False),
        ("surface", "null surfaces"): lambda: ctx.surface_raw(n, r.ctypes.data, None, p["b"], False),
        ("surface", "unknown flag"): lambda: ctx.surface_raw(n, r.ctypes.data, p["a"], p["b"], False, 0x40000000),
        ("transmit", "no crossings allowed"): lambda: ctx.transmittance_raw(n, r.ctypes.data, None, p["a"], p["b"], False,
                                                                            max_crossings=0),
        ("transmit", "257 crossings"): lambda: ctx.transmittance_raw(n, r.ctypes.data, None, p["a"], p["b"], False,
                                                                     max_crossings=257),
        ("features", "no samples"): lambda: ctx.features_raw(cam, 0, pp, False),
        ("features", "tile 12"): lambda: ctx.features_raw(cam, 3, pp, False, tile_size=12),
        ("features", "reserved"): lambda: ctx.features_raw(cam, 3, pp, False, reserved=1),
        ("features", "no plane"): lambda: ctx.features_raw(cam, 3, {}, False),
        ("occlusion", "no samples"): lambda: ctx.occlusion_raw(n, r.ctypes.data, None, p["a"], p["b"], p["c"], False, 0),
        ("occlusion", "no output"): lambda: ctx.occlusion_raw(n, r.ctypes.data, None, None, None, p["c"], False, 3),
        ("direct", "no crossings allowed"): lambda: ctx.direct_raw(n, r.ctypes.data, lights, p["a"], p["b"], p["c"], False,
                                                                   0),
        ("direct", "no lights"): lambda: ctx.direct_raw(n, r.ctypes.data, [], p["a"], p["b"], p["c"], False),
        ("direct", "no output"): lambda: ctx.direct_raw(n, r.ctypes.data, lights, None, None, p["c"], False),
        ("probes", "no bounce"): lambda: ctx.light_probes_raw(n, r.ctypes.data, p["d"], p["a"], p["b"], p["c"], p["e"],
                                                              False, 1, 2, 0),
        ("probes", "no directions"): lambda: ctx.light_probes_raw(n, r.ctypes.data, p["d"], p["a"], p["b"], p["c"], p["e"],
                                                                  False, 0, 2, 3),
        ("probes", "counting flag"): lambda: ctx.light_probes_raw(n, r.ctypes.data, p["d"], p["a"], p["b"], p["c"], p["e"],
                                                                  False, 1, 2, 3, flags=count),
        ("probes", "reserved"): lambda: ctx.light_probes_raw(n, r.ctypes.data, p["d"], p["a"], p["b"], p["c"], p["e"],
                                                             False, 1, 2, 3, reserved=1)}
    assert set(calls) == set(REFUSALS)
    with pytest.raises(native.ZrtError) as e:
        calls[(op.call, op.why)]()
    assert e.value.status == -1, (what, e.value.status)
    assert all((v.view(np.uint8) == SENTINEL).all() for v in list(out.values()) + list(planes.values())), what
    return None


RUN = {"segments": _run_segments, "surface": _run_surface, "transmit": _run_transmit, "features": _run_features,
       "occlusion": _run_occlusion, "direct": _run_direct, "probes": _run_probes, "refused": _run_refused}


def run(world, rs, op, what):
    """Runs `op` on rs, compares it with the reference, returns trace_launches
    (None: a refused call, or an op left out because torch sees no device)."""
    k = kind(op)
    if k in ("render", "big", "trace", "radiance"):
        return hist.run(world, rs, op, what)
    if (op.device if k == "features" else k != "refused" and op.torch) and not _have_torch():
        return None
    return RUN[k](world, rs.context, op, (world.name, what, op))


_WORLDS = {}


@pytest.fixture(scope="module")
def world(oracle_mod):
    def get(name):
        if name not in _WORLDS:
            _WORLDS[name] = QueryWorld(oracle_mod, name)
        return _WORLDS[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_history_matches_the_references_op_by_op(seed, world):
    name, ops = history(seed)
    w = world(name)
    rs = w.make()
    try:
        for i, op in enumerate(ops):
            if op is NEW:
                rs.close()
                rs = w.make()
                continue
            before = rs.context.profile() if kind(op) in PROFILE_KEPT else None
            launches = run(w, rs, op, f"history {seed} op {i} after {ops[max(i - 3, 0):i]}")
            if before is not None:
                assert rs.context.profile() == before, (name, seed, i, op, "the profile record of the last render")
            if launches is not None and not isinstance(op, Big):
                assert launches == w.fresh_launches(op), (name, seed, i, op, ops[max(i - 3, 0):i])
    finally:
        rs.close()
