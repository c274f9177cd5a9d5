"""One context, many calls: seeded histories of renders, ray queries, radiance
queries and one big render on the same zrt_context, every result against the
CPU oracle, bit for bit.

What a call launches depends on state the context keeps between calls
(render.hip, resolve_plan / grow_pass_set / device_budget): the
grow-only buffers of the pass sets and of the frame, the cached pixel list,
the escape table and the cull masks that the first big call (2^23 samples or
more) or the first forcing flag builds, the second stream and its events, the
event pools.  The three entry points also share pass set 0, d_rgb, d_lin and
ev_trace.  The other GPU tests make a fresh context per case, or repeat one
fixed order; here the order is drawn.

history(seed) names one list of OPS ops for good (the draw order is part of
the test, as in fuzz_scenes.py), on scene SCENE_NAMES[seed % 4]: Cornell at
128^3, the contest stand-in at 64^3, the textured fuzz draw FUZZ_SEED on its
drawn grid (built on the device) and the draw WIDE_SEED, whose grid has an
axis above 1024 (the wide walk, no park kernel).  A scene's ops
come from a pool of POOL distinct ones, so they repeat at different positions
and each reference is computed once.  After every op:

1. the result equals the oracle's: RGB8, linear bits, segments (and the
   counters of a counting call) for a render -- of a rank's pixels, the
   caller's image untouched elsewhere; the four hit words for a trace;
   radiance bits and RGB8 for a radiance query;
2. trace_launches equals that of the same op on a fresh context (recorded
   once per op): a split does not depend on the calls before.  Not asked of
   the big op, whose split may follow the device's free memory;
3. for torch-tensor ops a guard tensor allocated before and one after the
   call are unchanged.

One more history runs on native.Group(scene, [0, 0]) with a direct radiance
query on the second context between two group renders.

The host-only test asserts from the op lists alone that the histories contain
the sequences the file is about.
"""
import collections
import ctypes

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import fuzz_scenes
import radiance_ref
import trace_ref
import test_tall_gpu as tall_mod
from test_gpu_fuzz import MODES as RENDER_FLAGS
from test_query_fuzz_gpu import RADIANCE_MODES, TRACE_MODES

SCENE_NAMES = ("cornell", "contest", "fuzz", "wide")
FUZZ_SEED = 92           # a textured draw (BLEND and MASK on textures with alpha, clamp wrap) on a 37 x 30 x 41 grid
WIDE_SEED = 15           # 90 triangles on a 1100 x 8 x 7 grid; half of the primary rays hit
HISTORIES = 8            # per scene
SEEDS = list(range(HISTORIES * len(SCENE_NAMES)))
OPS, POOL = 24, 14
THREADS = 16
BIG = 1 << 23            # kSetsMinSamples (render.hip)
SENTINEL = 0xA5

FRAMES = ((1, 1), (24, 24), (40, 7), (96, 80), (200, 120))
BIG_FRAMES = ((13, 10, 65535), (512, 512, 32))          # (w, h, spp), max_bounce 4
OUTPUTS = (("image",), ("packed",), ("linear",), ("image", "linear"), ("packed", "linear"),
           ("image", "packed", "linear"))

Render = collections.namedtuple("Render", "w h spp spp_pass mb seed rank nranks tile flags stats outputs")
Trace = collections.namedtuple("Trace", "n rayseed torch flags stats")
Radiance = collections.namedtuple("Radiance", "n rayseed spp mb seed torch flags rgb")
Big = collections.namedtuple("Big", "w h spp mb seed")


def kind(op):
    return type(op).__name__.lower()


def owns_pixels(op):
    """A rank owns tile `rank` first, so it has pixels iff the frame has more tiles than that."""
    return op.rank < -(-op.w // op.tile) * -(-op.h // op.tile)


def _draw_split(rng, w, h, empty=False):
    """(rank, num_ranks, tile) of a render; `empty`: a rank that owns no pixel of the frame."""
    nranks, tile = ((1, 64), (3, 64), (5, 8), (2, 4096))[int(rng.integers(0, 4))]
    if empty:
        nranks, tile = ((3, 64), (2, 4096))[int(rng.integers(0, 2))]
        return nranks - 1, nranks, tile
    return int(rng.integers(0, min(nranks, -(-w // tile) * -(-h // tile)))), nranks, tile


def _draw_render(rng, **fixed):
    empty = fixed.pop("empty", False)
    w, h = FRAMES[int(rng.integers(0, 2 if empty else len(FRAMES)))]
    spp = int(rng.integers(1, 7))
    spp_pass = 0 if rng.random() < 0.5 else int(rng.integers(1, 4))
    mb = int(rng.integers(0, 6))
    seed = int(rng.integers(0, 2 ** 31))
    rank, nranks, tile = _draw_split(rng, w, h, empty)
    flags = list(RENDER_FLAGS.values())[int(rng.integers(0, len(RENDER_FLAGS)))]
    extra = (0, 0, native.FLAG_ONE_SET, native.FLAG_KERNEL_TIMES)[int(rng.integers(0, 4))]
    stats = bool(rng.random() < 0.2)
    outputs = OUTPUTS[int(rng.integers(0, len(OUTPUTS)))]
    op = Render(w, h, spp, spp_pass, mb, seed, rank, nranks, tile, 0 if stats else flags | extra, stats, outputs)
    return op._replace(**fixed)


def _draw_trace(rng, **fixed):
    n = (1, 100, 3000)[int(rng.integers(0, 3))]
    rayseed = int(rng.integers(0, 2 ** 31))
    on_torch = bool(rng.random() < 0.4)
    flags = list(TRACE_MODES.values())[int(rng.integers(0, len(TRACE_MODES)))]
    stats = bool(rng.random() < 0.25)
    return Trace(n, rayseed, on_torch, 0 if stats else flags, stats)._replace(**fixed)


def _draw_radiance(rng, **fixed):
    n = (1, 33, 200)[int(rng.integers(0, 3))]
    rayseed = int(rng.integers(0, 2 ** 31))
    spp, mb = int(rng.integers(1, 6)), int(rng.integers(0, 6))
    seed = int(rng.integers(0, 2 ** 31))
    on_torch = bool(rng.random() < 0.4)
    flags = list(RADIANCE_MODES.values())[int(rng.integers(0, len(RADIANCE_MODES)))]
    return Radiance(n, rayseed, spp, mb, seed, on_torch, flags, bool(rng.random() < 0.6))._replace(**fixed)


def pool(name):
    """The scene's POOL distinct ops and its big ops.  The first six carry
    what the file is about whatever else is drawn: a lane-walk render, a
    render with per-kernel times, a counting render, a render that forces the
    cull masks, a rank without pixels and a parked trace; the last two are a
    one-pixel render and a 200-ray radiance query."""
    rng = np.random.default_rng(6000 + SCENE_NAMES.index(name))
    ops = [_draw_render(rng, flags=native.FLAG_LANE_WALK, stats=False),
           _draw_render(rng, flags=native.FLAG_KERNEL_TIMES, stats=False),
           _draw_render(rng, flags=0, stats=True),
           _draw_render(rng, flags=native.FLAG_BFCULL, stats=False),
           _draw_render(rng, empty=True),
           _draw_trace(rng, flags=native.TRACE_PARK, stats=False)]
    draws = (_draw_render, _draw_trace, _draw_radiance, _draw_radiance, _draw_trace, _draw_render)
    for draw in draws:
        op = draw(rng)
        while op in ops:
            op = draw(rng)
        ops.append(op)
    # a one-pixel frame and a 200-ray radiance query: its chunk outgrows the frame's d_rgb
    ops.append(_draw_render(rng, w=1, h=1, rank=0, nranks=1, tile=64))
    ops.append(_draw_radiance(rng, n=200, mb=3))
    assert len(ops) == len(set(ops)) == POOL and all(owns_pixels(o) for o in ops[:4])
    bigs = [Big(w, h, spp, 4, int(rng.integers(0, 2 ** 31))) for w, h, spp in BIG_FRAMES]
    # (the oracle walks up to 1100 cells per segment of the wide grid: one big reference there, not two)
    return ops, bigs[:1] if name == "wide" else bigs


def history(seed):
    """(scene name, the list of OPS ops) of `seed`; one of the ops is a big
    render, at a drawn position.  Each scene's second history opens with the
    lane-walk render and the parked trace: the context has grown no hit
    records when the park kernel first asks for them.  Its third opens with
    the one-pixel render, the 200-ray radiance query, which reallocates d_rgb,
    and the render again."""
    name = SCENE_NAMES[seed % len(SCENE_NAMES)]
    ops, bigs = pool(name)
    rng = np.random.default_rng(7000 + seed)
    out = [ops[int(i)] for i in rng.integers(0, POOL, OPS)]
    at, big = int(rng.integers(0, OPS)), bigs[int(rng.integers(0, len(bigs)))]
    if seed // len(SCENE_NAMES) == 1:
        out[:2] = [ops[0], ops[5]]
        at = max(at, 2)
    if seed // len(SCENE_NAMES) == 2:
        out[:3] = [ops[12], ops[13], ops[12]]
        at = max(at, 3)
    out[at] = big
    return name, out


# ------------------------------------------------- the op lists alone (CPU)
def _counting(op):
    return bool(getattr(op, "stats", False))


def _forces_cull(op):
    return not isinstance(op, Big) and not _counting(op) and bool(op.flags & native.FLAG_BFCULL)


def _wavefront_mb(op):
    """max_bounce of a call that runs the wavefront kernels, else None."""
    if isinstance(op, Trace) or (isinstance(op, Render) and (op.stats or not owns_pixels(op))):
        return None
    return op.mb


def test_histories_contain_the_sequences():
    hs = [history(s)[1] for s in SEEDS]
    pairs = [(a, b) for h in hs for a, b in zip(h, h[1:])]
    kinds = {(kind(a), kind(b)) for a, b in pairs}
    all_kinds = ("render", "trace", "radiance", "big")
    assert all((a, b) in kinds for a in all_kinds for b in all_kinds if a != b), kinds
    assert all(sum(isinstance(o, Big) for o in h) >= 1 and len(h) == OPS for h in hs)
    assert {(o.w, o.h, o.spp) for h in hs for o in h if isinstance(o, Big)} == set(BIG_FRAMES)
    assert all(o.w * o.h * o.spp >= BIG for h in hs for o in h if isinstance(o, Big))

    def area(o):
        return o.w * o.h if isinstance(o, (Render, Big)) and (isinstance(o, Big) or owns_pixels(o)) else None
    frames = [(area(a), area(b)) for a, b in pairs if area(a) and area(b)]
    assert any(a > b for a, b in frames) and any(a < b for a, b in frames)
    # a smaller frame with another stride T right after the big one
    assert any(isinstance(a, Big) and isinstance(b, Render) and owns_pixels(b) for a, b in pairs)
    mbs = [(_wavefront_mb(a), _wavefront_mb(b)) for a, b in pairs]
    mbs = [(a, b) for a, b in mbs if a is not None and b is not None]
    assert any(a < b for a, b in mbs) and any(a > b for a, b in mbs)
    assert any(isinstance(a, Render) and not a.stats and owns_pixels(a) and a.flags & native.FLAG_LANE_WALK and
               isinstance(b, (Trace, Radiance)) and b.flags & native.TRACE_PARK for a, b in pairs)
    # ... and as a context's first two calls: no hit records grown before the park kernel asks for them
    for name in SCENE_NAMES:
        assert any(history(s)[0] == name and history(s)[1][0].flags & native.FLAG_LANE_WALK and
                   isinstance(history(s)[1][1], Trace) and history(s)[1][1].flags & native.TRACE_PARK for s in SEEDS)

    def rgb_need(o):
        """The elements of d_rgb a call asks for (grow-only: a larger need reallocates)."""
        if isinstance(o, Radiance):
            return 3 * o.n if o.mb else 0
        if isinstance(o, Trace):
            return 0
        return 3 * o.w * o.h if isinstance(o, Big) else 3 * native.tile_pixels(o.w, o.h, o.tile, o.rank, o.nranks).size
    regrown = 0
    for h in hs:                         # a radiance chunk that reallocates d_rgb between two renders
        cap = 0
        for i, o in enumerate(h):
            regrown += (isinstance(o, Radiance) and rgb_need(o) > cap > 0 and i + 1 < len(h) and
                        isinstance(h[i + 1], Render) and owns_pixels(h[i + 1]))
            cap = max(cap, rgb_need(o))
    assert regrown
    before = after = 0
    for h in hs:
        first_big = next(i for i, o in enumerate(h) if isinstance(o, Big))
        before += any(_forces_cull(o) for o in h[:first_big])
        after += any(_forces_cull(o) for o in h[first_big + 1:])
    assert before and after, (before, after)
    # a counting call right after a timed one: after a render of the timed kernels, and after one that
    # recorded per-kernel times; and a counting query after a timed one
    assert any(isinstance(a, Render) and not a.stats and owns_pixels(a) and isinstance(b, Render) and b.stats
               for a, b in pairs)
    assert any(isinstance(a, Render) and a.flags & native.FLAG_KERNEL_TIMES and owns_pixels(a) and
               _counting(b) for a, b in pairs)
    assert any(isinstance(b, Trace) and b.stats and not _counting(a) for a, b in pairs)
    empty = [o for h in hs for o in h if isinstance(o, Render) and not owns_pixels(o)]
    assert empty
    for o in empty:
        assert native.tile_pixels(o.w, o.h, o.tile, o.rank, o.nranks).size == 0
    assert any(isinstance(o, (Trace, Radiance)) and o.torch for h in hs for o in h)
    # every pool op and both big ops of every scene run somewhere
    for name in SCENE_NAMES:
        ops, bigs = pool(name)
        ran = {o for s in SEEDS if history(s)[0] == name for o in history(s)[1]}
        assert set(ops) | set(bigs) == ran, name


def test_the_scenes_are_what_the_file_says():
    soup, res = fuzz_scenes.scene(WIDE_SEED)[:2]
    assert max(res) > 1024 and soup.num_triangles >= 90
    soup, res = fuzz_scenes.scene(FUZZ_SEED)[:2]
    assert max(res) <= 1024 and soup.num_triangles >= 400
    used = [soup.materials[i] for i in np.unique(soup.mat)]
    assert any(tall_mod._is_blend_textured(soup, m) for m in used)
    assert any(tall_mod._is_clamp_wrapped(soup, m) for m in used)


# ------------------------------------------------------------------- the GPU
def _scene(name):
    """(soup, grid resolution, built on the device)"""
    if name == "cornell":
        return scenes.get_scene("cornell"), (128, 128, 128), False
    if name == "contest":
        return scenes.get_scene("contest"), (64, 64, 64), False
    if name == "fuzz":
        soup, res = fuzz_scenes.scene(FUZZ_SEED)[:2]
        return soup, res, True
    soup, res = fuzz_scenes.scene(WIDE_SEED)[:2]
    return soup, res, False


def rays(soup, n, rayseed):
    """n rays, (origins, dirs) float32: the even rows aim at a random
    triangle's centroid from outside the box (every fourth not unit length),
    the odd ones start inside it in a random direction."""
    rng = np.random.default_rng(rayseed)
    tris = soup.pos.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, ext = (lo + hi) / 2, hi - lo
    R = 1.5 * max(float(np.linalg.norm(ext)), 1e-3)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tgt = tris[rng.integers(0, len(tris), n)].mean(1)
    o = np.where((np.arange(n) % 2 == 0)[:, None], c + R * u, lo + rng.random((n, 3)) * ext)
    d = np.where((np.arange(n) % 2 == 0)[:, None], tgt - o, rng.normal(size=(n, 3)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where(np.arange(n) % 4 == 0, 2.5, 1.0)[:, None]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


class World:
    """A scene, its references, and per distinct op the reference's answer and
    the launches of a fresh context (each computed once, left unchanged)."""

    def __init__(self, orc, name):
        self.orc, self.name = orc, name
        self.soup, self.res, self.device_build = _scene(name)
        self.oracle = orc.OracleScene(self.soup, self.res)
        self.ray_ref = trace_ref.RayRef(orc, self.soup, self.res)
        self.rad_ref = radiance_ref.RadianceRef(orc, self.soup, self.res)
        self._want, self._fresh = {}, {}

    def make(self):
        return RenderScene(self.soup, self.res, device=0, device_build=self.device_build)

    def want(self, op):
        key = op._replace(torch=False) if hasattr(op, "torch") else op
        if isinstance(op, Render):      # the reference does not depend on how the call is made
            key = op._replace(spp_pass=0, flags=0, stats=False, outputs=())
        elif isinstance(op, Trace):
            key = key._replace(flags=0, stats=False)
        elif isinstance(op, Radiance):
            key = key._replace(flags=0, rgb=True)
        if key not in self._want:
            self._want[key] = self._reference(key)
        return self._want[key]

    def _reference(self, op):
        if isinstance(op, (Render, Big)):
            c = self.soup.camera(None)
            ocam = self.orc.camera_from_matrix(c.matrix, c.yfov, None, op.w, op.h)
            pix = native.tile_pixels(op.w, op.h) if isinstance(op, Big) else \
                native.tile_pixels(op.w, op.h, op.tile, op.rank, op.nranks)
            if pix.size == 0:
                return pix, np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint32), np.zeros(5, np.uint64)
            rgb, lin, ctr = self.oracle.render_pixels(ocam, op.spp, op.mb, pix, seed=op.seed, num_threads=THREADS)
            out = (pix, rgb, lin.view(np.uint32).copy(), ctr)
        elif isinstance(op, Trace):
            o, d = rays(self.soup, op.n, op.rayseed)
            bits, counts = self.ray_ref.trace_batch(o, d)
            out = (o, d, bits, counts)
        else:
            o, d = rays(self.soup, op.n, op.rayseed)
            lin, rgb, ctr = self.rad_ref.radiance(o, d, op.spp, op.mb, seed=op.seed)
            out = (o, d, lin.view(np.uint32).copy(), rgb, ctr)
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out

    def fresh_launches(self, op):
        """trace_launches of `op` on a context that has run nothing else."""
        if op not in self._fresh:
            rs = self.make()
            try:
                self._fresh[op] = run(self, rs, op, "fresh")
            finally:
                rs.close()
        return self._fresh[op]


def _have_torch():
    return torch is not None and torch.cuda.is_available()


def _on_device(fn, o, d):
    """fn(o, d) on torch tensors, between guard tensors that must come back unchanged."""
    dev = torch.device("cuda", 0)
    g0 = torch.arange(4096, dtype=torch.int32, device=dev)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    g1 = torch.full((4096,), 3, dtype=torch.int32, device=dev)
    res = fn(to, td)
    g2 = torch.full((4096,), 5, dtype=torch.int32, device=dev)
    out = {k: (v.cpu().numpy() if k != "stats" else v) for k, v in res.items()}
    assert torch.equal(g0.cpu(), torch.arange(4096, dtype=torch.int32)), "guard before the inputs"
    assert bool((g1 == 3).all()) and bool((g2 == 5).all()), "guards around the outputs"
    assert np.array_equal(to.cpu().numpy(), o) and np.array_equal(td.cpu().numpy(), d), "the caller's rays"
    return out


def run(world, rs, op, what):
    """Runs `op` on rs, compares it with the reference, returns trace_launches
    (None: an op left out because torch sees no device)."""
    what = (world.name, what, op)
    if isinstance(op, (Render, Big)):
        pix, rgb, bits, ctr = world.want(op)
        c = world.soup.camera(None)                     # (its aspect ratio, if any, dropped: the frames are the ops')
        cam = native.camera_from_matrix(c.matrix, c.yfov, None, op.w, op.h)
        if isinstance(op, Big):
            op = Render(op.w, op.h, op.spp, 0, op.mb, op.seed, 0, 1, 64, 0, False, ("image", "linear"))
        assert (pix.size > 0) == owns_pixels(op), what
        img = np.full((op.h, op.w, 3), SENTINEL, np.uint8) if "image" in op.outputs else None
        res = rs.context.render(cam, op.spp, op.mb, seed=op.seed, rank=op.rank, num_ranks=op.nranks, tile=op.tile,
                                stats=op.stats, image=img, packed="packed" in op.outputs,
                                linear="linear" in op.outputs, samples_per_pass=op.spp_pass, flags=op.flags)
        st = res["stats"]
        if img is not None:
            flat = img.reshape(-1, 3)
            assert np.array_equal(flat[pix], rgb), what
            rest = np.ones(op.w * op.h, bool)
            rest[pix] = False
            assert (flat[rest] == SENTINEL).all(), what
        if "packed" in op.outputs:
            assert np.array_equal(res["packed"], rgb), what
        if "linear" in op.outputs:
            assert np.array_equal(res["linear"].view(np.uint32), bits), what
        assert st["segments"] == int(ctr[0]) and st["samples"] == pix.size * op.spp, what
        if op.stats:
            assert (st["cells_visited"], st["triangle_tests"], st["hits"]) == tuple(int(x) for x in ctr[1:4]), what
        if pix.size:
            passes = -(-op.spp // op.spp_pass) if op.spp_pass else None
            prof = rs.context.profile()
            if passes:
                assert prof["passes"] == passes, what
                assert st["trace_launches"] == passes * (1 if op.stats else max(op.mb, 1)), what
        return st["trace_launches"]
    if op.torch and not _have_torch():
        return None
    if isinstance(op, Trace):
        o, d, bits, counts = world.want(op)
        if op.torch:
            res = _on_device(lambda a, b: rs.trace(a, b, flags=op.flags, stats=op.stats), o, d)
            got = res["hits"].view(np.uint32)
        else:
            res = rs.trace(o, d, flags=op.flags, stats=op.stats)
            got = trace_ref.hit_bits(res)
        bad = np.nonzero((got != bits).any(axis=1))[0]
        assert bad.size == 0, (what, bad.size, int(bad[0]), got[bad[0]], bits[bad[0]])
        st = res["stats"]
        assert st["segments"] == op.n and st["samples"] == 0, what
        if op.stats:
            assert (st["cells_visited"], st["triangle_tests"], st["hits"]) == counts, what
        return st["trace_launches"]
    o, d, bits, rgb, ctr = world.want(op)

    def call(a, b):
        return rs.radiance(a, b, op.spp, op.mb, seed=op.seed, flags=op.flags, rgb=op.rgb)
    res = _on_device(call, o, d) if op.torch else call(o, d)
    bad = np.nonzero((res["radiance"].view(np.uint32) != bits).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, int(bad[0]))
    if op.rgb:
        assert np.array_equal(res["rgb"], rgb), what
    st = res["stats"]
    assert st["segments"] == int(ctr[0]) and st["samples"] == op.n * op.spp, what
    return st["trace_launches"]


_WORLDS = {}


@pytest.fixture(scope="module")
def world(oracle_mod):
    def get(name):
        if name not in _WORLDS:
            _WORLDS[name] = World(oracle_mod, name)
        return _WORLDS[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_history_matches_the_oracle_op_by_op(seed, world):
    name, ops = history(seed)
    w = world(name)
    rs = w.make()
    try:
        for i, op in enumerate(ops):
            launches = run(w, rs, op, f"history {seed} op {i} after {ops[max(i - 3, 0):i]}")
            if launches is not None and not isinstance(op, Big):
                assert launches == w.fresh_launches(op), (name, seed, i, op, ops[:i])
    finally:
        rs.close()


@pytest.mark.gpu
def test_group_history_with_a_direct_query_on_the_second_context(oracle_mod):
    """Group renders on two contexts of device 0: in 20x20 one 32-pixel tile
    holds the image, so the second context owns nothing; a radiance query on
    the second context itself goes between two renders."""
    soup, res = scenes.get_scene("cornell"), (32, 32, 32)
    oracle = oracle_mod.OracleScene(soup, res)
    c = soup.camera(None)
    geo = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, res)
    keep = []
    native.attach_materials(geo.scene, soup.tex_desc, soup.texels, keep)
    o, d = rays(soup, 200, 5)
    lin, rgb8, ctr = radiance_ref.RadianceRef(oracle_mod, soup, res).radiance(o, d, 3, 4, seed=9)
    want = {}

    def frame(w, h, spp, mb, seed):
        if (w, h, spp, mb, seed) not in want:
            ocam = oracle_mod.camera_from_matrix(c.matrix, c.yfov, None, w, h)
            want[(w, h, spp, mb, seed)] = oracle.render(ocam, spp, mb, oracle_mod.RNG_PATH, seed, THREADS)
        return want[(w, h, spp, mb, seed)]

    assert native.tile_pixels(20, 20, 32, 1, 2).size == 0 and native.tile_pixels(24, 24, 32, 1, 2).size == 0
    assert native.tile_pixels(200, 120, 32, 1, 2).size > 0
    grp = native.Group(geo.scene, [0, 0])
    second = native.Context.__new__(native.Context)     # borrowed: the group destroys it
    second._h = None
    try:
        h = ctypes.c_void_p()
        native.check(native.lib().zrt_group_context(grp._h, 1, ctypes.byref(h)), "zrt_group_context")
        order = [(20, 20, 3, 4, 1), (200, 120, 2, 4, 2), "query", (24, 24, 4, 2, 3), "query", (200, 120, 2, 4, 2),
                 (20, 20, 3, 4, 1), "query", (200, 120, 5, 3, 4), (24, 24, 4, 2, 3)]
        for i, step in enumerate(order):
            if step == "query":
                second._h = h
                try:
                    res_q = second.radiance(o, d, 3, 4, seed=9, flags=native.TRACE_PARK if i % 2 else 0, rgb=True)
                finally:
                    second._h = None
                assert np.array_equal(res_q["radiance"].view(np.uint32), lin.view(np.uint32)), i
                assert np.array_equal(res_q["rgb"], rgb8) and res_q["stats"]["segments"] == int(ctr[0]), i
                continue
            w, hh, spp, mb, seed = step
            cam = camera_for(soup, None, w, hh)
            img, st = grp.render(cam, spp, mb, seed=seed)
            rgb, _, fctr = frame(*step)
            assert np.array_equal(img.reshape(-1, 3), rgb), (i, step)
            assert st["segments"] == int(fctr[0]) and st["samples"] == w * hh * spp, (i, step)
    finally:
        second._h = None
        grp.close()
