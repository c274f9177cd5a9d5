"""Light-probe queries on the GPU (zrt_context_light_probes,
Context.light_probes), bit for bit as uint32 patterns, the stats in every call:

  * against the per-probe reference (light_probe_ref.py) on the Cornell box in
    brick-major and field words and on the contest scene, D in {1, 16, 65},
    (S, max_bounce) in {(1, 1), (3, 4), (2, 32)}, through every launch mode, on
    both ways of making a context, host arrays and device tensors by turns, all
    five outputs between guard words;
  * against the device composition a caller writes without the call -- the
    call's own directions through Context.radiance with the same keys,
    Context.trace for the first hits, the ordered float32 sum in numpy -- over
    N x D around the wave and half-wave sizes, sliced batches, and a batch whose
    items cross the 2^20 cut inside a probe while the keys wrap at 2^32, and a
    batch of three chunks whose middle one begins and ends inside a probe;
  * 65535 samples per direction, each output alone, alternation with renders and
    radiance calls, empty and bad batches.

A case's probes (seeded): 24 at 0.15 .. 0.85 of the box extent and 2 outside
the box.  A (case, D, S, max_bounce) reference is computed once and shared,
test_light_probes_host.py counts what the cases reach.
"""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: libzrt then binds to torch's HIP runtime, as in bench.py)
except ImportError:
    torch = None

from zig_raytracing_contest_amd import RenderScene, camera_for, native, scenes

import light_probe_ref as lpr

pytestmark = pytest.mark.gpu

F = np.float32
CASES = {"cornell_bm": (lambda: scenes.get_scene("cornell"), (16, 16, 16)),       # brick-major words
         "cornell_fields": (lambda: scenes.get_scene("cornell"), (12, 20, 9)),    # field words
         "contest": (lambda: scenes.get_scene("contest"), (32, 32, 32))}          # textures, pass-through segments
DIRS = [1, 16, 65]
CONFIGS = [(1, 1), (3, 4), (2, 32)]                                               # (S, max_bounce)
MODES = {"default": 0, "park": native.TRACE_PARK, "lane": native.FLAG_LANE_WALK, "mt_exact": native.FLAG_MT_EXACT,
         "park_escape": native.TRACE_PARK | native.FLAG_ESCAPE,
         "park_release": native.TRACE_PARK | native.FLAG_RELEASE,
         "park_no_release": native.TRACE_PARK | native.FLAG_NO_RELEASE}
SEED = 11
N_IN, N_OUT = 24, 2
OUTPUTS = ("sh", "distance", "hits", "directions", "radiance")
GUARD = 0xA5A5A5A5
PAD = 4


def case_probes(soup, seed):
    """The case's N_IN + N_OUT probe positions, (26, 3) float32."""
    rng = np.random.default_rng(seed)
    xyz = soup.pos.reshape(-1, 3).astype(np.float64)
    lo, hi = xyz.min(0), xyz.max(0)
    ext = hi - lo
    inside = lo + (0.15 + 0.7 * rng.random((N_IN, 3))) * ext
    outside = (lo + hi) / 2 + ext * np.array([[0.65, 0.1, 0.05], [-0.1, 0.65, 0.05]])      # off two faces
    return np.ascontiguousarray(np.concatenate([inside, outside]), F)


class Case:
    def __init__(self, orc, name):
        mk, self.res = CASES[name]
        self.soup = mk()
        self.ref = lpr.LightProbeRef(orc, self.soup, self.res)
        self.pos = case_probes(self.soup, sorted(CASES).index(name) + 31)
        self._want = {}

    def want(self, D, S, mb):
        """The reference at seed SEED, index_base 0 (read-only arrays)."""
        key = (D, S, mb)
        if key not in self._want:
            w = self.ref.probes(self.pos, D, S, mb, seed=SEED)
            for k in OUTPUTS:
                w[k].setflags(write=False)
            self._want[key] = w
        return self._want[key]


_CASES = {}


def get_case(orc, name):
    if name not in _CASES:                         # one set of references for every module that needs them
        _CASES[name] = Case(orc, name)
    return _CASES[name]


@pytest.fixture(scope="module")
def case(oracle_mod):
    return lambda name: get_case(oracle_mod, name)


@pytest.fixture(scope="module")
def scene(case):
    """The context of (case, build), made once."""
    made = {}

    def get(name, build="host"):
        if (name, build) not in made:
            cs = case(name)
            made[(name, build)] = RenderScene(cs.soup, cs.res, device=0, device_build=build == "device")
        return made[(name, build)]
    yield get
    for rs in made.values():
        rs.close()


def have_torch():
    return torch is not None and torch.cuda.is_available()


def sizes(n, D):
    return {"sh": 27 * n, "distance": 2 * n, "hits": n, "directions": 3 * n * D, "radiance": 3 * n * D}


def call(ctx, pos, D, S, mb, seed=SEED, index_base=0, flags=0, want=OUTPUTS, dev=False):
    """zrt_context_light_probes through light_probes_raw, every asked output
    between PAD guard words on each side: {name: uint32 patterns (flat), "stats"}.
    dev: the positions and outputs are device tensors."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    words = sizes(n, D)
    if dev:
        d0 = torch.device("cuda", 0)
        bufs = {k: torch.full((words[k] + 2 * PAD,), GUARD - (1 << 32), dtype=torch.int32, device=d0) for k in want}
        tpos = torch.from_numpy(pos).to(d0)
        torch.cuda.synchronize()
        ptr = {k: b.data_ptr() + 4 * PAD for k, b in bufs.items()}
        ppos = tpos.data_ptr()
    else:
        bufs = {k: np.full(words[k] + 2 * PAD, GUARD, np.uint32) for k in want}
        ptr = {k: b.ctypes.data + 4 * PAD for k, b in bufs.items()}
        ppos = pos.ctypes.data
    st = ctx.light_probes_raw(n, ppos, ptr.get("sh"), ptr.get("distance"), ptr.get("hits"), ptr.get("directions"),
                              ptr.get("radiance"), dev, D, S, mb, seed, index_base, flags)
    res = {"stats": st}
    for k, b in bufs.items():
        a = b.cpu().numpy().view(np.uint32) if dev else b
        assert (a[:PAD] == GUARD).all() and (a[PAD + words[k]:] == GUARD).all(), f"{k}: a guard word was written"
        res[k] = a[PAD:PAD + words[k]].copy()
    return res


def bits(a):
    a = np.ascontiguousarray(a)
    return (a if a.dtype == np.uint32 else a.view(np.uint32)).reshape(-1)


def check(got, want, what, names=OUTPUTS):
    """got: call()'s result; want: arrays by name (float32 or uint32, any shape)."""
    for k in names:
        g, w = got[k], bits(want[k])
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (f"{what}: {k}: {bad.size} words differ, first {bad[0]}: got {hex(int(g[bad[0]]))}, "
                               f"expected {hex(int(w[bad[0]]))}")


def check_stats(st, want, what):
    assert (st["segments"], st["samples"], st["hits"]) == (want["segments"], want["samples"], want["hits_total"]), \
        (what, st, want["segments"], want["samples"], want["hits_total"])


# --------------------------------------------------------- against the reference
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"spp{c[0]}_mb{c[1]}")
@pytest.mark.parametrize("D", DIRS)
@pytest.mark.parametrize("name", list(CASES))
def test_light_probes_match_the_reference(name, D, cfg, build, case, scene):
    S, mb = cfg
    cs, rs = case(name), scene(name, build)
    want = cs.want(D, S, mb)
    turn = list(CASES).index(name) + DIRS.index(D) + CONFIGS.index(cfg)
    for i, (mode, flags) in enumerate(MODES.items()):
        dev = have_torch() and (i + turn) % 2 == 1
        what = f"{name} D {D} spp {S} max_bounce {mb} {mode} {build} {'device' if dev else 'host'}"
        res = call(rs.context, cs.pos, D, S, mb, flags=flags, dev=dev)
        check(res, want, what)
        check_stats(res["stats"], want, what)
        assert res["stats"]["trace_launches"] > 0 and res["stats"]["render_ms"] > 0


# ------------------------------------------------- against the device composition
def composition(rs, pos, D, S, mb, dirs, seed=SEED, index_base=0, dev=False):
    """What a caller computes without the call from its `directions` output
    ((n * D * 3) patterns): Context.radiance over (x_p, d_j) with the same keys,
    Context.trace over (x_p, u_j), the ordered float32 sums."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    d = dirs.view(F).reshape(n * D, 3)
    o = np.ascontiguousarray(np.repeat(pos, D, axis=0))
    with np.errstate(all="ignore"):
        z = (d + F(0.0)) + F(0.0)
        n2 = (z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]) + z[:, 2] * z[:, 2]
        u = np.ascontiguousarray(z * (F(1.0) / np.sqrt(n2))[:, None])
    assert u.dtype == F
    if dev:
        d0 = torch.device("cuda", 0)
        to, td, tu = (torch.from_numpy(np.ascontiguousarray(x)).to(d0) for x in (o, d, u))
        r = rs.radiance(to, td, S, mb, seed=seed, index_base=index_base)
        lin, rst = r["radiance"].cpu().numpy(), r["stats"]
        t = rs.trace(to, tu)["hits"][:, 0].cpu().numpy()
    else:
        r = rs.radiance(o, d, S, mb, seed=seed, index_base=index_base)
        lin, rst = r["radiance"], r["stats"]
        t = rs.trace(o, u)["t"]
    sh, dist, hits = lpr.fold_batch(d.reshape(n, D, 3), lin.reshape(n, D, 3), t.reshape(n, D))
    return {"sh": sh, "distance": dist, "hits": hits, "directions": d, "radiance": lin,
            "segments": rst["segments"], "samples": n * D * S, "hits_total": int(hits.sum())}


def grid_probes(soup, n, seed):
    rng = np.random.default_rng(seed)
    xyz = soup.pos.reshape(-1, 3).astype(np.float64)
    lo, hi = xyz.min(0), xyz.max(0)
    return np.ascontiguousarray(lo - 0.1 * (hi - lo) + 1.2 * rng.random((n, 3)) * (hi - lo), F)


@pytest.mark.parametrize("D", [1, 2, 27, 63, 64, 65])
def test_probe_and_direction_counts_around_the_wave_sizes(D, case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    for n in (1, 2, 63, 64, 65):
        pos = grid_probes(cs.soup, n, 100 + n)
        for dev in ([False, True] if have_torch() else [False]):
            res = call(rs.context, pos, D, 2, 3, index_base=7 * n, dev=dev)
            comp = composition(rs, pos, D, 2, 3, res["directions"], index_base=7 * n)
            what = f"N {n} D {D} {'device' if dev else 'host'}"
            check(res, comp, what)
            check_stats(res["stats"], comp, what)
    assert comp["hits_total"] > 0 and comp["sh"].any()


@pytest.mark.parametrize("D", [16, 65])
def test_a_slice_with_its_index_base_is_the_rows_of_the_whole(D, case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    want = cs.want(D, 3, 4)
    for k, n in ((0, 1), (5, 7), (25, 1), (13, 13)):
        res = call(rs.context, cs.pos[k:k + n], D, 3, 4, index_base=k * D)
        check(res, {name: want[name][k:k + n] for name in OUTPUTS}, f"probes [{k}, {k + n}) of D {D}")
        assert res["stats"]["hits"] == int(want["hits"][k:k + n].sum())


def test_the_cut_falls_inside_a_probe_and_the_keys_wrap(case, scene, oracle_mod):
    """4099 probes x 257 directions: item 2^20 is direction 16 of probe 4080, and
    the keys wrap at 2^32 at item 600000."""
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    dev = have_torch()                             # (on the device; host arrays only where torch sees none)
    n, D = 4099, 257
    assert (1 << 20) // D == 4080 and (1 << 20) % D == 16
    wrap = 600000
    base = (1 << 32) - wrap
    pos = grid_probes(cs.soup, n, 7)
    res = call(rs.context, pos, D, 1, 1, index_base=base, dev=dev)
    comp = composition(rs, pos, D, 1, 1, res["directions"], index_base=base, dev=dev)
    check(res, comp, "the cut", names=("sh", "distance", "hits", "radiance"))
    check_stats(res["stats"], comp, "the cut")
    assert 0 < comp["hits"][4080] and comp["sh"][4080].any()
    # the directions themselves: 4096 items, 64 on each side of the cut and of the wrap among them
    rng = np.random.default_rng(3)
    items = np.unique(np.concatenate([np.arange((1 << 20) - 64, (1 << 20) + 64), np.arange(wrap - 64, wrap + 64),
                                      [0, n * D - 1], rng.integers(0, n * D, 3838)]))
    keys = (base + items) & 0xFFFFFFFF
    assert keys[items == wrap][0] == 0 and keys[items == wrap - 1][0] == 0xFFFFFFFF
    want = lpr.directions(oracle_mod, SEED, keys)
    got = res["directions"].reshape(-1, 3)[items]
    assert np.array_equal(got, want.view(np.uint32)), np.nonzero((got != want.view(np.uint32)).any(1))[0][:8]


def test_a_middle_chunk_takes_a_carried_probe_and_leaves_another(case, scene):
    """8200 probes x 257 directions: three chunks.  The middle one, items 2^20 ..
    2^21, begins with direction 16 of probe 4080 and ends after direction 31 of
    probe 8160: its fold reads one probe's carried sums and leaves another's."""
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    dev = have_torch()                             # (on the device; host arrays only where torch sees none)
    n, D = 8200, 257
    assert (1 << 21) // D == 8160 and (1 << 21) % D == 32 and n * D > (1 << 21)
    pos = grid_probes(cs.soup, n, 8)
    res = call(rs.context, pos, D, 1, 1, index_base=5, dev=dev)
    comp = composition(rs, pos, D, 1, 1, res["directions"], index_base=5, dev=dev)
    check(res, comp, "three chunks", names=("sh", "distance", "hits", "radiance"))
    check_stats(res["stats"], comp, "three chunks")
    for p in (4080, 8160):
        assert 0 < comp["hits"][p] and comp["sh"][p].any(), p
    again = call(rs.context, pos, D, 1, 1, index_base=5, want=("sh", "distance", "hits"), dev=dev)
    for k in ("sh", "distance", "hits"):
        assert np.array_equal(again[k], res[k]), k


def test_65535_samples_per_direction(case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    pos = cs.pos[3:4]
    want = cs.ref.probes(pos, 2, 65535, 2, seed=SEED, index_base=9)
    res = call(rs.context, pos, 2, 65535, 2, index_base=9)
    check(res, want, "1 x 2 x 65535")
    check_stats(res["stats"], want, "1 x 2 x 65535")
    assert want["radiance"].any()


def test_each_output_alone(case, scene):
    cs, rs = case("contest"), scene("contest")
    want = cs.want(16, 3, 4)
    for dev in ([False, True] if have_torch() else [False]):
        for k in OUTPUTS:
            res = call(rs.context, cs.pos, 16, 3, 4, want=(k,), dev=dev)
            check(res, want, f"{k} alone", names=(k,))
            check_stats(res["stats"], want, f"{k} alone")


def test_probes_renders_and_radiance_share_a_context_cleanly(case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    want = cs.want(16, 3, 4)
    cam = camera_for(cs.soup, None, 24, 24)
    fresh = RenderScene(cs.soup, cs.res, device=0)
    frame, _ = fresh.render(cam, num_samples=2, max_bounce=4)
    fresh.close()
    o = np.repeat(cs.pos, 16, axis=0)
    d = np.ascontiguousarray(want["directions"].reshape(-1, 3))
    for mode, flags in MODES.items():
        img, _ = rs.render(cam, num_samples=2, max_bounce=4, flags=native.FLAG_KERNEL_TIMES)
        assert np.array_equal(img, frame), f"render before a {mode} call"
        prof = rs.context.profile()
        a = call(rs.context, cs.pos, 16, 3, 4, flags=flags)
        assert rs.context.profile() == prof, "zrt_context_profile's record is the last render's"
        img, _ = rs.render(cam, num_samples=2, max_bounce=4)
        assert np.array_equal(img, frame), f"render after a {mode} call"
        rad = rs.radiance(o, d, 3, 4, seed=SEED, flags=flags)
        assert np.array_equal(bits(rad["radiance"]), bits(want["radiance"])), mode
        b = call(rs.context, cs.pos, 16, 3, 4, flags=flags)
        for k in OUTPUTS:
            assert np.array_equal(a[k], b[k]), (mode, k)
        check(a, want, mode)


def test_seed_and_index_base_change_the_directions(case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    a = call(rs.context, cs.pos, 16, 1, 1)
    b = call(rs.context, cs.pos, 16, 1, 1, seed=SEED + 1)
    c = call(rs.context, cs.pos, 16, 1, 1, index_base=1)
    assert not np.array_equal(a["directions"], b["directions"])
    assert np.array_equal(a["directions"][3:], c["directions"][:-3])      # the keys moved by one item
    n2 = (a["directions"].view(F).reshape(-1, 3).astype(np.float64) ** 2).sum(1)
    assert np.abs(n2 - 1).max() < 1e-6


def test_the_wrappers_shapes_and_tensors(case, scene):
    cs, rs = case("cornell_bm"), scene("cornell_bm")
    want = cs.want(16, 3, 4)
    n = len(cs.pos)
    res = rs.light_probes(cs.pos, 16, 3, 4, seed=SEED, distance=True, hits=True, directions=True, radiance=True)
    assert res["sh"].shape == (n, 9, 3) and res["distance"].shape == (n, 2) and res["hits"].shape == (n,)
    assert res["directions"].shape == res["radiance"].shape == (n, 16, 3) and res["hits"].dtype == np.uint32
    for k in OUTPUTS:
        assert np.array_equal(bits(res[k]), bits(want[k])), k
    only = rs.light_probes(cs.pos, 16, 3, 4, seed=SEED)
    assert sorted(only) == ["sh", "stats"] and np.array_equal(bits(only["sh"]), bits(want["sh"]))
    with pytest.raises(ValueError):
        rs.light_probes(cs.pos, 16, 3, 4, sh=False)
    if not have_torch():
        return
    t = rs.light_probes(torch.from_numpy(cs.pos).to("cuda:0"), 16, 3, 4, seed=SEED, distance=True, hits=True,
                        directions=True, radiance=True)
    assert t["sh"].shape == (n, 9, 3) and t["sh"].is_cuda and t["hits"].dtype == torch.int32
    for k in OUTPUTS:
        assert np.array_equal(bits(t[k].cpu().numpy().view(np.uint32)), bits(want[k])), k
    check_stats(t["stats"], want, "tensors")


def test_empty_and_bad_batches_on_a_live_context(scene):
    ctx = scene("cornell_bm").context
    out = np.full(64, 0xABABABAB, np.uint32)
    pos = np.zeros(3, F)
    x, p = pos.ctypes.data, out.ctypes.data
    st = ctx.light_probes_raw(0, x, p, p, p, p, p, False, 4, 1, 1)
    assert st["segments"] == 0 and st["hits"] == 0 and st["samples"] == 0
    ctx.light_probes_raw(0, None, None, None, None, None, None, False, 4, 1, 1, flags=native.TRACE_PARK)
    z = ctx.light_probes(np.zeros((0, 3), F), 4, 1, 1, distance=True, hits=True, directions=True, radiance=True)
    assert z["sh"].shape == (0, 9, 3) and z["directions"].shape == (0, 4, 3) and z["hits"].shape == (0,)
    ok = dict(pos=x, sh=p, D=4, S=1, mb=1, flags=0, reserved=0, dev=False)
    for kw, status in ((dict(pos=None), -1), (dict(sh=None), -1), (dict(dev=2), -1), (dict(reserved=1), -1),
                       (dict(D=0), -1), (dict(D=65536), -1), (dict(S=0), -1), (dict(S=65536), -1), (dict(mb=0), -1),
                       (dict(mb=33), -5), (dict(flags=native.RADIANCE_PER_SAMPLE), -1),
                       (dict(flags=native.FLAG_COUNT_STATS), -1), (dict(flags=native.FLAG_ONE_SET), -1),
                       (dict(flags=native.SEGMENT_ANY), -1), (dict(flags=native.DIRECT_UNSHADOWED), -1),
                       (dict(flags=0x4), -1)):
        a = dict(ok)
        a.update(kw)
        batch = native.LightProbeBatch(1, a["pos"], a["sh"], None, None, None, None, a["dev"], a["flags"], a["D"],
                                       a["S"], a["mb"], a["reserved"], 0, 0)
        assert native.lib().zrt_context_light_probes(ctx._h, C.byref(batch), None) == status, kw
    assert (out == 0xABABABAB).all()
    ctx.light_probes_raw(1, x, p, None, None, None, None, False, 4, 1, 32)      # the control: the valid batch runs
    assert (out[:27] != 0xABABABAB).any() and (out[27:] == 0xABABABAB).all()
