#!/usr/bin/env python3
"""Device time of transmittance queries (zrt_context_transmittance) against the
calls a direct-light pass has today, in the same process, device batches
(torch tensors), lane walk and park path both forced:

  (a) opaque   the cfg3 contest scene, segment_bench.py's `shadow` and `ao_0.25`
               ray sets through this call and through zrt_context_segments
               any-hit on the same rays (zrt_stats.trace_kernel_ms): where
               almost nothing is transparent the difference is what the alpha
               lookup and the chain's bookkeeping cost;
  (b) alpha    a canopy of BLEND panes (alpha 128 / 255) and MASK leaf cards in
               four layers over a ground plane; rays from the ground towards a
               light above the layers, t_max = the distance.  This call against
               the loop a caller writes today: segments (closest) -> surface on
               the hits -> T, origin and bound updated and the survivors
               compacted with torch on the device -> repeat.  Both are timed by
               the host clock around a synchronised call, the results compared
               bit for bit first;
  (c) rounds   the park path's ways to end its round loop on both scenes: the
               survivor counts read back after each round and a small remainder
               handed to one lane launch (the default), the read-back with every
               round run (ZRT_TRANSMIT_TAIL=0), or max_crossings rounds without a
               read-back (ZRT_TRANSMIT_ROUNDS=fixed).

Per size: two warm-up calls per variant, then `--rounds` rounds alternating all
variants, the median of each round kept.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402
from segment_bench import cosine_dirs, surface_points  # noqa: E402

PATHS = {"lane": native.FLAG_LANE_WALK, "park": native.TRACE_PARK}
EPS = float(np.finfo(np.float32).eps)
CAP = 16


def canopy_scene():
    """Ground, four layers of 40 x 40 quads over it -- BLEND panes and MASK
    leaf cards by turns -- and a few opaque boxes."""
    mb = scenes.MeshBuilder()
    textures = [scenes.Texture(scenes._checker(16, 4, alpha=128)), scenes.Texture(scenes._leaf_mask(32, 3))]
    mats = [scenes.Material(base_color=(0.8, 0.8, 0.8, 1), name="ground"),
            scenes.Material(base_color=(1, 1, 1, 1), base_texture=0, alpha_mode="BLEND", name="pane"),
            scenes.Material(base_color=(1, 1, 1, 1), base_texture=1, alpha_mode="MASK", name="leaf"),
            scenes.Material(base_color=(0.7, 0.3, 0.2, 1), name="box")]
    mb.quad((-20, 0, 20), (20, 0, 20), (20, 0, -20), (-20, 0, -20), 0, nu=40, nv=40)
    for k, y in enumerate((2.0, 4.0, 6.0, 8.0)):        # facing down: shadow rays come from below
        mb.quad((-20, y, -20), (20, y, -20), (20, y, 20), (-20, y, 20), 1 + k % 2, uv_scale=(40, 40), nu=40, nv=40)
        mb.quad((-20, y, 20), (20, y, 20), (20, y, -20), (-20, y, -20), 1 + k % 2, uv_scale=(40, 40), nu=40, nv=40)
    rng = np.random.default_rng(1)
    for _ in range(20):
        x, z = rng.uniform(-15, 15, 2)
        mb.box((x - 0.5, 0, z - 0.5), (x + 0.5, float(rng.uniform(1, 7)), z + 0.5), 3)
    pos, nrm, uv, mat = mb.soup()
    cams = [scenes.CameraDef("Camera", scenes.look_at((0, 1, 25), (0, 4, 0)), math.radians(50.0), 16 / 9)]
    return scenes.SceneSoup("canopy", pos, nrm, uv, mat, mats, textures, cams).bake_materials()


def canopy_rays(n, seed):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-18, 18, n), np.full(n, 1e-3), rng.uniform(-18, 18, n)], axis=1).astype(np.float32)
    to = np.array([4.0, 30.0, -3.0], np.float32) - p
    dist = np.sqrt((to * to).sum(1, dtype=np.float32), dtype=np.float32)
    return p, (to / dist[:, None]).astype(np.float32), dist


def composed(ctx, o, d, b, flags, cap=CAP):
    """What a caller writes today; (T, crossings) as torch tensors."""
    n = o.shape[0]
    T = torch.ones(n, dtype=torch.float32, device=o.device)
    cr = torch.zeros(n, dtype=torch.int32, device=o.device)
    idx = torch.arange(n, device=o.device)
    for k in range(cap):
        seg = ctx.segments(o, d, b, flags=flags)
        hit = seg["occluded"]
        if not bool(hit.any()):
            break
        idx, o, d, b, t = idx[hit], o[hit], d[hit], b[hit], seg["hits"][hit, 0]
        surf = ctx.surface(o.contiguous(), d.contiguous(), flags=flags)["surfaces"]
        p = 1.0 - surf[:, 7]
        go = p > 0
        T[idx] = torch.where(go, T[idx] * torch.clamp(p, max=1.0), torch.zeros_like(p))
        cr[idx] += 1
        if k + 1 == cap:
            break
        idx, o, d = idx[go], surf[go, 0:3].contiguous(), d[go].contiguous()
        b = (b[go] - (t[go] + EPS)).contiguous()
        if idx.numel() == 0:
            break
    return T, cr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmit_bench.json"))
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("transmit_bench: no HIP device (a time is measured on the GPU or not at all)")
    dev = torch.device("cuda", 0)
    log_path = os.path.splitext(a.out)[0] + ".log"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(log_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def rounds_env(ending):
        """None: the default (read-back, the tail); "every_round": read-back, no tail; "fixed": no read-back."""
        os.environ.pop("ZRT_TRANSMIT_ROUNDS", None)
        os.environ.pop("ZRT_TRANSMIT_TAIL", None)
        if ending == "fixed":
            os.environ["ZRT_TRANSMIT_ROUNDS"] = "fixed"
        elif ending == "every_round":
            os.environ["ZRT_TRANSMIT_TAIL"] = "0"

    def measure(variants, calls):
        """variants: name -> callable returning ms; the median per round."""
        for f in variants.values():
            f()
            f()
        med = {k: [] for k in variants}
        for _ in range(a.rounds):
            ms = {k: [] for k in variants}
            for _ in range(calls):
                for k, f in variants.items():
                    ms[k].append(f())
            for k in variants:
                med[k].append(float(np.median(ms[k])))
        return med

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"rounds": a.rounds, "cap": CAP, "opaque": [], "alpha": []}

    # ---- (a), (c): the cfg3 scene
    cfgd = dict(scenes.CONFIGS["cfg3"])
    soup = scenes.get_scene(cfgd["scene"])
    cam = camera_for(soup, cfgd["camera"], cfgd["width"], cfgd["height"])
    rs = RenderScene(soup, Config.load(os.path.join(ROOT, "config.json")).grid_resolution, device=0)
    ctx = rs.context
    xyz = soup.pos.reshape(-1, 3)
    lo, hi = xyz.min(0).astype(np.float32), xyz.max(0).astype(np.float32)
    diag = np.float32(np.linalg.norm(hi - lo))
    light = (lo + np.array([0.5, 0.8, 0.5], np.float32) * (hi - lo)).astype(np.float32)
    for lg in a.log2:
        n = 1 << lg
        p, back, _ = surface_points(ctx, cam, n, diag)
        to = light - p
        dist = np.sqrt((to * to).sum(1, dtype=np.float32), dtype=np.float32)
        sets = {"shadow": (np.concatenate([p, to / dist[:, None]], axis=1).astype(np.float32), dist),
                "ao_0.25": (np.concatenate([p, cosine_dirs(back.astype(np.float64), 3)], axis=1),
                            np.full(n, np.float32(0.25) * diag, np.float32))}
        for sname, (rays, tm) in sets.items():
            r, t = up(rays.astype(np.float32)), up(tm)
            T = torch.empty(n, dtype=torch.float32, device=dev)
            occ = torch.empty(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def tr(path, ending=None):
                rounds_env(ending)
                ms = ctx.transmittance_raw(n, r.data_ptr(), t.data_ptr(), T.data_ptr(), None, True, PATHS[path],
                                           max_crossings=CAP)["trace_kernel_ms"]
                rounds_env(None)
                return ms

            def sg(path):
                return ctx.segments_raw(n, r.data_ptr(), t.data_ptr(), None, occ.data_ptr(), True,
                                        PATHS[path] | native.SEGMENT_ANY)["trace_kernel_ms"]
            # where nothing is transparent the two agree exactly; leaf cards make T = 1 behind an occluded byte
            sg("lane")
            tr("lane")
            Tl = T.clone()
            tr("park")
            assert torch.equal(Tl, T), "park = lane"
            for ending in ("every_round", "fixed"):
                tr("park", ending)
                assert torch.equal(Tl, T), ending
            blocked, occl = float((Tl == 0).float().mean()), float((occ != 0).float().mean())
            med = measure({"lane_transmit": lambda: tr("lane"), "lane_any": lambda: sg("lane"),
                           "park_transmit": lambda: tr("park"), "park_any": lambda: sg("park"),
                           "park_every_round": lambda: tr("park", "every_round"),
                           "park_fixed": lambda: tr("park", "fixed")}, min(200, max(5, (1 << 23) // n)))
            out["opaque"].append({"set": sname, "rays": n, "blocked_fraction": blocked, "occluded_fraction": occl, "ms": med})
            say(f"opaque {sname:8s} 2^{lg:<2d} " + "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                f" ms  T = 0: {blocked:.3f}, any-hit occluded {occl:.3f}")
    rs.close()

    # ---- (b), (c): the canopy
    soup = canopy_scene()
    rs = RenderScene(soup, (64, 32, 64), device=0)
    ctx = rs.context
    for lg in a.log2:
        n = 1 << lg
        p, d, dist = canopy_rays(n, 5)
        o_t, d_t, b_t = up(p), up(d), up(dist)
        res = {}
        for path, f in PATHS.items():
            res[path] = ctx.transmittance(o_t, d_t, b_t, max_crossings=CAP, flags=f, crossings=True)
            Tc, crc = composed(ctx, o_t, d_t, b_t, f)
            assert torch.equal(Tc, res[path]["transmittance"]) and torch.equal(crc, res[path]["crossings"]), path
        assert torch.equal(res["lane"]["transmittance"], res["park"]["transmittance"])
        for ending in ("every_round", "fixed"):
            rounds_env(ending)
            fx = ctx.transmittance(o_t, d_t, b_t, max_crossings=CAP, flags=native.TRACE_PARK, crossings=True)
            rounds_env(None)
            assert torch.equal(fx["transmittance"], res["park"]["transmittance"]), ending
        cr = res["lane"]["crossings"].float()
        Tm = res["lane"]["transmittance"]

        def call(path, ending=None):
            rounds_env(ending)
            ms = wall(lambda: ctx.transmittance(o_t, d_t, b_t, max_crossings=CAP, flags=PATHS[path]))
            rounds_env(None)
            return ms
        med = measure({"lane_transmit": lambda: call("lane"),
                       "lane_composed": lambda: wall(lambda: composed(ctx, o_t, d_t, b_t, PATHS["lane"])),
                       "park_transmit": lambda: call("park"),
                       "park_composed": lambda: wall(lambda: composed(ctx, o_t, d_t, b_t, PATHS["park"])),
                       "park_every_round": lambda: call("park", "every_round"),
                       "park_fixed": lambda: call("park", "fixed")}, min(100, max(5, (1 << 22) // n)))
        row = {"rays": n, "mean_crossings": float(cr.mean()), "max_crossings": int(cr.max()),
               "between_fraction": float(((Tm > 0) & (Tm < 1)).float().mean()),
               "device_ms_once": {pa: res[pa]["stats"]["trace_kernel_ms"] for pa in PATHS},
               "launches": {pa: res[pa]["stats"]["trace_launches"] for pa in PATHS}, "host_clock_ms": med}
        row["faster_than_composed"] = {pa: all(x < y for x, y in zip(med[f"{pa}_transmit"], med[f"{pa}_composed"]))
                                       for pa in PATHS}
        out["alpha"].append(row)
        say(f"alpha canopy 2^{lg:<2d} " + "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
            f" ms (host clock)  crossings mean {row['mean_crossings']:.2f} max {row['max_crossings']}, 0 < T < 1: "
            f"{row['between_fraction']:.3f}, faster than composed: {row['faster_than_composed']}")
    rs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    log.close()


if __name__ == "__main__":
    main()
