#!/usr/bin/env python3
"""Time and error of area-light queries (zrt_context_area_lights), device
batches (torch tensors), in one process:

  the call        Context.area_lights, S samples per ray, 16 crossings at most;
  unshadowed      the same call with ZRT_AREA_UNSHADOWED (no chain is walked);
  the composed    Context.surface -> per (ray, sample) the emitter (torch.randint
                  below Q and torch.searchsorted over C), the point on it
                  (torch.rand, folded), w, b, g and the traced mask, all with
                  torch on the device -> the traced items' rays gathered ->
                  Context.transmittance over them -> the samples summed per ray
                  with torch.  Its draws are torch's and it samples no texture
                  (Le = the emitter's material maximum, alpha = 1), so its sums
                  are another estimate of the same integral only where the
                  emitters are untextured; the work is the same or less.

Two scenes, each through a camera 512 pixels high: the cfg3 contest scene and
the Cornell box (cfg2).  Sizes are ITEMS (rays x samples): 2^lg / S rays per
call.  Times are the host clock around a synchronised call (two warm-up calls
per variant, then `--rounds` rounds alternating all variants, the median of
each round kept) and the call's own device time once (zrt_stats.render_ms).

Then the set's build time for both scenes, and on cfg2 the mean absolute error
of `radiance` and of Context.radiance(max_bounce = 2) against a 4096-sample
Context.radiance(max_bounce = 2) run, at equal samples and at equal device
time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from zig_raytracing_contest_amd import Config, RenderScene, camera_for, native, scenes  # noqa: E402
from segment_bench import camera_rays  # noqa: E402

H = 512
CAP = 16


def unit(v):
    return v / torch.sqrt((v * v).sum(-1, keepdim=True))


class TorchSet:
    """The set's records on the device as torch tensors."""

    def __init__(self, em, soup, dev):
        rec, C = em.read()
        self.count, self.Q = em.info()[:2]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.C = t(C.astype(np.int64))
        self.v0, self.e1, self.e2, self.a = t(rec["v0"]), t(rec["e1"]), t(rec["e2"]), t(rec["a"])
        self.q = t(rec["q"].astype(np.float32))
        n = np.cross(rec["e1"].astype(np.float64), rec["e2"].astype(np.float64))
        self.n = t((n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)).astype(np.float32))
        mm = []
        for m in np.asarray(soup.tex_desc).reshape(-1, 3, 7):
            off, w, h = (int(x) for x in m[1][:3])
            mm.append(np.fmax.reduce(np.append(np.float32(0), np.asarray(soup.texels, np.float32)[off:off + 3 * w * h])))
        self.Le = t(np.asarray(mm, np.float32)[rec["material"]])


def composed(ctx, ts, o, d, S):
    """What a caller writes without the call; (irradiance (n,), traced items) on the device."""
    n = o.shape[0]
    surf = ctx.surface(o, d)["surfaces"]
    hit = surf[:, 3].view(torch.int32) != -1
    pos, N = surf[:, 0:3], unit(surf[:, 4:7])
    shaded = hit & torch.isfinite(pos).all(1) & torch.isfinite(N).all(1)
    k = torch.searchsorted(ts.C, torch.randint(0, ts.Q, (n, S), device=o.device), right=True) - 1
    bu, bv = torch.rand((n, S), device=o.device), torch.rand((n, S), device=o.device)
    fold = bu + bv > 1
    bu, bv = torch.where(fold, 1 - bu, bu), torch.where(fold, 1 - bv, bv)
    y = ts.v0[k] + ts.e1[k] * bu[..., None] + ts.e2[k] * bv[..., None]
    v = y - pos[:, None, :]
    d2 = (v * v).sum(-1)
    b = torch.sqrt(d2)
    w = v / b[..., None]
    c = (N[:, None, :] * w).sum(-1)
    cl = -(ts.n[k] * w).sum(-1)
    TR = shaded[:, None] & (c > 0) & (cl > 0)
    g = c * cl / d2 * (float(ts.Q) / ts.q[k] * ts.a[k])
    T = torch.ones((n, S), dtype=torch.float32, device=o.device)
    po = pos[:, None, :].expand(n, S, 3)[TR].contiguous()
    if po.shape[0]:
        T[TR] = ctx.transmittance(po, w[TR].contiguous(), (b[TR] * (1 - 2.0 ** -10)).contiguous(),
                                  max_crossings=CAP)["transmittance"]
    E = (torch.where(TR, g * T, torch.zeros((), device=o.device)) * ts.Le[k]).sum(1) / S       # (one channel: Le is a maximum)
    return E, int(po.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 18, 20], help="items (rays x samples) per call")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_lights_bench.json"))
    a = ap.parse_args()
    if native.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("area_lights_bench: no HIP device (a time is measured on the GPU or not at all)")
    dev = torch.device("cuda", 0)
    log_path = os.path.splitext(a.out)[0] + ".log"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(log_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def measure(variants, calls):
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

    out = {"rounds": a.rounds, "max_crossings": CAP, "cases": [], "build": [], "error": []}
    cfgd = dict(scenes.CONFIGS["cfg3"])
    todo = (("cfg3", scenes.get_scene(cfgd["scene"]), cfgd["camera"],
             Config.load(os.path.join(ROOT, "config.json")).grid_resolution),
            ("cfg2", scenes.get_scene("cornell"), None, (16, 16, 16)))
    for sname, soup, camera, res in todo:
        cam = camera_for(soup, camera, None if soup.camera(camera).aspect else H, H)
        rs = RenderScene(soup, res, device=0)
        ctx = rs.context
        pos, uv = np.asarray(soup.pos, np.float32).reshape(-1, 9), np.asarray(soup.uv, np.float32).reshape(-1, 6)
        builds = []
        for _ in range(5):
            t0 = time.perf_counter()
            em = native.Emitters(ctx, pos, uv, soup.mat)
            builds.append((time.perf_counter() - t0) * 1e3)
            em.close()
        em = rs.emitters()
        count, Q, ntri = em.info()
        out["build"].append({"scene": sname, "triangles": ntri, "emitters": count, "Q": Q, "host_clock_ms": builds})
        say(f"{sname:5s} set build: {ntri} triangles -> {count} emitters, Q {Q}: " +
            " / ".join(f"{x:.3f}" for x in builds) + " ms (host clock, upload included)")
        ts = TorchSet(em, soup, dev)
        for S in a.samples:
            for lg in a.log2:
                n = (1 << lg) // S
                rays = torch.from_numpy(camera_rays(cam, n, 1)).to(dev)
                o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
                res_c = ctx.area_lights(o, d, em, S, max_crossings=CAP)
                res_u = ctx.area_lights(o, d, em, S, max_crossings=CAP, unshadowed=True)
                E_c, traced = composed(ctx, ts, o, d, S)
                st = res_c["stats"]
                variants = {"call": lambda: wall(lambda: ctx.area_lights(o, d, em, S, max_crossings=CAP)),
                            "unshadowed": lambda: wall(lambda: ctx.area_lights(o, d, em, S, max_crossings=CAP,
                                                                               unshadowed=True)),
                            "composed": lambda: wall(lambda: composed(ctx, ts, o, d, S))}
                med = measure(variants, min(30, max(5, (1 << 22) >> lg)))
                row = {"scene": sname, "items": n * S, "rays": n, "samples": S, "traced_items": st["samples"],
                       "composed_traced_items": traced, "chain_segments": st["segments"] - n, "crossings": st["hits"],
                       "launches": st["trace_launches"], "device_ms_once": st["render_ms"],
                       "unshadowed_device_ms_once": res_u["stats"]["render_ms"],
                       "mean_irradiance": float(res_c["irradiance"].max(1).values.mean()), "composed_mean_irradiance": float(E_c.mean()),
                       "host_clock_ms": med,
                       "faster_than_composed": all(x < y for x, y in zip(med["call"], med["composed"]))}
                out["cases"].append(row)
                say(f"{sname:5s} 2^{lg:<2d} items S {S:<2d} " +
                    "  ".join(f"{k} {' / '.join(f'{x:.4f}' for x in v)}" for k, v in med.items()) +
                    f" ms (host clock)  device once {st['render_ms']:.4f} / unshadowed {res_u['stats']['render_ms']:.4f} ms"
                    f"  traced {st['samples']} (composed {traced}) chain segments {row['chain_segments']}"
                    f" crossings {st['hits']} launches {st['trace_launches']}"
                    f" mean E {row['mean_irradiance']:.5f} (composed {row['composed_mean_irradiance']:.5f})"
                    f" faster than composed {row['faster_than_composed']}")
        if sname == "cfg2":
            n = 1 << 14
            rays = torch.from_numpy(camera_rays(cam, n, 2)).to(dev)
            o, d = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
            want = ctx.radiance(o, d, 4096, 2, seed=99)["radiance"]
            for S in (4, 16, 64):
                ar = ctx.area_lights(o, d, em, S, max_crossings=CAP, seed=5, irradiance=False, radiance=True)
                pt = ctx.radiance(o, d, S, 2, seed=5, stats=True)
                t_a, t_p = ar["stats"]["render_ms"], pt["stats"]["render_ms"]
                # equal device time: the path tracer with as many samples as fit the call's time
                S_eq = max(1, int(round(S * t_a / max(t_p, 1e-9))))
                pe = ctx.radiance(o, d, S_eq, 2, seed=5, stats=True)
                mae = lambda x: float((x - want).abs().mean())
                row = {"rays": n, "samples": S, "area_lights_ms": t_a, "radiance_ms": t_p, "mae_area_lights": mae(ar["radiance"]),
                       "mae_radiance_equal_samples": mae(pt["radiance"]), "equal_time_samples": S_eq,
                       "radiance_equal_time_ms": pe["stats"]["render_ms"], "mae_radiance_equal_time": mae(pe["radiance"]),
                       "reference_mean": float(want.mean())}
                out["error"].append(row)
                say(f"cfg2 error, {n} rays, S {S}: area_lights {t_a:.3f} ms MAE {row['mae_area_lights']:.6f};"
                    f" radiance(mb 2) S {S} {t_p:.3f} ms MAE {row['mae_radiance_equal_samples']:.6f};"
                    f" S {S_eq} {row['radiance_equal_time_ms']:.3f} ms MAE {row['mae_radiance_equal_time']:.6f}"
                    f" (4096-sample reference mean {row['reference_mean']:.5f})")
        rs.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    log.close()


if __name__ == "__main__":
    main()
