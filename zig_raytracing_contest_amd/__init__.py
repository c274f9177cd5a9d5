"""MI355X-native render hot path of tigrazone/zig_raytracing_contest.

Host-side mirror of the reference's interface around the one accelerated
seam, `Scene.render(threads, camera, img)` (src/stage3.zig:247):

  * `Config`       -- main.zig:56-69 config.json (grid_resolution, num_threads,
                      num_samples, max_bounce), same keys, same file.
  * `RenderScene`  -- stage2 Geometry.build + bakeInto (host C++, libzrt) and
                      the device-resident scene; `.render(camera, img)` is the
                      drop-in for Scene.render (HIP kernels on gfx950).
  * `camera_for`   -- stage1.loadCamera rules (width/height/aspect ratio).

Everything computes through libzrt.so (include/zrt.h).  There is no CPU
fallback: without the HIP library or a GPU, rendering raises.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Optional, Tuple

import numpy as np

from . import native

__all__ = ["Config", "RenderScene", "camera_for", "native"]


@dataclasses.dataclass
class Config:
    """main.zig:56-69; parsed strictly like std.json (unknown keys rejected)."""
    grid_resolution: Tuple[int, int, int] = (128, 128, 128)
    num_threads: Optional[int] = None
    num_samples: int = 3
    max_bounce: int = 4

    @classmethod
    def load(cls, path: str = "config.json") -> "Config":
        with open(path) as f:
            d = json.load(f)
        keys = {"grid_resolution", "num_threads", "num_samples", "max_bounce"}
        unknown = set(d) - keys
        if unknown:
            raise ValueError(f"UnknownField: {sorted(unknown)}")
        missing = {"grid_resolution", "num_samples", "max_bounce"} - set(d)
        if missing:
            raise ValueError(f"MissingField: {sorted(missing)}")
        gr = d["grid_resolution"]
        if not (isinstance(gr, list) and len(gr) == 3 and all(isinstance(x, int) and 0 <= x < 2**32
                                                              for x in gr)):
            raise ValueError("grid_resolution must be [u32, u32, u32]")
        nt = d.get("num_threads")
        if nt is not None and not (isinstance(nt, int) and 0 <= nt < 256):
            raise ValueError("num_threads must be null or u8")
        for k in ("num_samples", "max_bounce"):
            if not (isinstance(d[k], int) and 0 <= d[k] < 65536):
                raise ValueError(f"{k} must be u16")
        return cls(tuple(gr), nt, d["num_samples"], d["max_bounce"])


def camera_for(soup, name=None, width=None, height=None) -> native.Camera:
    """stage1.zig:309-371: find the camera by name, apply the size rules."""
    c = soup.camera(name)
    return native.camera_from_matrix(c.matrix, c.yfov, c.aspect, width, height)


class RenderScene:
    """Baked scene on one GPU; `render` mirrors stage3.Scene.render."""

    def __init__(self, soup, resolution=(128, 128, 128), device: int = -1, num_threads: int = 0,
                 device_build: bool = False):
        """device_build: stage 2 on the GPU straight into the context
        (zrt_context_create_built); otherwise host threads + upload."""
        self.soup = soup
        self._keep = []
        if device_build:
            self.geometry = None
            mats = native.Scene()
            native.attach_materials(mats, soup.tex_desc, soup.texels, self._keep)
            self.context = native.Context.built(soup.pos, soup.nrm, soup.uv, soup.mat, mats,
                                                resolution, device)
            return
        self.geometry = native.Geometry(soup.pos, soup.nrm, soup.uv, soup.mat, resolution,
                                        num_threads)
        native.attach_materials(self.geometry.scene, soup.tex_desc, soup.texels, self._keep)
        self.context = native.Context(self.geometry.scene, device)

    def close(self):
        if getattr(self, "_emitters", None) is not None:
            self._emitters.close()
            self._emitters = None
        self.context.close()

    def render(self, camera: native.Camera, img: Optional[np.ndarray] = None, num_samples: int = 3,
               max_bounce: int = 4, seed: int = 0, rank: int = 0, num_ranks: int = 1,
               stats: bool = False, linear: bool = False, packed: bool = False,
               samples_per_pass: int = 0, flags: int = 0):
        """Fills img (h, w, 3) uint8 (this rank's pixels) and returns (img, extras)."""
        if img is None:
            img = np.zeros((camera.h, camera.w, 3), np.uint8)
        assert img.shape == (camera.h, camera.w, 3) and img.dtype == np.uint8 and \
            img.flags["C_CONTIGUOUS"]
        res = self.context.render(camera, num_samples, max_bounce, seed=seed, rank=rank,
                                  num_ranks=num_ranks, stats=stats, image=img, linear=linear,
                                  packed=packed, samples_per_pass=samples_per_pass, flags=flags)
        return img, res

    def trace(self, origins, dirs, flags: int = 0, stats: bool = False):
        """Scene.traceRay (stage3.zig:152-186) for a batch of rays: see
        native.Context.trace.  With numpy inputs and a host-built scene the
        result also holds "source_triangle": each hit's ref mapped through
        stage 2's Geometry.indices to the soup's triangle (native.MISS kept)."""
        res = self.context.trace(origins, dirs, flags=flags, stats=stats)
        if self.geometry is not None and "triangle" in res:
            ref = res["triangle"]
            hit = ref != native.MISS
            src = np.full(ref.shape, native.MISS, np.uint32)
            src[hit] = self.geometry.indices()[ref[hit]]
            res["source_triangle"] = src
        return res

    def segments(self, origins, dirs, t_max, any_hit: bool = False, flags: int = 0, stats: bool = False):
        """Scene.traceRay for rays with an end t_max (a scalar or one per
        ray), nearest or any hit: see native.Context.segments."""
        return self.context.segments(origins, dirs, t_max, any_hit=any_hit, flags=flags, stats=stats)

    def surface(self, origins, dirs, flags: int = 0, stats: bool = False, hits: bool = False):
        """The shading inputs at each ray's first hit (stage3.zig:199-206):
        see native.Context.surface.  With numpy inputs, hits=True and a
        host-built scene the result also holds "source_triangle", as trace()'s."""
        res = self.context.surface(origins, dirs, flags=flags, stats=stats, hits=hits)
        if self.geometry is not None and "triangle" in res:
            ref = res["triangle"]
            hit = ref != native.MISS
            src = np.full(ref.shape, native.MISS, np.uint32)
            src[hit] = self.geometry.indices()[ref[hit]]
            res["source_triangle"] = src
        return res

    def transmittance(self, origins, dirs, t_max=float("inf"), max_crossings: int = 16, flags: int = 0,
                      stats: bool = False, crossings: bool = False):
        """The expected pass-through of the path tracer's transparency chain
        along rays with an end t_max: see native.Context.transmittance."""
        return self.context.transmittance(origins, dirs, t_max, max_crossings=max_crossings, flags=flags,
                                          stats=stats, crossings=crossings)

    def features(self, camera: native.Camera, num_samples: int = 3, seed: int = 0, **kw):
        """The auxiliary planes (first-hit base colour, normal, emission,
        depth, transparency, hit count) of the frame render(camera,
        num_samples, seed=seed) gives: see native.Context.features."""
        return self.context.features(camera, num_samples, seed=seed, **kw)

    def denoise(self, w: int, h: int, **kw):
        """The edge-avoiding a-trous filter over a colour frame or a film's
        frame so far, guided by the feature planes: see native.Context.denoise."""
        return self.context.denoise(w, h, **kw)

    def reproject(self, camera: native.Camera, prev_camera: native.Camera, **kw):
        """The previous frame's history carried across a camera change and
        blended with the current colour: see native.Context.reproject."""
        return self.context.reproject(camera, prev_camera, **kw)

    def history(self, w: int, h: int, **kw):
        """A native.History of this scene's context: the buffers of a preview
        under a moving camera."""
        return native.History(self.context, w, h, **kw)

    def occlusion(self, origins, dirs, spp: int, radius=float("inf"), seed: int = 0, index_base: int = 0,
                  flags: int = 0, stats: bool = False, hits: bool = False):
        """Hemisphere visibility at each ray's first hit, `spp` samples of the
        path tracer's own scatter directions within `radius`: see
        native.Context.occlusion."""
        return self.context.occlusion(origins, dirs, spp, radius, seed=seed, index_base=index_base, flags=flags,
                                      stats=stats, hits=hits)

    def direct(self, origins, dirs, lights, max_crossings: int = 16, flags: int = 0, unshadowed: bool = False,
               irradiance: bool = True, radiance: bool = False, hits: bool = False, stats: bool = False):
        """Direct light of punctual lights (native.Light) at each ray's first
        hit, shadowed through transparent hits: see native.Context.direct."""
        return self.context.direct(origins, dirs, lights, max_crossings=max_crossings, flags=flags,
                                   unshadowed=unshadowed, irradiance=irradiance, radiance=radiance, hits=hits,
                                   stats=stats)

    def emitters(self):
        """The native.Emitters of this scene's own emissive triangles (its soup
        and the context's materials), built on first use and kept."""
        if getattr(self, "_emitters", None) is None:
            self._emitters = native.Emitters(self.context, np.asarray(self.soup.pos, np.float32).reshape(-1, 9),
                                             np.asarray(self.soup.uv, np.float32).reshape(-1, 6), self.soup.mat)
        return self._emitters

    def area_lights(self, origins, dirs, spp: int, emitters=None, **kw):
        """Direct light of the scene's emissive triangles at each ray's first
        hit, `spp` next-event samples per ray (emitters: a native.Emitters,
        by default this scene's own): see native.Context.area_lights."""
        return self.context.area_lights(origins, dirs, self.emitters() if emitters is None else emitters, spp, **kw)

    def sky_light(self, origins, dirs, spp: int, **kw):
        """The sky's direct light at each ray's first hit, `spp` cosine-weighted
        hemisphere samples per ray shadowed through transparent hits: see
        native.Context.sky_light."""
        return self.context.sky_light(origins, dirs, spp, **kw)

    def light_probes(self, positions, num_directions: int, spp: int, max_bounce: int, seed: int = 0,
                     index_base: int = 0, flags: int = 0, sh: bool = True, distance: bool = False, hits: bool = False,
                     directions: bool = False, radiance: bool = False):
        """Order-2 SH radiance, first-hit distance moments and hit counts at
        points, from `num_directions` device-made directions of `spp` paths
        each: see native.Context.light_probes."""
        return self.context.light_probes(positions, num_directions, spp, max_bounce, seed=seed, index_base=index_base,
                                         flags=flags, sh=sh, distance=distance, hits=hits, directions=directions,
                                         radiance=radiance)

    def radiance(self, origins, dirs, spp: int, max_bounce: int, seed: int = 0, index_base: int = 0,
                 flags: int = 0, rgb: bool = False, stats: bool = False):
        """Scene.traceRayRecursive (stage3.zig:188-220) for a batch of rays,
        `spp` path samples each: see native.Context.radiance."""
        return self.context.radiance(origins, dirs, spp, max_bounce, seed=seed, index_base=index_base,
                                     flags=flags, rgb=rgb, stats=stats)
