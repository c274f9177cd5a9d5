"""ctypes binding of libzrt.so (include/zrt.h) -- the product's C ABI.

No fallback: if the HIP library is missing the import of `lib()` raises, so a
GPU test can never pass on a silent CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZRT_LIB: an alternative build of the library (tools/ tuning builds only)
LIB_PATH = os.environ.get("ZRT_LIB") or os.path.join(_HERE, "libzrt.so")
_lib = None

ZRT_OK = 0
STATUS = {0: "ok", -1: "invalid argument", -2: "no HIP device", -3: "HIP runtime error",
          -4: "out of memory", -5: "unsupported configuration", -6: "I/O error",
          -7: "parse error", -8: "not found", -9: "camera/output size rules violated"}
FLAG_COUNT_STATS, FLAG_LANE_WALK = 0x1, 0x2
FLAG_ESCAPE, FLAG_NO_ESCAPE = 0x40, 0x80
FLAG_FRUSTUM, FLAG_NO_FRUSTUM = 0x100, 0x200
FLAG_ONE_SET, FLAG_KERNEL_TIMES = 0x10, 0x20
FLAG_MT_EXACT = 0x400
FLAG_RELEASE, FLAG_NO_RELEASE = 0x800, 0x1000
FLAG_BFCULL, FLAG_NO_BFCULL = 0x2000, 0x4000
FLAG_HOP, FLAG_NO_HOP = 0x8000, 0x8
TRACE_PARK = 0x10000       # ZRT_TRACE_PARK (zrt_ray_batch / zrt_radiance_batch flags only)
RADIANCE_PER_SAMPLE = 0x20000   # ZRT_RADIANCE_PER_SAMPLE (zrt_radiance_batch.flags only)
SEGMENT_ANY = 0x40000      # ZRT_SEGMENT_ANY (zrt_segment_batch.flags only)
DIRECT_UNSHADOWED = 0x80000   # ZRT_DIRECT_UNSHADOWED (zrt_direct_batch.flags only)
AREA_UNSHADOWED = 0x800000    # ZRT_AREA_UNSHADOWED (zrt_area_light_batch.flags only)
SKY_UNSHADOWED = 0x1000000    # ZRT_SKY_UNSHADOWED (zrt_sky_light_batch.flags only)
DENOISE_ROW_MAJOR = 0x100000  # ZRT_DENOISE_ROW_MAJOR (zrt_denoise_batch.flags only)
# Context.denoise's default sigmas (colour, normal, depth, albedo): the C interface has none.  Chosen on the
# CPU reference over oracle frames: every finite sigma_color tried lowers the error of a
# 4-sample frame; these lower it most on the larger frames without blurring the textured scene
DENOISE_SIGMAS = (4.0, 0.5, 0.1, 0.25)
REPROJECT_ROW_MAJOR = 0x200000  # ZRT_REPROJECT_ROW_MAJOR (zrt_reproject_batch.flags only)
# Context.reproject's and History's defaults (max_history, depth_tolerance, normal_tolerance): the C interface
# has none.  The values the quality condition of tests/test_reproject_host.py is stated for
REPROJECT_DEFAULTS = (32, 0.05, 0.5)
SVGF_ROW_MAJOR = 0x400000  # ZRT_SVGF_ROW_MAJOR (zrt_illumination_batch.flags and zrt_svgf_batch.flags only)
# Context.svgf's default sigmas (luminance, in standard deviations; normal; depth): the C interface has none.
# The values the quality condition of tests/test_svgf_host.py is stated for
SVGF_SIGMAS = (4.0, 0.5, 0.1)
LIGHT_POINT, LIGHT_DIRECTIONAL, LIGHT_SPOT = 0, 1, 2
MISS = 0xFFFFFFFF          # zrt_hit.triangle of a ray that hit nothing
# zrt_kernel_profile classes (include/zrt.h)
KERNEL_CLASSES = ("primary", "park", "shade", "bounce", "resolve", "count")

PROBE_TRIANGLE, PROBE_BBOX, PROBE_DDA, PROBE_TO_RGB = 0, 1, 2, 3
PROBE_RNG_F32, PROBE_RNG_NORM, PROBE_EXP_LOG, PROBE_TEXTURE = 4, 5, 6, 7
PROBE_TRIANGLE_FLAT = 8
PROBE_RECIP, PROBE_RECIP_SWEEP, PROBE_TRIANGLE_EXACT = 9, 10, 11
PROBE_QUOT, PROBE_QUOT_SWEEP = 12, 13
DDA_PROBE_WIDTH = 4 + 4 * 64      # floats per ray: steps, first cell, 64 x (cell, t)


class ZrtError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__(f"{what}: {STATUS.get(status, status)} ({status})")


class Grid(C.Structure):
    _fields_ = [("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3),
                ("resolution", C.c_uint32 * 3), ("cell_size", C.c_float * 3)]


class Texture(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("w", C.c_int32), ("h", C.c_int32),
                ("u_min", C.c_int32), ("u_max", C.c_int32), ("v_min", C.c_int32),
                ("v_max", C.c_int32), ("_pad", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("base_color", Texture), ("emissive", Texture), ("transparency", Texture)]


class Scene(C.Structure):
    _fields_ = [("grid", Grid), ("num_cells", C.c_uint32), ("cells", C.POINTER(C.c_uint32)),
                ("num_triangles", C.c_uint32), ("triangles_pos", C.POINTER(C.c_float)),
                ("triangles_data", C.POINTER(C.c_float)),
                ("triangles_material", C.POINTER(C.c_uint32)), ("num_materials", C.c_uint32),
                ("materials", C.POINTER(Material)), ("texels", C.POINTER(C.c_float)),
                ("num_texel_floats", C.c_uint64)]


class Camera(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("origin", C.c_float * 3),
                ("lower_left_corner", C.c_float * 3), ("right", C.c_float * 3),
                ("up", C.c_float * 3)]

    def as_dict(self):
        return {"w": self.w, "h": self.h, "origin": list(self.origin),
                "llc": list(self.lower_left_corner), "right": list(self.right), "up": list(self.up)}


class RenderConfig(C.Structure):
    _fields_ = [("num_samples", C.c_uint32), ("max_bounce", C.c_uint32), ("seed", C.c_uint64),
                ("device", C.c_int32), ("rank", C.c_uint32), ("num_ranks", C.c_uint32),
                ("tile_size", C.c_uint32), ("flags", C.c_uint32), ("samples_per_pass", C.c_uint32),
                ("num_devices", C.c_uint32), ("_reserved0", C.c_uint32),
                ("devices", C.POINTER(C.c_int32))]


class Stats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("cells_visited", C.c_uint64),
                ("triangle_tests", C.c_uint64), ("hits", C.c_uint64), ("samples", C.c_uint64),
                ("render_ms", C.c_double), ("trace_kernel_ms", C.c_double),
                ("trace_launches", C.c_uint32), ("_pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("_")}


class KernelProfile(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_uint32 * 8), ("passes", C.c_uint32),
                ("sets", C.c_uint32), ("primary_counts", C.c_uint64 * 4)]

    def as_dict(self):
        return {"kernels": {k: {"ms": self.ms[i], "launches": int(self.launches[i])}
                            for i, k in enumerate(KERNEL_CLASSES) if self.launches[i]},
                "passes": int(self.passes), "sets": int(self.sets),
                "primary": dict(zip(("segments", "cells_visited", "triangle_tests", "hits"),
                                    (int(x) for x in self.primary_counts)))}


class Outputs(C.Structure):
    _fields_ = [("rgb_image", C.c_void_p), ("rgb_packed", C.c_void_p),
                ("linear_packed", C.c_void_p), ("device_rgb_packed", C.c_void_p)]


class RefineConfig(C.Structure):
    _fields_ = [("sample_counts", C.c_void_p), ("threshold", C.c_float), ("min_samples", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_uint32)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("triangle", "<u4")])


class RayBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("hits", C.c_void_p),
                ("on_device", C.c_uint32), ("flags", C.c_uint32)]


class SegmentBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("t_max", C.c_void_p), ("hits", C.c_void_p),
                ("occluded", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("t_max_all", C.c_float), ("_reserved", C.c_uint32)]


class Surface(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("material", C.c_uint32), ("normal", C.c_float * 3),
                ("transparency", C.c_float), ("base_color", C.c_float * 3), ("texcoord_s", C.c_float),
                ("emissive", C.c_float * 3), ("texcoord_t", C.c_float)]


SURFACE_DTYPE = np.dtype([("position", "<f4", (3,)), ("material", "<u4"), ("normal", "<f4", (3,)),
                          ("transparency", "<f4"), ("base_color", "<f4", (3,)), ("texcoord_s", "<f4"),
                          ("emissive", "<f4", (3,)), ("texcoord_t", "<f4")])


class SurfaceBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("surfaces", C.c_void_p), ("hits", C.c_void_p),
                ("on_device", C.c_uint32), ("flags", C.c_uint32)]


class TransmittanceBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("t_max", C.c_void_p), ("transmittance", C.c_void_p),
                ("crossings", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("t_max_all", C.c_float), ("max_crossings", C.c_uint32)]


class FeatureOutputs(C.Structure):
    _fields_ = [("base_color", C.c_void_p), ("normal", C.c_void_p), ("emissive", C.c_void_p), ("depth", C.c_void_p),
                ("transparency", C.c_void_p), ("hits", C.c_void_p), ("on_device", C.c_uint32),
                ("_reserved", C.c_uint32)]


# zrt_feature_outputs' planes: (name, floats or counts per pixel)
FEATURE_PLANES = (("base_color", 3), ("normal", 3), ("emissive", 3), ("depth", 1), ("transparency", 1), ("hits", 1))


class OcclusionBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("radius", C.c_void_p), ("visibility", C.c_void_p),
                ("occluded", C.c_void_p), ("hits", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("radius_all", C.c_float), ("num_samples", C.c_uint32), ("seed", C.c_uint64),
                ("index_base", C.c_uint64)]


class Light(C.Structure):
    """zrt_light.  Light.point / .directional / .spot build one; a spot's
    angle_scale and angle_offset come from its cone angles in float32:
    1 / max(0.001, cos_inner - cos_outer) and -cos_outer * angle_scale."""
    _fields_ = [("type", C.c_uint32), ("position", C.c_float * 3), ("direction", C.c_float * 3),
                ("color", C.c_float * 3), ("angle_scale", C.c_float), ("angle_offset", C.c_float)]

    @classmethod
    def point(cls, position, color):
        return cls(LIGHT_POINT, (C.c_float * 3)(*position), (C.c_float * 3)(), (C.c_float * 3)(*color), 0.0, 0.0)

    @classmethod
    def directional(cls, direction, color):
        return cls(LIGHT_DIRECTIONAL, (C.c_float * 3)(), (C.c_float * 3)(*direction), (C.c_float * 3)(*color), 0.0, 0.0)

    @classmethod
    def spot(cls, position, direction, color, inner_angle, outer_angle):
        """Cone angles in radians from the axis (KHR_lights_punctual's)."""
        ci, co = np.float32(np.cos(inner_angle)), np.float32(np.cos(outer_angle))
        scale = np.float32(1.0) / max(np.float32(0.001), np.float32(ci - co))
        return cls(LIGHT_SPOT, (C.c_float * 3)(*position), (C.c_float * 3)(*direction), (C.c_float * 3)(*color),
                   float(scale), float(np.float32(-co * scale)))


class DirectBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("lights", C.c_void_p), ("irradiance", C.c_void_p),
                ("radiance", C.c_void_p), ("hits", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("num_lights", C.c_uint32), ("max_crossings", C.c_uint32)]


class AreaLightBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("emitters", C.c_void_p), ("irradiance", C.c_void_p),
                ("radiance", C.c_void_p), ("hits", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("num_samples", C.c_uint32), ("max_crossings", C.c_uint32), ("seed", C.c_uint64),
                ("index_base", C.c_uint64)]


class SkyLightBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("irradiance", C.c_void_p), ("radiance", C.c_void_p),
                ("visibility", C.c_void_p), ("hits", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("num_samples", C.c_uint32), ("max_crossings", C.c_uint32), ("seed", C.c_uint64),
                ("index_base", C.c_uint64)]


# zrt_emitter, 80 bytes
EMITTER_DTYPE = np.dtype([("v0", np.float32, 3), ("a", np.float32), ("e1", np.float32, 3), ("q", np.uint32),
                          ("e2", np.float32, 3), ("material", np.uint32), ("texcoords", np.float32, 6),
                          ("triangle", np.uint32), ("_reserved", np.uint32)])


class LightProbeBatch(C.Structure):
    _fields_ = [("num_probes", C.c_uint64), ("positions", C.c_void_p), ("sh", C.c_void_p), ("distance", C.c_void_p),
                ("hits", C.c_void_p), ("directions", C.c_void_p), ("radiance", C.c_void_p), ("on_device", C.c_uint32),
                ("flags", C.c_uint32), ("num_directions", C.c_uint32), ("num_samples", C.c_uint32),
                ("max_bounce", C.c_uint32), ("_reserved", C.c_uint32), ("seed", C.c_uint64),
                ("index_base", C.c_uint64)]


class DenoiseBatch(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("tile_size", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float), ("color", C.c_void_p), ("film", C.c_void_p), ("normal", C.c_void_p),
                ("depth", C.c_void_p), ("albedo", C.c_void_p), ("linear", C.c_void_p), ("rgb", C.c_void_p),
                ("on_device", C.c_uint32), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class ReprojectBatch(C.Structure):
    _fields_ = [("tile_size", C.c_uint32), ("max_history", C.c_uint32), ("depth_tolerance", C.c_float),
                ("normal_tolerance", C.c_float), ("on_device", C.c_uint32), ("flags", C.c_uint32),
                ("camera", C.c_void_p), ("prev_camera", C.c_void_p), ("color", C.c_void_p), ("film", C.c_void_p),
                ("depth", C.c_void_p), ("normal", C.c_void_p), ("prev_color", C.c_void_p), ("prev_depth", C.c_void_p),
                ("prev_normal", C.c_void_p), ("prev_length", C.c_void_p), ("color_out", C.c_void_p),
                ("length_out", C.c_void_p), ("motion", C.c_void_p), ("_reserved", C.c_uint64)]


class IlluminationBatch(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("tile_size", C.c_uint32), ("color", C.c_void_p),
                ("film", C.c_void_p), ("albedo", C.c_void_p), ("illumination", C.c_void_p), ("moments", C.c_void_p),
                ("on_device", C.c_uint32), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class SvgfBatch(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("tile_size", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("color", C.c_void_p), ("moments", C.c_void_p), ("length", C.c_void_p), ("normal", C.c_void_p),
                ("depth", C.c_void_p), ("albedo", C.c_void_p), ("linear", C.c_void_p), ("rgb", C.c_void_p),
                ("variance", C.c_void_p), ("on_device", C.c_uint32), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class RadianceBatch(C.Structure):
    _fields_ = [("num_rays", C.c_uint64), ("rays", C.c_void_p), ("radiance", C.c_void_p), ("rgb", C.c_void_p),
                ("on_device", C.c_uint32), ("flags", C.c_uint32), ("num_samples", C.c_uint32),
                ("max_bounce", C.c_uint32), ("seed", C.c_uint64), ("index_base", C.c_uint64)]


EXPORTS = [
    "zrt_error_string", "zrt_abi_version", "zrt_device_count", "zrt_device_warmup", "zrt_geometry_build",
    "zrt_geometry_build_device",
    "zrt_geometry_scene", "zrt_geometry_indices", "zrt_geometry_free", "zrt_render",
    "zrt_context_create", "zrt_context_create_built", "zrt_context_grid_info", "zrt_context_render", "zrt_context_destroy", "zrt_tile_pixels",
    "zrt_gltf_load", "zrt_gltf_soup", "zrt_gltf_materials", "zrt_gltf_camera", "zrt_gltf_free",
    "zrt_camera_from_matrix", "zrt_probe", "zrt_timed_kernels", "zrt_context_profile", "zrt_context_trace",
    "zrt_group_create", "zrt_group_create_built", "zrt_group_render", "zrt_group_context", "zrt_group_destroy",
    "zrt_context_radiance", "zrt_context_segments", "zrt_context_surface", "zrt_context_transmittance",
    "zrt_context_features", "zrt_context_occlusion", "zrt_context_direct",
    "zrt_context_light_probes",
    "zrt_film_create", "zrt_film_reset", "zrt_film_info", "zrt_film_read", "zrt_film_write", "zrt_film_destroy",
    "zrt_context_accumulate",
    "zrt_context_refine", "zrt_film_counts",
    "zrt_context_denoise",
    "zrt_context_reproject",
    "zrt_context_illumination", "zrt_context_svgf",
    "zrt_emitters_create", "zrt_emitters_info", "zrt_emitters_read", "zrt_emitters_destroy",
    "zrt_context_area_lights",
    "zrt_context_sky_light",
]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libzrt.so not built at {LIB_PATH} (run `make` or "
                          "__graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    L.zrt_error_string.restype = C.c_char_p
    L.zrt_error_string.argtypes = [C.c_int]
    L.zrt_device_count.argtypes = [C.POINTER(C.c_int)]
    L.zrt_geometry_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_void_p)]
    L.zrt_geometry_build_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_void_p)]
    L.zrt_geometry_scene.argtypes = [C.c_void_p, C.POINTER(Scene)]
    L.zrt_geometry_indices.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)),
                                       C.POINTER(C.c_uint32)]
    L.zrt_geometry_free.argtypes = [C.c_void_p]
    L.zrt_geometry_free.restype = None
    L.zrt_render.argtypes = [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(RenderConfig),
                             C.c_void_p, C.POINTER(Stats)]
    L.zrt_context_create.argtypes = [C.POINTER(Scene), C.c_int, C.POINTER(C.c_void_p)]
    L.zrt_context_create_built.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Material),
                                           C.POINTER(C.c_float), C.c_uint64, C.c_int,
                                           C.POINTER(C.c_void_p)]
    L.zrt_context_grid_info.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.zrt_context_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderConfig),
                                     C.POINTER(Outputs), C.POINTER(Stats)]
    L.zrt_context_profile.argtypes = [C.c_void_p, C.POINTER(KernelProfile)]
    L.zrt_context_trace.argtypes = [C.c_void_p, C.POINTER(RayBatch), C.POINTER(Stats)]
    L.zrt_context_destroy.argtypes = [C.c_void_p]
    L.zrt_context_destroy.restype = None
    L.zrt_context_radiance.argtypes = [C.c_void_p, C.POINTER(RadianceBatch), C.POINTER(Stats)]
    L.zrt_context_segments.argtypes = [C.c_void_p, C.POINTER(SegmentBatch), C.POINTER(Stats)]
    L.zrt_context_surface.argtypes = [C.c_void_p, C.POINTER(SurfaceBatch), C.POINTER(Stats)]
    L.zrt_context_transmittance.argtypes = [C.c_void_p, C.POINTER(TransmittanceBatch), C.POINTER(Stats)]
    L.zrt_context_features.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderConfig),
                                       C.POINTER(FeatureOutputs), C.POINTER(Stats)]
    L.zrt_context_occlusion.argtypes = [C.c_void_p, C.POINTER(OcclusionBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_direct"):   # (a build from before this query: tools/ A/B baselines only)
        L.zrt_context_direct.argtypes = [C.c_void_p, C.POINTER(DirectBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_light_probes"):   # (likewise)
        L.zrt_context_light_probes.argtypes = [C.c_void_p, C.POINTER(LightProbeBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_accumulate"):   # (likewise)
        L.zrt_film_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_void_p)]
        L.zrt_film_reset.argtypes = [C.c_void_p]
        L.zrt_film_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.zrt_film_read.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.zrt_film_write.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.zrt_film_destroy.argtypes = [C.c_void_p]
        L.zrt_film_destroy.restype = None
        L.zrt_context_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.POINTER(RenderConfig),
                                             C.POINTER(Outputs), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_refine"):   # (likewise)
        L.zrt_context_refine.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.POINTER(RenderConfig),
                                         C.POINTER(RefineConfig), C.POINTER(Outputs), C.POINTER(Stats),
                                         C.POINTER(C.c_uint32)]
        L.zrt_film_counts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "zrt_context_denoise"):   # (likewise)
        L.zrt_context_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_reproject"):   # (likewise)
        L.zrt_context_reproject.argtypes = [C.c_void_p, C.POINTER(ReprojectBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_svgf"):   # (likewise)
        L.zrt_context_illumination.argtypes = [C.c_void_p, C.POINTER(IlluminationBatch), C.POINTER(Stats)]
        L.zrt_context_svgf.argtypes = [C.c_void_p, C.POINTER(SvgfBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_area_lights"):   # (likewise)
        L.zrt_emitters_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_void_p)]
        L.zrt_emitters_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint32)]
        L.zrt_emitters_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.zrt_emitters_destroy.argtypes = [C.c_void_p]
        L.zrt_emitters_destroy.restype = None
        L.zrt_context_area_lights.argtypes = [C.c_void_p, C.POINTER(AreaLightBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_context_sky_light"):   # (likewise)
        L.zrt_context_sky_light.argtypes = [C.c_void_p, C.POINTER(SkyLightBatch), C.POINTER(Stats)]
    if hasattr(L, "zrt_group_create"):     # ABI 2 (an ABI-1 build: tools/ A/B baselines only)
        L.zrt_group_create.argtypes = [C.POINTER(Scene), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_void_p)]
        L.zrt_group_create_built.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Material),
                                             C.POINTER(C.c_float), C.c_uint64, C.POINTER(C.c_int32), C.c_uint32,
                                             C.POINTER(C.c_void_p)]
        L.zrt_group_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderConfig), C.c_void_p,
                                       C.POINTER(Stats)]
        L.zrt_group_context.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.zrt_group_destroy.argtypes = [C.c_void_p]
        L.zrt_group_destroy.restype = None
    L.zrt_tile_pixels.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_void_p, C.POINTER(C.c_uint32)]
    L.zrt_camera_from_matrix.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_int32,
                                         C.c_int32, C.POINTER(Camera)]
    L.zrt_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    L.zrt_timed_kernels.restype = C.c_char_p
    L.zrt_timed_kernels.argtypes = []
    if hasattr(L, "zrt_gltf_load"):
        L.zrt_gltf_load.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.zrt_gltf_soup.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 + [
            C.POINTER(C.c_uint32)]
        L.zrt_gltf_materials.argtypes = [C.c_void_p, C.POINTER(Scene)]
        L.zrt_gltf_camera.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32,
                                      C.POINTER(Camera)]
        L.zrt_gltf_free.argtypes = [C.c_void_p]
        L.zrt_gltf_free.restype = None
    _lib = L
    return L


def check(rc, what):
    if rc != ZRT_OK:
        raise ZrtError(rc, what)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().zrt_device_count(C.byref(n))
    return n.value if rc == ZRT_OK else 0


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def camera_from_matrix(m16, yfov, aspect=None, width=None, height=None) -> Camera:
    """stage1.zig:309-371 loadCamera through the C ABI."""
    cam = Camera()
    m = np.ascontiguousarray(m16, np.float32)
    rc = lib().zrt_camera_from_matrix(m.ctypes.data, float(yfov), 0 if aspect is None else 1,
                                      0.0 if aspect is None else float(aspect),
                                      -1 if width is None else int(width),
                                      -1 if height is None else int(height), C.byref(cam))
    check(rc, "zrt_camera_from_matrix")
    return cam


def tile_pixels(w, h, tile=64, rank=0, num_ranks=1) -> np.ndarray:
    n = C.c_uint32(0)
    check(lib().zrt_tile_pixels(w, h, tile, rank, num_ranks, None, C.byref(n)), "zrt_tile_pixels")
    out = np.zeros(max(n.value, 1), np.uint32)
    check(lib().zrt_tile_pixels(w, h, tile, rank, num_ranks, out.ctypes.data, C.byref(n)),
          "zrt_tile_pixels")
    return out[:n.value]


class Geometry:
    """stage2.Geometry: build (SAT binning) + bake, on host threads, or on
    GPU `device` (zrt_geometry_build_device: same arrays, bit for bit)."""

    def __init__(self, pos, nrm, uv, mat, resolution=(128, 128, 128), num_threads=0, device=None):
        self._keep = [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32),
                      np.ascontiguousarray(uv, np.float32), np.ascontiguousarray(mat, np.uint32)]
        n = self._keep[3].size
        res = (C.c_uint32 * 3)(*resolution)
        h = C.c_void_p()
        args = [k.ctypes.data for k in self._keep] + [n, res]
        if device is None:
            check(lib().zrt_geometry_build(*args, num_threads, C.byref(h)), "zrt_geometry_build")
        else:
            check(lib().zrt_geometry_build_device(*args, int(device), C.byref(h)),
                  "zrt_geometry_build_device")
        self._h = h
        self.scene = Scene()
        check(lib().zrt_geometry_scene(self._h, C.byref(self.scene)), "zrt_geometry_scene")

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.zrt_geometry_free(self._h)
            self._h = None

    @property
    def num_refs(self):
        return int(self.scene.num_triangles)

    def indices(self):
        p = C.POINTER(C.c_uint32)()
        n = C.c_uint32(0)
        check(lib().zrt_geometry_indices(self._h, C.byref(p), C.byref(n)), "zrt_geometry_indices")
        return np.ctypeslib.as_array(p, (n.value,)).copy() if n.value else np.zeros(0, np.uint32)

    def cells(self):
        n = self.scene.num_cells
        return np.ctypeslib.as_array(self.scene.cells, (n, 2)).copy()

    def tri_pos(self):
        return np.ctypeslib.as_array(self.scene.triangles_pos, (self.num_refs, 9)).copy()

    def tri_data(self):
        return np.ctypeslib.as_array(self.scene.triangles_data, (self.num_refs, 15)).copy()

    def tri_material(self):
        return np.ctypeslib.as_array(self.scene.triangles_material, (self.num_refs,)).copy()


def attach_materials(scene: Scene, tex_desc: np.ndarray, texels: np.ndarray, keep: list):
    """Fill the material fields of a zrt_scene from (nmat,3,7) descriptors."""
    td = np.asarray(tex_desc, np.int64).reshape(-1, 3, 7)
    mats = (Material * len(td))()
    for i, m in enumerate(td):
        for k, name in enumerate(("base_color", "emissive", "transparency")):
            t = getattr(mats[i], name)
            t.offset, t.w, t.h, t.u_min, t.u_max, t.v_min, t.v_max = (int(x) for x in m[k])
    tx = np.ascontiguousarray(texels, np.float32)
    keep += [mats, tx]
    scene.num_materials = len(td)
    scene.materials = C.cast(mats, C.POINTER(Material))
    scene.texels = _ptr(tx, C.c_float)
    scene.num_texel_floats = tx.size


class Film:
    """zrt_film: the per-pixel sample sums of one rank's share of a w x h
    frame, kept between Context.accumulate calls (progressive renders,
    checkpoint and resume).  Close it before its context."""

    def __init__(self, context: "Context", w: int, h: int, tile: int = 64, rank: int = 0, num_ranks: int = 1):
        h_ = C.c_void_p()
        check(lib().zrt_film_create(context._h, w, h, tile, rank, num_ranks, C.byref(h_)), "zrt_film_create")
        self._h = h_
        self._context = context          # (keeps the context alive as long as the film)
        self.w, self.h, self.tile, self.rank, self.num_ranks = w, h, tile or 64, rank, num_ranks or 1
        self.n_owned = self.info()[0]

    def info(self):
        """(pixels owned, samples summed so far)."""
        n, s = C.c_uint32(0), C.c_uint32(0)
        check(lib().zrt_film_info(self._h, C.byref(n), C.byref(s)), "zrt_film_info")
        return int(n.value), int(s.value)

    @property
    def samples(self) -> int:
        return self.info()[1]

    def counts(self):
        """(samples each owned pixel holds (n_owned,) uint32, pixels not frozen):
        zrt_film_counts.  They differ between pixels after Context.refine."""
        n = np.zeros(self.n_owned, np.uint32)
        a = C.c_uint32(0)
        check(lib().zrt_film_counts(self._h, n.ctypes.data, C.byref(a)), "zrt_film_counts")
        return n, int(a.value)

    def reset(self):
        check(lib().zrt_film_reset(self._h), "zrt_film_reset")

    def read(self):
        """(sums (n_owned, 3) float32 as stored -- no division --, samples): a checkpoint."""
        sums = np.zeros((self.n_owned, 3), np.float32)
        s = C.c_uint32(0)
        check(lib().zrt_film_read(self._h, sums.ctypes.data, C.byref(s)), "zrt_film_read")
        return sums, int(s.value)

    def write(self, sums, samples: int):
        """Resume from a checkpoint: the sums of `samples` samples (0: a reset)."""
        a = np.ascontiguousarray(sums, np.float32)
        if a.size != 3 * self.n_owned:
            raise ValueError(f"zrt_film_write: {self.n_owned} x 3 sums expected")
        check(lib().zrt_film_write(self._h, a.ctypes.data, int(samples)), "zrt_film_write")

    def denoise(self, **kw):
        """Context.denoise(w, h, film=self, tile=self.tile, ...) of the film's
        context: the frame the film shows, filtered (a film of rank 0 of 1)."""
        return self._context.denoise(self.w, self.h, film=self, tile=self.tile, **kw)

    def reproject(self, camera, prev_camera, **kw):
        """Context.reproject(camera, prev_camera, film=self, tile=self.tile, ...)
        of the film's context: the frame the film shows, blended with the
        previous frame's history (a film of rank 0 of 1)."""
        return self._context.reproject(camera, prev_camera, film=self, tile=self.tile, **kw)

    def illumination(self, albedo=None, **kw):
        """Context.illumination(w, h, film=self, albedo=albedo, tile=self.tile,
        ...) of the film's frame so far (rank 0 of 1)."""
        return self._context.illumination(self.w, self.h, film=self, albedo=albedo, tile=self.tile, **kw)

    def close(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.zrt_film_destroy(self._h)       # (frees its device memory; does not touch the context)
            self._h = None

    def __del__(self):
        self.close()


class Emitters:
    """zrt_emitters: the emissive triangles of a source soup as a sampling
    distribution on the context's device, built once (positions (n, 9),
    texcoords (n, 6) or None for zeros, material (n,) indices into the
    context's materials) and read by Context.area_lights.  Close it before its
    context."""

    def __init__(self, context: "Context", positions, texcoords, material):
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1)
        mat = np.ascontiguousarray(material, np.uint32).reshape(-1)
        uv = None if texcoords is None else np.ascontiguousarray(texcoords, np.float32).reshape(-1)
        n = mat.size
        if pos.size != 9 * n or (uv is not None and uv.size != 6 * n):
            raise ValueError("Emitters: (n, 9) positions, (n, 6) texcoords or None and (n,) materials expected")
        h_ = C.c_void_p()
        check(lib().zrt_emitters_create(context._h, pos.ctypes.data if n else None,
                                        uv.ctypes.data if uv is not None and n else None,
                                        mat.ctypes.data if n else C.cast(C.pointer(C.c_uint32(0)), C.c_void_p),
                                        n, C.byref(h_)), "zrt_emitters_create")
        self._h = h_
        self._context = context          # (keeps the context alive as long as the set)

    def info(self):
        """(emitters, Q: the total of their integer weights, source triangles)."""
        n, q, t = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        check(lib().zrt_emitters_info(self._h, C.byref(n), C.byref(q), C.byref(t)), "zrt_emitters_info")
        return int(n.value), int(q.value), int(t.value)

    @property
    def count(self) -> int:
        return self.info()[0]

    def read(self):
        """(records: (count,) EMITTER_DTYPE, C: (count,) uint64 exclusive prefix sums of q)."""
        n = self.count
        rec, pre = np.zeros(n, EMITTER_DTYPE), np.zeros(n, np.uint64)
        check(lib().zrt_emitters_read(self._h, rec.ctypes.data if n else None, pre.ctypes.data if n else None),
              "zrt_emitters_read")
        return rec, pre

    def close(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.zrt_emitters_destroy(self._h)   # (frees its device memory; does not touch the context)
            self._h = None

    def __del__(self):
        self.close()


class Context:
    """Device-resident scene (zrt_context): upload once, render many times."""

    def __init__(self, scene: Scene, device: int = -1):
        h = C.c_void_p()
        check(lib().zrt_context_create(C.byref(scene), device, C.byref(h)), "zrt_context_create")
        self._h = h

    @classmethod
    def built(cls, pos, nrm, uv, mat, materials: Scene, resolution=(128, 128, 128), device: int = -1):
        """zrt_context_create_built: grid built on the GPU straight into the
        context (materials/texels taken from `materials`' material fields)."""
        keep = [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32),
                np.ascontiguousarray(uv, np.float32), np.ascontiguousarray(mat, np.uint32)]
        res = (C.c_uint32 * 3)(*resolution)
        h = C.c_void_p()
        check(lib().zrt_context_create_built(*[k.ctypes.data for k in keep], keep[3].size, res,
                                             materials.num_materials, materials.materials,
                                             materials.texels, materials.num_texel_floats, device,
                                             C.byref(h)), "zrt_context_create_built")
        self = cls.__new__(cls)
        self._h = h
        return self

    def grid_info(self):
        """(num_refs, empty cells, min refs of a non-empty cell, max refs)."""
        info = (C.c_uint32 * 4)()
        check(lib().zrt_context_grid_info(self._h, None, info), "zrt_context_grid_info")
        return tuple(int(x) for x in info)

    def profile(self):
        """zrt_context_profile: per-kernel launches (and device ms with
        FLAG_KERNEL_TIMES) of the last render, primary-segment counts of a
        counting render."""
        kp = KernelProfile()
        check(lib().zrt_context_profile(self._h, C.byref(kp)), "zrt_context_profile")
        return kp.as_dict()

    def close(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.zrt_context_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def render(self, cam: Camera, spp: int, max_bounce: int, seed: int = 0, rank: int = 0,
               num_ranks: int = 1, tile: int = 64, stats: bool = False, image=None,
               packed=False, linear=False, device_ptr=None, samples_per_pass=0, flags=0):
        cfg = RenderConfig()
        cfg.num_samples, cfg.max_bounce, cfg.seed = spp, max_bounce, seed
        cfg.device, cfg.rank, cfg.num_ranks, cfg.tile_size = -1, rank, num_ranks, tile
        cfg.flags = (FLAG_COUNT_STATS if stats else 0) | flags
        cfg.samples_per_pass = samples_per_pass
        n = None
        out = Outputs()
        res = {}
        if image is not None:
            out.rgb_image = image.ctypes.data
        if packed or linear:
            n = int(tile_pixels(cam.w, cam.h, tile, rank, num_ranks).size)
        if packed:
            res["packed"] = np.zeros((n, 3), np.uint8)
            out.rgb_packed = res["packed"].ctypes.data
        if linear:
            res["linear"] = np.zeros((n, 3), np.float32)
            out.linear_packed = res["linear"].ctypes.data
        if device_ptr is not None:
            out.device_rgb_packed = device_ptr
        st = Stats()
        check(lib().zrt_context_render(self._h, C.byref(cam), C.byref(cfg), C.byref(out),
                                       C.byref(st)), "zrt_context_render")
        res["stats"] = st.as_dict()
        return res

    def film(self, w: int, h: int, tile: int = 64, rank: int = 0, num_ranks: int = 1) -> "Film":
        """A Film of this context for this rank's share of a w x h frame."""
        return Film(self, w, h, tile, rank, num_ranks)

    def accumulate(self, film: "Film", cam: Camera, spp: int, max_bounce: int, seed: int = 0,
                   stats: bool = False, image=None, packed=False, linear=False, device_ptr=None,
                   samples_per_pass=0, flags=0, want_linear=None):
        """zrt_context_accumulate: the next `spp` samples of every pixel of
        `film` (samples film.samples .. film.samples + spp - 1 of the stream a
        render of the same camera, seed and max_bounce draws), added to its
        sums in sample order.  The outputs asked for, as in render (image,
        packed, linear -- want_linear is its other name -- and device_ptr), show
        the frame so far: after any split of N samples over calls they are, bit
        for bit, one render's of N.  rank, num_ranks and tile are the film's.
        With no output asked the call only accumulates."""
        cfg = RenderConfig()
        cfg.num_samples, cfg.max_bounce, cfg.seed = spp, max_bounce, seed
        cfg.device, cfg.rank, cfg.num_ranks, cfg.tile_size = -1, film.rank, film.num_ranks, film.tile
        cfg.flags = (FLAG_COUNT_STATS if stats else 0) | flags
        cfg.samples_per_pass = samples_per_pass
        if want_linear is not None:
            linear = want_linear
        out = Outputs()
        res = {}
        if image is not None:
            out.rgb_image = image.ctypes.data
        if packed:
            res["packed"] = np.zeros((film.n_owned, 3), np.uint8)
            out.rgb_packed = res["packed"].ctypes.data
        if linear:
            res["linear"] = np.zeros((film.n_owned, 3), np.float32)
            out.linear_packed = res["linear"].ctypes.data
        if device_ptr is not None:
            out.device_rgb_packed = device_ptr
        asked = image is not None or packed or linear or device_ptr is not None
        st = Stats()
        check(lib().zrt_context_accumulate(self._h, film._h, C.byref(cam), C.byref(cfg),
                                           C.byref(out) if asked else None, C.byref(st)), "zrt_context_accumulate")
        res["stats"] = st.as_dict()
        res["samples"] = film.samples
        return res

    def refine(self, film: "Film", cam: Camera, spp: int, max_bounce: int, threshold: float, min_samples: int = 0,
               seed: int = 0, stats: bool = False, image=None, packed=False, linear=False, device_ptr=None,
               samples_per_pass=0, flags=0, want_linear=None, counts=False):
        """zrt_context_refine: accumulate for the pixels of `film` that have not
        converged.  A pixel whose image changed by no more than `threshold`
        (relative, see include/zrt.h) since the previous refine call is frozen
        at the samples it holds, once the film holds `min_samples`; the others
        get the next `spp` samples.  The outputs show every pixel at its own
        count -- bit for bit a render's pixel of that many samples.
        res["active"]: pixels traced; res["counts"] (with counts=True): samples
        per owned pixel; res["stats"]: of the traced paths only."""
        cfg = RenderConfig()
        cfg.num_samples, cfg.max_bounce, cfg.seed = spp, max_bounce, seed
        cfg.device, cfg.rank, cfg.num_ranks, cfg.tile_size = -1, film.rank, film.num_ranks, film.tile
        cfg.flags = (FLAG_COUNT_STATS if stats else 0) | flags
        cfg.samples_per_pass = samples_per_pass
        if want_linear is not None:
            linear = want_linear
        rf = RefineConfig()
        rf.threshold, rf.min_samples = threshold, min_samples
        out = Outputs()
        res = {}
        if counts:
            res["counts"] = np.zeros(film.n_owned, np.uint32)
            rf.sample_counts = res["counts"].ctypes.data
        if image is not None:
            out.rgb_image = image.ctypes.data
        if packed:
            res["packed"] = np.zeros((film.n_owned, 3), np.uint8)
            out.rgb_packed = res["packed"].ctypes.data
        if linear:
            res["linear"] = np.zeros((film.n_owned, 3), np.float32)
            out.linear_packed = res["linear"].ctypes.data
        if device_ptr is not None:
            out.device_rgb_packed = device_ptr
        asked = image is not None or packed or linear or device_ptr is not None
        st = Stats()
        act = C.c_uint32(0)
        check(lib().zrt_context_refine(self._h, film._h, C.byref(cam), C.byref(cfg), C.byref(rf),
                                       C.byref(out) if asked else None, C.byref(st), C.byref(act)),
              "zrt_context_refine")
        res["stats"] = st.as_dict()
        res["samples"] = film.samples
        res["active"] = int(act.value)
        return res

    @staticmethod
    def _rays(what, origins, dirs):
        """The input checks of a query call `what` and its rays as one (n, 6)
        array: (torch or None, n, rays) -- torch for two CUDA tensors, whose
        rays are a CUDA tensor, None for anything numpy takes."""
        if type(origins).__module__.split(".")[0] == "torch":
            import torch
            if not (origins.is_cuda and dirs.is_cuda and origins.device == dirs.device):
                raise ValueError(f"{what}: torch inputs must be CUDA tensors on the context's device")
            if origins.dtype != torch.float32 or dirs.dtype != torch.float32:
                raise ValueError(f"{what}: float32 tensors expected")
            if origins.dim() != 2 or origins.shape[1] != 3 or origins.shape != dirs.shape:
                raise ValueError(f"{what}: two (n, 3) tensors expected")
            return torch, int(origins.shape[0]), torch.cat([origins, dirs], dim=1).contiguous()
        o = np.asarray(origins, np.float32)
        d = np.asarray(dirs, np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError(f"{what}: two (n, 3) arrays expected")
        return None, o.shape[0], np.ascontiguousarray(np.concatenate([o, d], axis=1))

    def trace_raw(self, num_rays: int, rays_ptr, hits_ptr, on_device: bool, flags: int = 0):
        """zrt_context_trace on raw pointers; returns the stats dict."""
        batch = RayBatch(int(num_rays), rays_ptr, hits_ptr, 1 if on_device else 0, int(flags))
        st = Stats()
        check(lib().zrt_context_trace(self._h, C.byref(batch), C.byref(st)), "zrt_context_trace")
        return st.as_dict()

    def trace(self, origins, dirs, flags: int = 0, stats: bool = False):
        """Scene.traceRay (stage3.zig:152-186) for n rays: where each one first
        hits the context's scene.  `dirs` need not be unit length.

        Two (n, 3) float32 numpy arrays give {"t", "u", "v", "triangle"} as
        (n,) numpy arrays -- a miss is (+inf, 0, 0, MISS); "triangle" is the
        baked ref -- and "stats" (the work counters filled with stats=True).

        Two (n, 3) float32 CUDA tensors (torch-ROCm) on the context's device
        are traced in place, after a sync of torch's current stream; the
        result is {"hits": an (n, 4) float32 CUDA tensor of (t, u, v, ref bit
        pattern), "stats"}; `hits[:, 3].view(torch.int32)` is the ref (-1: a
        miss).  The call returns with the tensor complete."""
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0)
        torch, n, rays = self._rays("trace", origins, dirs)
        if torch:
            hits = torch.empty((n, 4), dtype=torch.float32, device=origins.device)
            torch.cuda.current_stream(origins.device).synchronize()
            st = self.trace_raw(n, rays.data_ptr() if n else None, hits.data_ptr() if n else None, True, flags)
            return {"hits": hits, "stats": st}
        hits = np.empty(n, HIT_DTYPE)
        st = self.trace_raw(n, rays.ctypes.data if n else None, hits.ctypes.data if n else None, False, flags)
        return {"t": hits["t"].copy(), "u": hits["u"].copy(), "v": hits["v"].copy(),
                "triangle": hits["triangle"].copy(), "stats": st}

    def segments_raw(self, num_rays: int, rays_ptr, t_max_ptr, hits_ptr, occluded_ptr, on_device: bool,
                     flags: int = 0, t_max_all: float = float("inf"), reserved: int = 0):
        """zrt_context_segments on raw pointers; returns the stats dict."""
        batch = SegmentBatch(int(num_rays), rays_ptr, t_max_ptr, hits_ptr, occluded_ptr, 1 if on_device else 0,
                             int(flags), float(t_max_all), int(reserved))
        st = Stats()
        check(lib().zrt_context_segments(self._h, C.byref(batch), C.byref(st)), "zrt_context_segments")
        return st.as_dict()

    def segments(self, origins, dirs, t_max, any_hit: bool = False, flags: int = 0, stats: bool = False):
        """Scene.traceRay for n rays with an end (zrt_context_segments): ray i
        is traced with its nearest hit starting at t_max[i] -- `t_max` a
        scalar for every ray or n values, in the ray's own parameter (`dirs`
        need not be unit length; unit directions take the fast kernels).  A
        ref at exactly t_max is not a hit; t_max <= 0 or NaN is a miss.

        Two (n, 3) float32 numpy arrays give {"t", "u", "v", "triangle"} as in
        trace() (a miss is (+inf, 0, 0, MISS)), "occluded", an (n,) bool
        array, and "stats".  With any_hit=True only "occluded" and "stats"
        come back, the walk of a ray ending at its first hit; "stats" then
        holds "hits" in every call.

        Two (n, 3) float32 CUDA tensors (torch-ROCm) on the context's device
        (and `t_max` a float or an (n,) float32 tensor there) are traced in
        place, after a sync of torch's current stream: {"hits": an (n, 4)
        float32 CUDA tensor as in trace() (not with any_hit), "occluded": an
        (n,) torch.bool CUDA tensor, "stats"}."""
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0) | (SEGMENT_ANY if any_hit else 0)
        torch, n, rays = self._rays("segments", origins, dirs)
        if torch:
            tm, tm_all = None, float("inf")
            if torch.is_tensor(t_max) and t_max.dim() > 0:
                if t_max.device != origins.device or t_max.dtype != torch.float32 or t_max.shape != (n,):
                    raise ValueError("segments: t_max must be a float or an (n,) float32 tensor on the rays' device")
                tm = t_max.contiguous()
            else:
                tm_all = float(t_max)
            hits = None if any_hit else torch.empty((n, 4), dtype=torch.float32, device=origins.device)
            occ = torch.empty((n,), dtype=torch.bool, device=origins.device)     # one byte per ray, 0 / 1
            torch.cuda.current_stream(origins.device).synchronize()
            st = self.segments_raw(n, rays.data_ptr() if n else None, tm.data_ptr() if tm is not None and n else None,
                                   hits.data_ptr() if hits is not None and n else None,
                                   occ.data_ptr() if n else None, True, flags, tm_all)
            res = {"occluded": occ, "stats": st}
            if hits is not None:
                res["hits"] = hits
            return res
        tm, tm_all = None, float("inf")
        if np.ndim(t_max) == 0:
            tm_all = float(t_max)
        else:
            tm = np.ascontiguousarray(t_max, np.float32)
            if tm.shape != (n,):
                raise ValueError("segments: t_max must be a scalar or n values")
        hits = None if any_hit else np.empty(n, HIT_DTYPE)
        occ = np.zeros(n, np.uint8)
        st = self.segments_raw(n, rays.ctypes.data if n else None, tm.ctypes.data if tm is not None and n else None,
                               hits.ctypes.data if hits is not None and n else None,
                               occ.ctypes.data if n else None, False, flags, tm_all)
        res = {"occluded": occ.view(np.bool_), "stats": st}
        if hits is not None:
            res.update(t=hits["t"].copy(), u=hits["u"].copy(), v=hits["v"].copy(), triangle=hits["triangle"].copy())
        return res

    def surface_raw(self, num_rays: int, rays_ptr, surfaces_ptr, hits_ptr, on_device: bool, flags: int = 0):
        """zrt_context_surface on raw pointers; returns the stats dict."""
        batch = SurfaceBatch(int(num_rays), rays_ptr, surfaces_ptr, hits_ptr, 1 if on_device else 0, int(flags))
        st = Stats()
        check(lib().zrt_context_surface(self._h, C.byref(batch), C.byref(st)), "zrt_context_surface")
        return st.as_dict()

    def surface(self, origins, dirs, flags: int = 0, stats: bool = False, hits: bool = False):
        """What is at each ray's first hit (zrt_context_surface): the inputs
        traceRayRecursive shades with (stage3.zig:199-206) and the origin it
        continues from.  `dirs` need not be unit length; the rays are traced as
        trace() traces them.

        Two (n, 3) float32 numpy arrays give one array per field of
        zrt_surface -- "position", "normal", "base_color", "emissive" (n, 3)
        float32; "transparency", "texcoord_s", "texcoord_t" (n,) float32;
        "material" (n,) uint32 -- and "stats".  A miss is all zeros with
        material = MISS.  The normal is not normalised.  With hits=True also
        trace()'s "t", "u", "v", "triangle".

        Two (n, 3) float32 CUDA tensors (torch-ROCm) on the context's device
        are traced in place, after a sync of torch's current stream:
        {"surfaces": an (n, 16) float32 CUDA tensor of the records' words
        (`[:, 3].view(torch.int32)` is the material, -1: a miss), "stats"}, and
        with hits=True "hits" as in trace()."""
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0)
        torch, n, rays = self._rays("surface", origins, dirs)
        if torch:
            surf = torch.empty((n, 16), dtype=torch.float32, device=origins.device)
            rec = torch.empty((n, 4), dtype=torch.float32, device=origins.device) if hits else None
            torch.cuda.current_stream(origins.device).synchronize()
            st = self.surface_raw(n, rays.data_ptr() if n else None, surf.data_ptr() if n else None,
                                  rec.data_ptr() if hits and n else None, True, flags)
            res = {"surfaces": surf, "stats": st}
            if hits:
                res["hits"] = rec
            return res
        surf = np.empty(n, SURFACE_DTYPE)
        rec = np.empty(n, HIT_DTYPE) if hits else None
        st = self.surface_raw(n, rays.ctypes.data if n else None, surf.ctypes.data if n else None,
                              rec.ctypes.data if hits and n else None, False, flags)
        res = {k: surf[k].copy() for k in SURFACE_DTYPE.names}
        if hits:
            res.update(t=rec["t"].copy(), u=rec["u"].copy(), v=rec["v"].copy(), triangle=rec["triangle"].copy())
        res["stats"] = st
        return res

    def transmittance_raw(self, num_rays: int, rays_ptr, t_max_ptr, transmittance_ptr, crossings_ptr, on_device: bool,
                          flags: int = 0, t_max_all: float = float("inf"), max_crossings: int = 16):
        """zrt_context_transmittance on raw pointers; returns the stats dict."""
        batch = TransmittanceBatch(int(num_rays), rays_ptr, t_max_ptr, transmittance_ptr, crossings_ptr,
                                   1 if on_device else 0, int(flags), float(t_max_all), int(max_crossings))
        st = Stats()
        check(lib().zrt_context_transmittance(self._h, C.byref(batch), C.byref(st)), "zrt_context_transmittance")
        return st.as_dict()

    def transmittance(self, origins, dirs, t_max=float("inf"), max_crossings: int = 16, flags: int = 0,
                      stats: bool = False, crossings: bool = False):
        """Shadow rays that pass through transparent hits as the path tracer
        does (zrt_context_transmittance): per ray the product of 1 - alpha over
        the surfaces met before t_max -- `t_max` a scalar for every ray or n
        values, in the ray's own parameter -- 0 from the first opaque one on, 1
        if there is none; at most `max_crossings` (1..256) surfaces per ray.

        Two (n, 3) float32 numpy arrays give {"transmittance": (n,) float32,
        "stats"} and with crossings=True "crossings", (n,) uint32: the surfaces
        each ray met (== max_crossings: the chain was cut there).  "stats"
        holds "segments" and "hits" (the sum of the crossings) in every call,
        the cell and test counters with stats=True.

        Two (n, 3) float32 CUDA tensors (torch-ROCm) on the context's device
        (and `t_max` a float or an (n,) float32 tensor there) are traced in
        place, after a sync of torch's current stream: "transmittance" an (n,)
        float32 and "crossings" an (n,) int32 CUDA tensor."""
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0)
        torch, n, rays = self._rays("transmittance", origins, dirs)
        if torch:
            tm, tm_all = None, float("inf")
            if torch.is_tensor(t_max) and t_max.dim() > 0:
                if t_max.device != origins.device or t_max.dtype != torch.float32 or t_max.shape != (n,):
                    raise ValueError("transmittance: t_max must be a float or an (n,) float32 tensor on the rays' device")
                tm = t_max.contiguous()
            else:
                tm_all = float(t_max)
            T = torch.empty((n,), dtype=torch.float32, device=origins.device)
            cr = torch.empty((n,), dtype=torch.int32, device=origins.device) if crossings else None
            torch.cuda.current_stream(origins.device).synchronize()
            st = self.transmittance_raw(n, rays.data_ptr() if n else None,
                                        tm.data_ptr() if tm is not None and n else None, T.data_ptr() if n else None,
                                        cr.data_ptr() if crossings and n else None, True, flags, tm_all, max_crossings)
            res = {"transmittance": T, "stats": st}
            if crossings:
                res["crossings"] = cr
            return res
        tm, tm_all = None, float("inf")
        if np.ndim(t_max) == 0:
            tm_all = float(t_max)
        else:
            tm = np.ascontiguousarray(t_max, np.float32)
            if tm.shape != (n,):
                raise ValueError("transmittance: t_max must be a scalar or n values")
        T = np.empty(n, np.float32)
        cr = np.empty(n, np.uint32) if crossings else None
        st = self.transmittance_raw(n, rays.ctypes.data if n else None, tm.ctypes.data if tm is not None and n else None,
                                    T.ctypes.data if n else None, cr.ctypes.data if crossings and n else None, False,
                                    flags, tm_all, max_crossings)
        res = {"transmittance": T, "stats": st}
        if crossings:
            res["crossings"] = cr
        return res

    def features_raw(self, cam: Camera, spp: int, pointers: dict, on_device: bool, seed: int = 0, rank: int = 0,
                     num_ranks: int = 1, tile_size: int = 0, flags: int = 0, samples_per_pass: int = 0,
                     reserved: int = 0):
        """zrt_context_features on raw pointers: `pointers` maps the names of
        FEATURE_PLANES to addresses (absent or None: not asked for); returns
        the stats dict."""
        cfg = RenderConfig()
        cfg.num_samples, cfg.seed, cfg.device = int(spp), int(seed), -1
        cfg.rank, cfg.num_ranks, cfg.tile_size = int(rank), int(num_ranks), int(tile_size)
        cfg.flags, cfg.samples_per_pass = int(flags), int(samples_per_pass)
        out = FeatureOutputs(*[pointers.get(name) for name, _ in FEATURE_PLANES], 1 if on_device else 0, int(reserved))
        st = Stats()
        check(lib().zrt_context_features(self._h, C.byref(cam), C.byref(cfg), C.byref(out), C.byref(st)),
              "zrt_context_features")
        return st.as_dict()

    def features(self, cam: Camera, spp: int, seed: int = 0, rank: int = 0, num_ranks: int = 1, tile_size: int = 0,
                 flags: int = 0, samples_per_pass: int = 0, planes=None, stats: bool = False):
        """The auxiliary planes of the frame a render(cam, spp, ..., seed)
        gives (zrt_context_features): per pixel the base colour, interpolated
        normal (not normalised), emission, distance and transparency of the
        first hit, averaged over the render's own `spp` jittered camera
        samples -- a miss adds nothing -- and the number of samples that hit.

        `planes`: the names wanted, of "base_color", "normal", "emissive"
        ((n, 3) float32), "depth", "transparency" ((n,) float32), "hits"
        ((n,) uint32); None: all six.  The arrays are packed in
        tile_pixels(w, h, tile_size or 64, rank, num_ranks) order, n that
        call's count.  With num_ranks == 1 the result also holds "images":
        the same planes scattered into (h, w, C) arrays, C = 3 or 1.  "stats" is filled in
        every call (segments, samples, hits), the cell and test counters with
        stats=True."""
        names = [n for n, _ in FEATURE_PLANES] if planes is None else list(planes)
        width = dict(FEATURE_PLANES)
        if not names or any(n not in width for n in names):
            raise ValueError(f"features: planes must name some of {[n for n, _ in FEATURE_PLANES]}")
        pix = tile_pixels(cam.w, cam.h, tile_size or 64, rank, num_ranks)
        n = int(pix.size)
        res = {k: np.zeros((n, 3) if width[k] == 3 else (n,), np.uint32 if k == "hits" else np.float32)
               for k in names}
        st = self.features_raw(cam, spp, {k: v.ctypes.data for k, v in res.items()}, False, seed, rank, num_ranks,
                               tile_size, int(flags) | (FLAG_COUNT_STATS if stats else 0), samples_per_pass)
        if num_ranks == 1:
            images = {}
            for k in names:
                img = np.zeros((cam.h * cam.w, width[k]), res[k].dtype)
                img[pix] = res[k].reshape(n, width[k])
                images[k] = img.reshape(cam.h, cam.w, width[k])
            res["images"] = images
        res["stats"] = st
        return res

    def denoise_raw(self, w: int, h: int, color_ptr, film, normal_ptr, depth_ptr, albedo_ptr, linear_ptr, rgb_ptr,
                    on_device: bool, iterations: int, sigma_color: float, sigma_normal: float = 0.0,
                    sigma_depth: float = 0.0, sigma_albedo: float = 0.0, tile_size: int = 0, flags: int = 0,
                    reserved: int = 0):
        """zrt_context_denoise on raw pointers (`film`: a Film or None); returns
        the stats dict."""
        batch = DenoiseBatch(int(w), int(h), int(tile_size), int(iterations), sigma_color, sigma_normal, sigma_depth,
                             sigma_albedo, color_ptr, film._h if film is not None else None, normal_ptr, depth_ptr,
                             albedo_ptr, linear_ptr, rgb_ptr, 1 if on_device else 0, int(flags), int(reserved))
        st = Stats()
        check(lib().zrt_context_denoise(self._h, C.byref(batch), C.byref(st)), "zrt_context_denoise")
        return st.as_dict()

    def denoise(self, w: int, h: int, color=None, film=None, normal=None, depth=None, albedo=None,
                iterations: int = 5, sigma_color: float = DENOISE_SIGMAS[0], sigma_normal: float = DENOISE_SIGMAS[1],
                sigma_depth: float = DENOISE_SIGMAS[2], sigma_albedo: float = DENOISE_SIGMAS[3], tile: int = 64,
                row_major: bool = False, linear: bool = True, rgb: bool = False, stats: bool = False):
        """The edge-avoiding a-trous filter over a w x h colour frame
        (zrt_context_denoise): `iterations` levels of a 5x5 B3 kernel with
        holes, each tap weighted by how far its colour and its guides -- the
        planes Context.features gives: `normal`, `depth`, `albedo` (its
        "base_color"); each may be None -- are from the centre pixel's.

        The colour is `color`, (P, 3) float32 with P = w * h, or `film`, a Film
        of this context of rank 0 of 1, whose frame so far is filtered (every
        pixel at its own sample count).  All planes, in and out, are in
        tile_pixels(w, h, tile) order, as Context.features and the film's
        outputs are; with row_major=True in image order (not with a film).

        numpy arrays give {"linear": (P, 3) float32, "rgb": (P, 3) uint8} --
        those asked for -- in the planes' order, "images": the same as
        (h, w, 3) arrays, and "stats".  CUDA tensors (torch-ROCm) on the
        context's device -- every plane given must be one -- are filtered in
        place after a sync of torch's current stream and give "linear" and
        "rgb" as CUDA tensors, complete when the call returns, and no "images"
        (a film without a guide plane gives numpy arrays).  `stats` is accepted
        for symmetry: the stats are filled in every call."""
        P = int(w) * int(h)
        if (color is None) == (film is None):
            raise ValueError("denoise: exactly one of color and film")
        if not (linear or rgb):
            raise ValueError("denoise: linear or rgb (or both) must be asked for")
        given = {"color": (color, 3), "normal": (normal, 3), "depth": (depth, 1), "albedo": (albedo, 3)}
        planes = {k: v for k, (v, _) in given.items() if v is not None}
        on_torch = [type(v).__module__.split(".")[0] == "torch" for v in planes.values()]
        flags = DENOISE_ROW_MAJOR if row_major else 0
        sig = (float(sigma_color), float(sigma_normal), float(sigma_depth), float(sigma_albedo))
        res = {}
        if planes and all(on_torch):
            import torch
            dev = next(iter(planes.values())).device
            for k, v in planes.items():
                if not v.is_cuda or v.device != dev or v.dtype != torch.float32 or v.numel() != P * given[k][1]:
                    raise ValueError(f"denoise: {k}: a float32 CUDA tensor of {P} x {given[k][1]} on one device expected")
            planes = {k: v.contiguous() for k, v in planes.items()}
            if linear:
                res["linear"] = torch.empty((P, 3), dtype=torch.float32, device=dev)
            if rgb:
                res["rgb"] = torch.empty((P, 3), dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ptr = {k: v.data_ptr() for k, v in planes.items()}
            out = {k: v.data_ptr() for k, v in res.items()}
            on_device = True
        elif any(on_torch):
            raise ValueError("denoise: the planes must be all numpy arrays or all CUDA tensors")
        else:
            for k in planes:
                planes[k] = np.ascontiguousarray(planes[k], np.float32)
                if planes[k].size != P * given[k][1]:
                    raise ValueError(f"denoise: {k}: {P} x {given[k][1]} floats expected")
            if linear:
                res["linear"] = np.zeros((P, 3), np.float32)
            if rgb:
                res["rgb"] = np.zeros((P, 3), np.uint8)
            ptr = {k: v.ctypes.data for k, v in planes.items()}
            out = {k: v.ctypes.data for k, v in res.items()}
            on_device = False
        st = self.denoise_raw(w, h, ptr.get("color"), film, ptr.get("normal"), ptr.get("depth"), ptr.get("albedo"),
                              out.get("linear"), out.get("rgb"), on_device, iterations, *sig, tile_size=tile,
                              flags=flags)
        if not on_device:
            pix = None if row_major else tile_pixels(w, h, tile or 64)
            images = {}
            for k in list(res):
                img = res[k]
                if pix is not None:
                    img = np.zeros_like(res[k])
                    img[pix] = res[k]
                images[k] = img.reshape(h, w, 3)
            res["images"] = images
        res["stats"] = st
        return res

    def reproject_raw(self, camera: Camera, prev_camera: Camera, color_ptr, film, depth_ptr, normal_ptr, prev_color_ptr,
                      prev_depth_ptr, prev_normal_ptr, prev_length_ptr, color_out_ptr, length_out_ptr, motion_ptr,
                      on_device: bool, max_history: int = REPROJECT_DEFAULTS[0],
                      depth_tolerance: float = REPROJECT_DEFAULTS[1], normal_tolerance: float = REPROJECT_DEFAULTS[2],
                      tile_size: int = 0, flags: int = 0, reserved: int = 0):
        """zrt_context_reproject on raw pointers (`film`: a Film or None);
        returns the stats dict."""
        batch = ReprojectBatch(int(tile_size), int(max_history), depth_tolerance, normal_tolerance,
                               1 if on_device else 0, int(flags), C.addressof(camera), C.addressof(prev_camera),
                               color_ptr, film._h if film is not None else None, depth_ptr, normal_ptr, prev_color_ptr,
                               prev_depth_ptr, prev_normal_ptr, prev_length_ptr, color_out_ptr, length_out_ptr,
                               motion_ptr, int(reserved))
        st = Stats()
        check(lib().zrt_context_reproject(self._h, C.byref(batch), C.byref(st)), "zrt_context_reproject")
        return st.as_dict()

    def reproject(self, camera: Camera, prev_camera: Camera, color=None, film=None, depth=None, normal=None,
                  prev_color=None, prev_depth=None, prev_normal=None, prev_length=None,
                  max_history: int = REPROJECT_DEFAULTS[0], depth_tolerance: float = REPROJECT_DEFAULTS[1],
                  normal_tolerance: float = REPROJECT_DEFAULTS[2], tile: int = 64, row_major: bool = False,
                  motion: bool = False, out=None, length_out=None):
        """The previous frame's history carried to the current camera and
        blended with the current colour (zrt_context_reproject): each pixel's
        world point, from `depth` and `camera`, is projected into
        `prev_camera`; `prev_color` is fetched there with four bilinear taps,
        a tap counting only if `prev_depth` (and `prev_normal` against
        `normal`, when both are given) agrees; the result is
        hist * (1 - 1 / N) + colour / N with N = min(least tap length,
        max_history - 1) + 1, or the colour itself and N = 1 without history.

        The colour is `color`, (P, 3) float32 with P = w * h of the cameras,
        or `film`, a Film of this context of rank 0 of 1.  `depth`,
        `prev_color` and `prev_depth` are required; `prev_length` (P,) uint32
        or None: 1 everywhere.  All planes are in tile_pixels(w, h, tile)
        order, as Context.features and the film's outputs are; with
        row_major=True in image order (not with a film).

        numpy arrays give {"color": (P, 3) float32, "length": (P,) uint32,
        "motion": (P, 2) float32 with motion=True, "stats"}.  CUDA tensors
        (torch-ROCm) on the context's device -- every plane given must be one;
        lengths are int32 tensors holding the uint32 bits -- are read in place
        after a sync of torch's current stream and give CUDA tensors, complete
        when the call returns.  `out` / `length_out`: tensors to write instead
        of new ones; `out` may be `prev_color` or `color`, `length_out` may be
        `prev_length` (the call reads the previous planes before it writes)."""
        w, h = int(camera.w), int(camera.h)
        P = w * h
        if (color is None) == (film is None):
            raise ValueError("reproject: exactly one of color and film")
        given = {"color": (color, 3), "depth": (depth, 1), "normal": (normal, 3), "prev_color": (prev_color, 3),
                 "prev_depth": (prev_depth, 1), "prev_normal": (prev_normal, 3), "prev_length": (prev_length, 1)}
        for k in ("depth", "prev_color", "prev_depth"):
            if given[k][0] is None:
                raise ValueError(f"reproject: {k} is required")
        planes = {k: v for k, (v, _) in given.items() if v is not None}
        on_torch = [type(v).__module__.split(".")[0] == "torch" for v in planes.values()]
        flags = REPROJECT_ROW_MAJOR if row_major else 0
        res = {}
        if all(on_torch):
            import torch
            dev = planes["depth"].device
            for k, v in planes.items():
                want = torch.int32 if k == "prev_length" else torch.float32
                if not v.is_cuda or v.device != dev or v.dtype != want or v.numel() != P * given[k][1]:
                    raise ValueError(f"reproject: {k}: a {want} CUDA tensor of {P} x {given[k][1]} on one device expected")
            planes = {k: (v if v.is_contiguous() else v.contiguous()) for k, v in planes.items()}
            res["color"] = torch.empty((P, 3), dtype=torch.float32, device=dev) if out is None else out
            res["length"] = torch.empty((P,), dtype=torch.int32, device=dev) if length_out is None else length_out
            if motion:
                res["motion"] = torch.empty((P, 2), dtype=torch.float32, device=dev)
            for k, want, n in (("color", torch.float32, 3 * P), ("length", torch.int32, P)):
                v = res[k]
                if not v.is_cuda or v.device != dev or v.dtype != want or v.numel() != n or not v.is_contiguous():
                    raise ValueError(f"reproject: the {k} output: a contiguous {want} CUDA tensor of {n} expected")
            torch.cuda.current_stream(dev).synchronize()
            ptr = {k: v.data_ptr() for k, v in planes.items()}
            outp = {k: v.data_ptr() for k, v in res.items()}
            on_device = True
        elif any(on_torch):
            raise ValueError("reproject: the planes must be all numpy arrays or all CUDA tensors")
        else:
            if out is not None or length_out is not None:
                raise ValueError("reproject: out and length_out are for CUDA tensors")
            for k in planes:
                planes[k] = np.ascontiguousarray(planes[k], np.uint32 if k == "prev_length" else np.float32)
                if planes[k].size != P * given[k][1]:
                    raise ValueError(f"reproject: {k}: {P} x {given[k][1]} values expected")
            res["color"] = np.zeros((P, 3), np.float32)
            res["length"] = np.zeros(P, np.uint32)
            if motion:
                res["motion"] = np.zeros((P, 2), np.float32)
            ptr = {k: v.ctypes.data for k, v in planes.items()}
            outp = {k: v.ctypes.data for k, v in res.items()}
            on_device = False
        res["stats"] = self.reproject_raw(camera, prev_camera, ptr.get("color"), film, ptr["depth"], ptr.get("normal"),
                                          ptr["prev_color"], ptr["prev_depth"], ptr.get("prev_normal"),
                                          ptr.get("prev_length"), outp["color"], outp["length"], outp.get("motion"),
                                          on_device, max_history, float(depth_tolerance), float(normal_tolerance),
                                          tile_size=tile, flags=flags)
        return res

    @staticmethod
    def _planes(what, P, given, ints=()):
        """The planes of a whole-frame call that are not None: (planes, on_device, torch device or None), checked
        to be all float32 (`ints`: int32 tensors / uint32 arrays) numpy arrays or all CUDA tensors of P x channels."""
        planes = {k: v for k, (v, _) in given.items() if v is not None}
        on_torch = [type(v).__module__.split(".")[0] == "torch" for v in planes.values()]
        if planes and all(on_torch):
            import torch
            dev = next(iter(planes.values())).device
            for k, v in planes.items():
                want = torch.int32 if k in ints else torch.float32
                if not v.is_cuda or v.device != dev or v.dtype != want or v.numel() != P * given[k][1]:
                    raise ValueError(f"{what}: {k}: a {want} CUDA tensor of {P} x {given[k][1]} on one device expected")
            return {k: (v if v.is_contiguous() else v.contiguous()) for k, v in planes.items()}, True, dev
        if any(on_torch):
            raise ValueError(f"{what}: the planes must be all numpy arrays or all CUDA tensors")
        for k in planes:
            planes[k] = np.ascontiguousarray(planes[k], np.uint32 if k in ints else np.float32)
            if planes[k].size != P * given[k][1]:
                raise ValueError(f"{what}: {k}: {P} x {given[k][1]} values expected")
        return planes, False, None

    def illumination_raw(self, w: int, h: int, color_ptr, film, albedo_ptr, illumination_ptr, moments_ptr,
                         on_device: bool, tile_size: int = 0, flags: int = 0, reserved: int = 0):
        """zrt_context_illumination on raw pointers (`film`: a Film or None);
        returns the stats dict."""
        batch = IlluminationBatch(int(w), int(h), int(tile_size), color_ptr, film._h if film is not None else None,
                                  albedo_ptr, illumination_ptr, moments_ptr, 1 if on_device else 0, int(flags),
                                  int(reserved))
        st = Stats()
        check(lib().zrt_context_illumination(self._h, C.byref(batch), C.byref(st)), "zrt_context_illumination")
        return st.as_dict()

    def illumination(self, w: int, h: int, color=None, film=None, albedo=None, tile: int = 64, row_major: bool = False,
                     illumination: bool = True, moments: bool = True, out=None, moments_out=None):
        """The colour frame divided by max(albedo, 1/16) per component -- what
        Context.svgf filters, so that texture is not smoothed -- and the moments
        plane (l, l * l, 0) of its luminance l (zrt_context_illumination), which
        goes through Context.reproject as a colour plane.

        The colour is `color`, (P, 3) float32 with P = w * h, or `film`, a Film
        of this context of rank 0 of 1.  `albedo`: Context.features'
        "base_color", or None: the illumination is the colour bit for bit.
        Planes are in tile_pixels(w, h, tile) order; with row_major=True in
        image order (not with a film).

        numpy arrays give {"illumination": (P, 3), "moments": (P, 3) float32}
        -- those asked for -- and "stats".  CUDA tensors (torch-ROCm) on the
        context's device are read in place after a sync of torch's current
        stream and give CUDA tensors, complete when the call returns; `out` /
        `moments_out`: tensors to write instead of new ones (a film without an
        albedo plane gives numpy arrays unless one of them is given)."""
        P = int(w) * int(h)
        if (color is None) == (film is None):
            raise ValueError("illumination: exactly one of color and film")
        given = {"color": (color, 3), "albedo": (albedo, 3), "out": (out, 3), "moments_out": (moments_out, 3)}
        planes, on_device, dev = self._planes("illumination", P, given)
        illumination = illumination or out is not None
        moments = moments or moments_out is not None
        if not (illumination or moments):
            raise ValueError("illumination: illumination or moments (or both) must be asked for")
        res = {}
        if on_device:
            import torch
            if illumination:
                res["illumination"] = planes.get("out", None)
                if res["illumination"] is None:
                    res["illumination"] = torch.empty((P, 3), dtype=torch.float32, device=dev)
            if moments:
                res["moments"] = planes.get("moments_out", None)
                if res["moments"] is None:
                    res["moments"] = torch.empty((P, 3), dtype=torch.float32, device=dev)
            if (out is not None and res["illumination"] is not out) or \
                    (moments_out is not None and res["moments"] is not moments_out):
                raise ValueError("illumination: out and moments_out must be contiguous")
            torch.cuda.current_stream(dev).synchronize()
            ptr = {k: v.data_ptr() for k, v in planes.items()}
            outp = {k: v.data_ptr() for k, v in res.items()}
        else:
            if out is not None or moments_out is not None:
                raise ValueError("illumination: out and moments_out are for CUDA tensors")
            if illumination:
                res["illumination"] = np.zeros((P, 3), np.float32)
            if moments:
                res["moments"] = np.zeros((P, 3), np.float32)
            ptr = {k: v.ctypes.data for k, v in planes.items()}
            outp = {k: v.ctypes.data for k, v in res.items()}
        res["stats"] = self.illumination_raw(w, h, ptr.get("color"), film, ptr.get("albedo"), outp.get("illumination"),
                                             outp.get("moments"), on_device, tile_size=tile,
                                             flags=SVGF_ROW_MAJOR if row_major else 0)
        return res

    def svgf_raw(self, w: int, h: int, color_ptr, moments_ptr, length_ptr, normal_ptr, depth_ptr, albedo_ptr,
                 linear_ptr, rgb_ptr, variance_ptr, on_device: bool, iterations: int,
                 sigma_luminance: float = SVGF_SIGMAS[0], sigma_normal: float = 0.0, sigma_depth: float = 0.0,
                 tile_size: int = 0, flags: int = 0, reserved: int = 0):
        """zrt_context_svgf on raw pointers; returns the stats dict."""
        batch = SvgfBatch(int(w), int(h), int(tile_size), int(iterations), sigma_luminance, sigma_normal, sigma_depth,
                          color_ptr, moments_ptr, length_ptr, normal_ptr, depth_ptr, albedo_ptr, linear_ptr, rgb_ptr,
                          variance_ptr, 1 if on_device else 0, int(flags), int(reserved))
        st = Stats()
        check(lib().zrt_context_svgf(self._h, C.byref(batch), C.byref(st)), "zrt_context_svgf")
        return st.as_dict()

    def svgf(self, w: int, h: int, color=None, moments=None, length=None, normal=None, depth=None, albedo=None,
             iterations: int = 5, sigma_luminance: float = SVGF_SIGMAS[0], sigma_normal: float = SVGF_SIGMAS[1],
             sigma_depth: float = SVGF_SIGMAS[2], tile: int = 64, row_major: bool = False, linear: bool = True,
             rgb: bool = False, variance: bool = False, stats: bool = False):
        """The variance-guided a-trous filter (zrt_context_svgf) over a w x h
        illumination frame `color` (Context.illumination's, normally after
        Context.reproject): each pixel's variance is taken from `moments`
        where its history `length` is 4 or more, from its 7 x 7 neighbourhood
        otherwise; `iterations` levels of the 5x5 B3 kernel with holes follow,
        the luminance weight `sigma_luminance` local standard deviations wide,
        `normal` and `depth` the guides as in Context.denoise, the variance
        filtered along; the result is multiplied by max(albedo, 1/16).

        All planes are in tile_pixels(w, h, tile) order, or in image order
        with row_major=True.  numpy arrays give {"linear": (P, 3) float32,
        "rgb": (P, 3) uint8, "variance": (P,) float32} -- those asked for --
        "images" and "stats" (stats["hits"]: the pixels with a temporal
        variance).  CUDA tensors (torch-ROCm; lengths int32 holding the uint32
        bits) give CUDA tensors and no "images".  `stats` is accepted for
        symmetry: the stats are filled in every call."""
        P = int(w) * int(h)
        if color is None:
            raise ValueError("svgf: color is required")
        if not (linear or rgb):
            raise ValueError("svgf: linear or rgb (or both) must be asked for")
        given = {"color": (color, 3), "moments": (moments, 3), "length": (length, 1), "normal": (normal, 3),
                 "depth": (depth, 1), "albedo": (albedo, 3)}
        planes, on_device, dev = self._planes("svgf", P, given, ints=("length",))
        asked = [(k, n, f) for k, n, f, on in (("linear", 3, "float32", linear), ("rgb", 3, "uint8", rgb),
                                               ("variance", 1, "float32", variance)) if on]
        res = {}
        if on_device:
            import torch
            for k, n, f in asked:
                res[k] = torch.empty((P, n) if n > 1 else (P,), dtype=getattr(torch, f), device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ptr = {k: v.data_ptr() for k, v in planes.items()}
            out = {k: v.data_ptr() for k, v in res.items()}
        else:
            for k, n, f in asked:
                res[k] = np.zeros((P, n) if n > 1 else (P,), getattr(np, f))
            ptr = {k: v.ctypes.data for k, v in planes.items()}
            out = {k: v.ctypes.data for k, v in res.items()}
        st = self.svgf_raw(w, h, ptr["color"], ptr.get("moments"), ptr.get("length"), ptr.get("normal"),
                           ptr.get("depth"), ptr.get("albedo"), out.get("linear"), out.get("rgb"), out.get("variance"),
                           on_device, iterations, float(sigma_luminance), float(sigma_normal), float(sigma_depth),
                           tile_size=tile, flags=SVGF_ROW_MAJOR if row_major else 0)
        if not on_device:
            pix = None if row_major else tile_pixels(w, h, tile or 64)
            images = {}
            for k in list(res):
                img = res[k]
                if pix is not None:
                    img = np.zeros_like(res[k])
                    img[pix] = res[k]
                images[k] = img.reshape((h, w, 3) if img.ndim == 2 else (h, w))
            res["images"] = images
        res["stats"] = st
        return res

    def occlusion_raw(self, num_rays: int, rays_ptr, radius_ptr, visibility_ptr, occluded_ptr, hits_ptr,
                      on_device: bool, spp: int, radius_all: float = float("inf"), seed: int = 0, index_base: int = 0,
                      flags: int = 0):
        """zrt_context_occlusion on raw pointers; returns the stats dict."""
        batch = OcclusionBatch(int(num_rays), rays_ptr, radius_ptr, visibility_ptr, occluded_ptr, hits_ptr,
                               1 if on_device else 0, int(flags), float(radius_all), int(spp),
                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(index_base) & 0xFFFFFFFFFFFFFFFF)
        st = Stats()
        check(lib().zrt_context_occlusion(self._h, C.byref(batch), C.byref(st)), "zrt_context_occlusion")
        return st.as_dict()

    def occlusion(self, origins, dirs, spp: int, radius=float("inf"), seed: int = 0, index_base: int = 0,
                  flags: int = 0, stats: bool = False, hits: bool = False):
        """Hemisphere visibility at each ray's first hit (zrt_context_occlusion):
        `spp` directions normalize(normal + random unit vector) per hit, the
        path tracer's own scatter directions from the stream (seed, index_base +
        ray, sample), each traced as a segment of length `radius` -- a scalar
        for every ray or n values; +inf: open sky -- from the surface.  A miss
        is fully visible.

        Two (n, 3) float32 numpy arrays give {"visibility": (n,) float32 =
        (spp - occluded) / spp, "occluded": (n,) uint32, "stats"}, and with
        hits=True trace()'s "t", "u", "v", "triangle" of the first hits.
        "stats" holds "segments" (rays + traced samples) and "hits" (the sum of
        "occluded") in every call, the cell and test counters with stats=True.

        Two (n, 3) float32 CUDA tensors (torch-ROCm) on the context's device
        (and `radius` a float or an (n,) float32 tensor there) are traced in
        place, after a sync of torch's current stream: "visibility" an (n,)
        float32 and "occluded" an (n,) int32 CUDA tensor, with hits=True "hits"
        as in trace()."""
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0)
        torch, n, rays = self._rays("occlusion", origins, dirs)
        if torch:
            rad, rad_all = None, float("inf")
            if torch.is_tensor(radius) and radius.dim() > 0:
                if radius.device != origins.device or radius.dtype != torch.float32 or radius.shape != (n,):
                    raise ValueError("occlusion: radius must be a float or an (n,) float32 tensor on the rays' device")
                rad = radius.contiguous()
            else:
                rad_all = float(radius)
            vis = torch.empty((n,), dtype=torch.float32, device=origins.device)
            occ = torch.empty((n,), dtype=torch.int32, device=origins.device)
            rec = torch.empty((n, 4), dtype=torch.float32, device=origins.device) if hits else None
            torch.cuda.current_stream(origins.device).synchronize()
            st = self.occlusion_raw(n, rays.data_ptr() if n else None, rad.data_ptr() if rad is not None and n else None,
                                    vis.data_ptr() if n else None, occ.data_ptr() if n else None,
                                    rec.data_ptr() if hits and n else None, True, spp, rad_all, seed, index_base, flags)
            res = {"visibility": vis, "occluded": occ, "stats": st}
            if hits:
                res["hits"] = rec
            return res
        rad, rad_all = None, float("inf")
        if np.ndim(radius) == 0:
            rad_all = float(radius)
        else:
            rad = np.ascontiguousarray(radius, np.float32)
            if rad.shape != (n,):
                raise ValueError("occlusion: radius must be a scalar or n values")
        vis = np.empty(n, np.float32)
        occ = np.empty(n, np.uint32)
        rec = np.empty(n, HIT_DTYPE) if hits else None
        st = self.occlusion_raw(n, rays.ctypes.data if n else None, rad.ctypes.data if rad is not None and n else None,
                                vis.ctypes.data if n else None, occ.ctypes.data if n else None,
                                rec.ctypes.data if hits and n else None, False, spp, rad_all, seed, index_base, flags)
        res = {"visibility": vis, "occluded": occ, "stats": st}
        if hits:
            res.update(t=rec["t"].copy(), u=rec["u"].copy(), v=rec["v"].copy(), triangle=rec["triangle"].copy())
        return res

    def direct_raw(self, num_rays: int, rays_ptr, lights, irradiance_ptr, radiance_ptr, hits_ptr, on_device: bool,
                   max_crossings: int = 16, flags: int = 0):
        """zrt_context_direct on raw pointers; `lights`: a sequence of Light
        (always host memory).  Returns the stats dict."""
        arr = (Light * len(lights))(*lights)
        batch = DirectBatch(int(num_rays), rays_ptr, C.cast(arr, C.c_void_p) if len(lights) else None, irradiance_ptr,
                            radiance_ptr, hits_ptr, 1 if on_device else 0, int(flags), len(lights), int(max_crossings))
        st = Stats()
        check(lib().zrt_context_direct(self._h, C.byref(batch), C.byref(st)), "zrt_context_direct")
        return st.as_dict()

    def direct(self, origins, dirs, lights, max_crossings: int = 16, flags: int = 0, unshadowed: bool = False,
               irradiance: bool = True, radiance: bool = False, hits: bool = False, stats: bool = False):
        """Direct light of punctual lights at each ray's first hit
        (zrt_context_direct): per ray the irradiance E = sum over `lights` (a
        sequence of Light, in order) of colour * falloff * T, T the
        transmittance of the segment to the light through at most
        `max_crossings` transparent hits (unshadowed=True: T = 1, nothing
        traced), and the Lambertian radiance emissive + base_color * E / pi.
        A miss is zero in both.

        Two (n, 3) float32 numpy arrays give {"irradiance": (n, 3) float32,
        "radiance": (n, 3) float32 (each only when asked), "stats"}, and with
        hits=True trace()'s "t", "u", "v", "triangle" of the first hits.
        "stats" holds "segments" (rays + the chains' segments), "samples" (the
        traced (ray, light) items) and "hits" (the chains' crossings) in every
        call, the cell and test counters with stats=True.

        Two (n, 3) float32 CUDA tensors (torch-ROCm) on the context's device
        are traced in place, after a sync of torch's current stream: the
        outputs are (n, 3) float32 CUDA tensors, with hits=True "hits" as in
        trace()."""
        if not (irradiance or radiance):
            raise ValueError("direct: irradiance or radiance must be asked for")
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0) | (DIRECT_UNSHADOWED if unshadowed else 0)
        lights = list(lights)
        torch, n, rays = self._rays("direct", origins, dirs)
        if torch:
            irr = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if irradiance else None
            rad = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if radiance else None
            rec = torch.empty((n, 4), dtype=torch.float32, device=origins.device) if hits else None
            torch.cuda.current_stream(origins.device).synchronize()
            ptr = lambda x: x.data_ptr() if x is not None and n else None
        else:
            irr = np.empty((n, 3), np.float32) if irradiance else None
            rad = np.empty((n, 3), np.float32) if radiance else None
            rec = np.empty(n, HIT_DTYPE) if hits else None
            ptr = lambda x: x.ctypes.data if x is not None and n else None
        if n == 0:                                 # (an empty batch: any non-null output pointer passes the checks)
            st = self.direct_raw(0, None, lights, None, None, None, bool(torch), max_crossings, flags)
        else:
            st = self.direct_raw(n, ptr(rays), lights, ptr(irr), ptr(rad), ptr(rec), bool(torch), max_crossings, flags)
        res = {"stats": st}
        if irradiance:
            res["irradiance"] = irr
        if radiance:
            res["radiance"] = rad
        if hits and torch:
            res["hits"] = rec
        elif hits:
            res.update(t=rec["t"].copy(), u=rec["u"].copy(), v=rec["v"].copy(), triangle=rec["triangle"].copy())
        return res

    def area_lights_raw(self, num_rays: int, rays_ptr, emitters, irradiance_ptr, radiance_ptr, hits_ptr,
                        on_device: bool, spp: int, max_crossings: int = 16, seed: int = 0, index_base: int = 0,
                        flags: int = 0):
        """zrt_context_area_lights on raw pointers; `emitters`: an Emitters (or
        None).  Returns the stats dict."""
        batch = AreaLightBatch(int(num_rays), rays_ptr, emitters._h if emitters is not None else None, irradiance_ptr,
                               radiance_ptr, hits_ptr, 1 if on_device else 0, int(flags), int(spp), int(max_crossings),
                               int(seed) & (2 ** 64 - 1), int(index_base) & (2 ** 64 - 1))
        st = Stats()
        check(lib().zrt_context_area_lights(self._h, C.byref(batch), C.byref(st)), "zrt_context_area_lights")
        return st.as_dict()

    def area_lights(self, origins, dirs, emitters, spp: int, max_crossings: int = 16, seed: int = 0,
                    index_base: int = 0, flags: int = 0, unshadowed: bool = False, irradiance: bool = True,
                    radiance: bool = False, hits: bool = False, stats: bool = False):
        """Direct light of the scene's own emissive triangles at each ray's
        first hit (zrt_context_area_lights): `spp` next-event samples per ray
        from the set `emitters` (an Emitters of this context), drawn from the
        stream (seed, index_base + ray, sample), each shadowed through at most
        `max_crossings` transparent hits (unshadowed=True: T = 1, nothing
        traced).  Per ray the irradiance estimate and the Lambertian radiance
        emissive + base_color * irradiance / pi; a miss is zero in both.

        Inputs, outputs and "stats" are direct()'s: two (n, 3) float32 numpy
        arrays or CUDA tensors on the context's device; "samples" counts the
        traced (ray, sample) items."""
        if not (irradiance or radiance):
            raise ValueError("area_lights: irradiance or radiance must be asked for")
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0) | (AREA_UNSHADOWED if unshadowed else 0)
        torch, n, rays = self._rays("area_lights", origins, dirs)
        if torch:
            irr = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if irradiance else None
            rad = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if radiance else None
            rec = torch.empty((n, 4), dtype=torch.float32, device=origins.device) if hits else None
            torch.cuda.current_stream(origins.device).synchronize()
            ptr = lambda x: x.data_ptr() if x is not None and n else None
        else:
            irr = np.empty((n, 3), np.float32) if irradiance else None
            rad = np.empty((n, 3), np.float32) if radiance else None
            rec = np.empty(n, HIT_DTYPE) if hits else None
            ptr = lambda x: x.ctypes.data if x is not None and n else None
        st = self.area_lights_raw(n, ptr(rays), emitters, ptr(irr), ptr(rad), ptr(rec), bool(torch), spp,
                                  max_crossings, seed, index_base, flags)
        res = {"stats": st}
        if irradiance:
            res["irradiance"] = irr
        if radiance:
            res["radiance"] = rad
        if hits and torch:
            res["hits"] = rec
        elif hits:
            res.update(t=rec["t"].copy(), u=rec["u"].copy(), v=rec["v"].copy(), triangle=rec["triangle"].copy())
        return res

    def sky_light_raw(self, num_rays: int, rays_ptr, irradiance_ptr, radiance_ptr, visibility_ptr, hits_ptr,
                      on_device: bool, spp: int, max_crossings: int = 16, seed: int = 0, index_base: int = 0,
                      flags: int = 0):
        """zrt_context_sky_light on raw pointers.  Returns the stats dict."""
        batch = SkyLightBatch(int(num_rays), rays_ptr, irradiance_ptr, radiance_ptr, visibility_ptr, hits_ptr,
                              1 if on_device else 0, int(flags), int(spp), int(max_crossings),
                              int(seed) & (2 ** 64 - 1), int(index_base) & (2 ** 64 - 1))
        st = Stats()
        check(lib().zrt_context_sky_light(self._h, C.byref(batch), C.byref(st)), "zrt_context_sky_light")
        return st.as_dict()

    def sky_light(self, origins, dirs, spp: int, max_crossings: int = 16, seed: int = 0, index_base: int = 0,
                  flags: int = 0, unshadowed: bool = False, irradiance: bool = True, radiance: bool = True,
                  visibility: bool = True, hits: bool = False, stats: bool = False):
        """The sky's direct light at each ray's first hit
        (zrt_context_sky_light): `spp` cosine-weighted hemisphere samples per
        ray about the normalised shading normal, drawn from the stream (seed,
        index_base + ray, sample) as occlusion() draws them, each weighted by
        the reference's sky colour along it and shadowed through at most
        `max_crossings` transparent hits (unshadowed=True: T = 1, nothing
        traced).  Per ray the irradiance estimate pi * mean(L * T), the
        Lambertian radiance emissive + base_color * mean(L * T) and the
        visibility mean(T); a miss is zero in all three.

        Inputs and "stats" are area_lights()': two (n, 3) float32 numpy arrays
        or CUDA tensors on the context's device; "irradiance" and "radiance"
        are (n, 3) float32, "visibility" (n,) float32, each only when asked;
        "samples" counts the traced (ray, sample) items."""
        if not (irradiance or radiance or visibility):
            raise ValueError("sky_light: irradiance, radiance or visibility must be asked for")
        flags = int(flags) | (FLAG_COUNT_STATS if stats else 0) | (SKY_UNSHADOWED if unshadowed else 0)
        torch, n, rays = self._rays("sky_light", origins, dirs)
        if torch:
            irr = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if irradiance else None
            rad = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if radiance else None
            vis = torch.empty((n,), dtype=torch.float32, device=origins.device) if visibility else None
            rec = torch.empty((n, 4), dtype=torch.float32, device=origins.device) if hits else None
            torch.cuda.current_stream(origins.device).synchronize()
            ptr = lambda x: x.data_ptr() if x is not None and n else None
        else:
            irr = np.empty((n, 3), np.float32) if irradiance else None
            rad = np.empty((n, 3), np.float32) if radiance else None
            vis = np.empty(n, np.float32) if visibility else None
            rec = np.empty(n, HIT_DTYPE) if hits else None
            ptr = lambda x: x.ctypes.data if x is not None and n else None
        st = self.sky_light_raw(n, ptr(rays), ptr(irr), ptr(rad), ptr(vis), ptr(rec), bool(torch), spp, max_crossings,
                                seed, index_base, flags)
        res = {"stats": st}
        if irradiance:
            res["irradiance"] = irr
        if radiance:
            res["radiance"] = rad
        if visibility:
            res["visibility"] = vis
        if hits and torch:
            res["hits"] = rec
        elif hits:
            res.update(t=rec["t"].copy(), u=rec["u"].copy(), v=rec["v"].copy(), triangle=rec["triangle"].copy())
        return res

    def light_probes_raw(self, num_probes: int, positions_ptr, sh_ptr, distance_ptr, hits_ptr, directions_ptr,
                         radiance_ptr, on_device: bool, num_directions: int, spp: int, max_bounce: int, seed: int = 0,
                         index_base: int = 0, flags: int = 0, reserved: int = 0):
        """zrt_context_light_probes on raw pointers; returns the stats dict."""
        batch = LightProbeBatch(int(num_probes), positions_ptr, sh_ptr, distance_ptr, hits_ptr, directions_ptr,
                                radiance_ptr, 1 if on_device else 0, int(flags), int(num_directions), int(spp),
                                int(max_bounce), int(reserved), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                int(index_base) & 0xFFFFFFFFFFFFFFFF)
        st = Stats()
        check(lib().zrt_context_light_probes(self._h, C.byref(batch), C.byref(st)), "zrt_context_light_probes")
        return st.as_dict()

    def light_probes(self, positions, num_directions: int, spp: int, max_bounce: int, seed: int = 0,
                     index_base: int = 0, flags: int = 0, sh: bool = True, distance: bool = False, hits: bool = False,
                     directions: bool = False, radiance: bool = False):
        """The light arriving at each of n points (zrt_context_light_probes):
        `num_directions` random unit vectors per point, made on the device from
        the stream (seed, index_base + point * num_directions + j, sample
        65535), the path tracer's radiance along each (`spp` paths of at most
        `max_bounce` segments, as radiance()), projected onto the nine order-2
        real spherical harmonics and summed in direction order.

        An (n, 3) float32 numpy array gives, each only when asked, {"sh":
        (n, 9, 3) float32 -- coefficient k, RGB --, "distance": (n, 2) float32,
        the mean t and t * t of the first hits over all directions, "hits":
        (n,) uint32, the directions that hit, "directions" and "radiance":
        (n, num_directions, 3) float32, "stats"}.  "stats" holds "segments",
        "samples" and "hits" (the sum of the hits plane) in every call.

        An (n, 3) float32 CUDA tensor (torch-ROCm) on the context's device is
        read in place, after a sync of torch's current stream: the outputs are
        CUDA tensors of the same shapes ("hits" int32)."""
        if not (sh or distance or hits or directions or radiance):
            raise ValueError("light_probes: one output at least must be asked for")
        D = int(num_directions)
        torch = None
        if hasattr(positions, "is_cuda"):
            import torch
            if not positions.is_cuda or positions.dtype != torch.float32 or positions.dim() != 2 or \
                    positions.shape[1] != 3:
                raise ValueError("light_probes: an (n, 3) float32 CUDA tensor expected")
            pos = positions.contiguous()
            n = int(pos.shape[0])
            new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=pos.device)
            i32 = torch.int32
            ptr = lambda x: x.data_ptr() if x is not None and n else None
        else:
            pos = np.ascontiguousarray(positions, np.float32)
            if pos.ndim != 2 or pos.shape[1] != 3:
                raise ValueError("light_probes: an (n, 3) array expected")
            n = pos.shape[0]
            new = lambda shape, dt=np.float32: np.empty(shape, dt)
            i32 = np.uint32
            ptr = lambda x: x.ctypes.data if x is not None and n else None
        out = {"sh": new((n, 9, 3)) if sh else None, "distance": new((n, 2)) if distance else None,
               "hits": new((n,), i32) if hits else None, "directions": new((n, D, 3)) if directions else None,
               "radiance": new((n, D, 3)) if radiance else None}
        if torch:
            torch.cuda.current_stream(pos.device).synchronize()
        st = self.light_probes_raw(n, ptr(pos), ptr(out["sh"]), ptr(out["distance"]), ptr(out["hits"]),
                                   ptr(out["directions"]), ptr(out["radiance"]), bool(torch), D, spp, max_bounce, seed,
                                   index_base, flags)
        res = {k: v for k, v in out.items() if v is not None}
        res["stats"] = st
        return res

    def radiance_raw(self,num_rays: int, rays_ptr, radiance_ptr, rgb_ptr, on_device: bool, spp: int,
                     max_bounce: int, seed: int = 0, index_base: int = 0, flags: int = 0):
        """zrt_context_radiance on raw pointers; returns the stats dict."""
        batch = RadianceBatch(int(num_rays), rays_ptr, radiance_ptr, rgb_ptr, 1 if on_device else 0, int(flags),
                              int(spp), int(max_bounce), int(seed), int(index_base))
        st = Stats()
        check(lib().zrt_context_radiance(self._h, C.byref(batch), C.byref(st)), "zrt_context_radiance")
        return st.as_dict()

    def radiance(self, origins, dirs, spp: int, max_bounce: int, seed: int = 0, index_base: int = 0,
                 flags: int = 0, rgb: bool = False, stats: bool = False):
        """Scene.traceRayRecursive (stage3.zig:188-220) along n rays of the
        caller's: the mean of `spp` path samples per ray, each traced as a
        render traces a pixel's sample (include/zrt.h, zrt_context_radiance).
        `dirs` need not be unit length.  Ray i draws from the RNG stream of
        "pixel" index_base + i, so a batch cut in two gives the same rows.

        Two (n, 3) float32 numpy arrays give {"radiance": (n, 3) float32
        linear, "rgb": (n, 3) uint8 (with rgb=True), "stats"}.  Two (n, 3)
        float32 CUDA tensors (torch-ROCm) on the context's device are used in
        place, after a sync of torch's current stream, and the results are
        CUDA tensors, complete when the call returns.  `stats` is always
        filled (no counting variant exists); the argument is kept for symmetry
        with trace()."""
        del stats
        torch, n, rays = self._rays("radiance", origins, dirs)
        if torch:
            out = torch.empty((n, 3), dtype=torch.float32, device=origins.device)
            out8 = torch.empty((n, 3), dtype=torch.uint8, device=origins.device) if rgb else None
            torch.cuda.current_stream(origins.device).synchronize()
            st = self.radiance_raw(n, rays.data_ptr() if n else None, out.data_ptr() if n else None,
                                   out8.data_ptr() if rgb and n else None, True, spp, max_bounce, seed,
                                   index_base, flags)
            res = {"radiance": out, "stats": st}
            if rgb:
                res["rgb"] = out8
            return res
        out = np.empty((n, 3), np.float32)
        out8 = np.empty((n, 3), np.uint8) if rgb else None
        st = self.radiance_raw(n, rays.ctypes.data if n else None, out.ctypes.data if n else None,
                               out8.ctypes.data if rgb and n else None, False, spp, max_bounce, seed, index_base,
                               flags)
        res = {"radiance": out, "stats": st}
        if rgb:
            res["rgb"] = out8
        return res


class History:
    """The history of an interactive preview under a moving camera: the
    colour, history-length, depth and normal (and base-colour) planes of one
    frame size, on the context's device as torch tensors in tile_pixels(w, h,
    tile) order.  update() after each frame's Context.accumulate; its result
    goes to Context.denoise."""

    def __init__(self, context: "Context", w: int, h: int, tile: int = 64, max_history: int = REPROJECT_DEFAULTS[0],
                 depth_tolerance: float = REPROJECT_DEFAULTS[1], normal_tolerance: float = REPROJECT_DEFAULTS[2],
                 device=None):
        import torch
        self._context = context
        self.w, self.h, self.tile = int(w), int(h), int(tile) or 64
        self.max_history, self.depth_tolerance, self.normal_tolerance = max_history, depth_tolerance, normal_tolerance
        P = self.w * self.h
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.color = torch.zeros((P, 3), dtype=torch.float32, device=dev)
        self.length = torch.zeros((P,), dtype=torch.int32, device=dev)
        # the guides of the current frame and of the previous one, swapped by every update
        self._guides = [{"base_color": torch.zeros((P, 3), dtype=torch.float32, device=dev),
                         "normal": torch.zeros((P, 3), dtype=torch.float32, device=dev),
                         "depth": torch.zeros((P,), dtype=torch.float32, device=dev)} for _ in range(2)]
        self.camera = None               # the previous update's; None: no history yet
        self.stats = None                # the last update's reproject stats
        torch.cuda.synchronize(dev)

    def reset(self):
        """Forget the history: the next update yields the film's frame, lengths 1."""
        self.camera = None

    def update(self, film: "Film", camera: Camera, seed: int = 0, num_samples: int = 4, **features_kw):
        """One frame: Context.features(camera, num_samples, seed) into the
        history's own planes, then the film's frame so far reprojected in
        place against the previous update's guides and camera.  The first
        update (or the first after reset()) has no history: the film's frame,
        lengths 1.  Returns {"color", "normal", "depth", "albedo"}: what
        Context.denoise(w, h, tile=history.tile, **result) takes; the lengths
        are in .length, the call's stats in .stats."""
        if (film.w, film.h, film.tile) != (self.w, self.h, self.tile) or camera.w != self.w or camera.h != self.h:
            raise ValueError("History.update: the film and the camera must have the history's w, h and tile")
        cur, prev = self._guides
        self._context.features_raw(camera, num_samples, {k: v.data_ptr() for k, v in cur.items()}, True, seed,
                                   tile_size=self.tile, **features_kw)
        first = self.camera is None
        # (no history: the frame against itself with max_history 1 is the film's colour bit for bit, lengths 1)
        self.stats = self._context.reproject(
            camera, camera if first else self.camera, film=film, depth=cur["depth"], normal=cur["normal"],
            prev_color=self.color, prev_depth=cur["depth"] if first else prev["depth"],
            prev_normal=cur["normal"] if first else prev["normal"], prev_length=None if first else self.length,
            max_history=1 if first else self.max_history, depth_tolerance=self.depth_tolerance,
            normal_tolerance=self.normal_tolerance, tile=self.tile, out=self.color, length_out=self.length)["stats"]
        self.camera = Camera.from_buffer_copy(camera)
        self._guides = [prev, cur]
        return {"color": self.color, "normal": cur["normal"], "depth": cur["depth"], "albedo": cur["base_color"]}


class SvgfHistory:
    """History's counterpart for Context.svgf: the illumination (the colour
    divided by the first-hit albedo), the luminance-moments and the
    history-length planes of one frame size beside the two guide sets, on the
    context's device as torch tensors in tile_pixels(w, h, tile) order.
    update() after each frame's Context.accumulate; its result goes to
    Context.svgf."""

    def __init__(self, context: "Context", w: int, h: int, tile: int = 64, max_history: int = REPROJECT_DEFAULTS[0],
                 depth_tolerance: float = REPROJECT_DEFAULTS[1], normal_tolerance: float = REPROJECT_DEFAULTS[2],
                 device=None):
        import torch
        self._context = context
        self.w, self.h, self.tile = int(w), int(h), int(tile) or 64
        self.max_history, self.depth_tolerance, self.normal_tolerance = max_history, depth_tolerance, normal_tolerance
        P = self.w * self.h
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.color = torch.zeros((P, 3), dtype=torch.float32, device=dev)       # the illumination's history
        self.moments = torch.zeros((P, 3), dtype=torch.float32, device=dev)
        self.length = torch.zeros((P,), dtype=torch.int32, device=dev)
        # both reprojections of a frame read .length; they write this plane, which then takes its place
        self._length_next = torch.zeros((P,), dtype=torch.int32, device=dev)
        # this frame's illumination and moments before they are blended into the histories
        self._frame = [torch.zeros((P, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        # the guides of the current frame and of the previous one, swapped by every update
        self._guides = [{"base_color": torch.zeros((P, 3), dtype=torch.float32, device=dev),
                         "normal": torch.zeros((P, 3), dtype=torch.float32, device=dev),
                         "depth": torch.zeros((P,), dtype=torch.float32, device=dev)} for _ in range(2)]
        self.camera = None               # the previous update's; None: no history yet
        self.stats = None                # the last update's reproject stats: (illumination's, moments')
        torch.cuda.synchronize(dev)

    def reset(self):
        """Forget the history: the next update yields the film's frame, lengths 1."""
        self.camera = None

    def update(self, film: "Film", camera: Camera, seed: int = 0, num_samples: int = 4, **features_kw):
        """One frame: Context.features(camera, num_samples, seed) into the
        history's own planes, the film's frame so far demodulated by the new
        base colour (Context.illumination), then the illumination and its
        moments each reprojected in place against the previous update's
        guides, camera and lengths.  The lengths are written once, after both
        calls have read the previous ones.  The first update (or the first
        after reset()) has no history: the frame itself, lengths 1.  Returns
        {"color", "moments", "length", "normal", "depth", "albedo"}: what
        Context.svgf(w, h, tile=history.tile, **result) takes; the calls'
        stats are in .stats."""
        if (film.w, film.h, film.tile) != (self.w, self.h, self.tile) or camera.w != self.w or camera.h != self.h:
            raise ValueError("SvgfHistory.update: the film and the camera must have the history's w, h and tile")
        cur, prev = self._guides
        self._context.features_raw(camera, num_samples, {k: v.data_ptr() for k, v in cur.items()}, True, seed,
                                   tile_size=self.tile, **features_kw)
        illum, mom = self._frame
        self._context.illumination(self.w, self.h, film=film, albedo=cur["base_color"], tile=self.tile, out=illum,
                                   moments_out=mom)
        first = self.camera is None
        # (no history: the frame against itself with max_history 1 is the frame bit for bit, lengths 1)
        common = dict(depth=cur["depth"], normal=cur["normal"], prev_depth=cur["depth"] if first else prev["depth"],
                      prev_normal=cur["normal"] if first else prev["normal"],
                      prev_length=None if first else self.length, max_history=1 if first else self.max_history,
                      depth_tolerance=self.depth_tolerance, normal_tolerance=self.normal_tolerance, tile=self.tile,
                      length_out=self._length_next)
        prev_camera = camera if first else self.camera
        self.stats = tuple(self._context.reproject(camera, prev_camera, color=now, prev_color=hist, out=hist,
                                                   **common)["stats"]
                           for now, hist in ((illum, self.color), (mom, self.moments)))
        self.length, self._length_next = self._length_next, self.length
        self.camera = Camera.from_buffer_copy(camera)
        self._guides = [prev, cur]
        return {"color": self.color, "moments": self.moments, "length": self.length, "normal": cur["normal"],
                "depth": cur["depth"], "albedo": cur["base_color"]}


def render_oneshot(scene: Scene, cam: Camera, spp: int, max_bounce: int, seed: int = 0,
                   device: int = -1, devices=None, num_devices=None):
    """zrt_render: the one-shot drop-in for Scene.render (stage3.zig:247) --
    upload, render the whole image, download, free.  `devices`: a list of
    HIP ordinals (repeats allowed) to split the image's tiles over
    (zrt_render_config.devices / num_devices).  Returns (h, w, 3) RGB8."""
    cfg = RenderConfig()
    cfg.num_samples, cfg.max_bounce, cfg.seed, cfg.device = spp, max_bounce, seed, device
    cfg.num_ranks = 1
    if devices is not None:
        dl = (C.c_int32 * len(devices))(*devices)
        cfg.num_devices, cfg.devices = len(devices), dl
    elif num_devices is not None:      # a count without a list (ABI-1 callers)
        cfg.num_devices = num_devices
    img = np.zeros((cam.h, cam.w, 3), np.uint8)
    st = Stats()
    check(lib().zrt_render(C.byref(scene), C.byref(cam), C.byref(cfg), img.ctypes.data, C.byref(st)),
          "zrt_render")
    return img, st.as_dict()


class Group:
    """zrt_group: one context per device of `devices` (repeats allowed), one
    render call splitting the image's tiles over them and gathering them over
    xGMI into one image (Scene.render's spawn + join, stage3.zig:247-256)."""

    def __init__(self, scene: Scene, devices):
        self._dev = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        check(lib().zrt_group_create(C.byref(scene), self._dev, len(devices), C.byref(h)), "zrt_group_create")
        self._h = h
        self.devices = list(devices)

    @classmethod
    def built(cls, pos, nrm, uv, mat, materials: Scene, devices, resolution=(128, 128, 128)):
        """zrt_group_create_built: the grid built on every device."""
        keep = [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32),
                np.ascontiguousarray(uv, np.float32), np.ascontiguousarray(mat, np.uint32)]
        res = (C.c_uint32 * 3)(*resolution)
        self = cls.__new__(cls)
        self._dev = (C.c_int32 * len(devices))(*devices)
        self.devices = list(devices)
        h = C.c_void_p()
        check(lib().zrt_group_create_built(*[k.ctypes.data for k in keep], keep[3].size, res,
                                           materials.num_materials, materials.materials, materials.texels,
                                           materials.num_texel_floats, self._dev, len(devices), C.byref(h)),
              "zrt_group_create_built")
        self._h = h
        return self

    def render(self, cam: Camera, spp: int, max_bounce: int, seed: int = 0, rank: int = 0, num_ranks: int = 1,
               image=None, flags=0):
        """Returns ((h, w, 3) RGB8 with this process's pixels, stats dict)."""
        cfg = RenderConfig()
        cfg.num_samples, cfg.max_bounce, cfg.seed = spp, max_bounce, seed
        cfg.rank, cfg.num_ranks, cfg.flags = rank, num_ranks, flags
        img = np.zeros((cam.h, cam.w, 3), np.uint8) if image is None else image
        st = Stats()
        check(lib().zrt_group_render(self._h, C.byref(cam), C.byref(cfg), img.ctypes.data, C.byref(st)),
              "zrt_group_render")
        return img, st.as_dict()

    def close(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.zrt_group_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def timed_kernels():
    """Mangled-name substrings of the timed kernel instantiations (no HIP call)."""
    return lib().zrt_timed_kernels().decode().split(",")


# bytes per item the probe reads / writes (probe.hip zrt_probe)
_PROBE_IO = {PROBE_TRIANGLE: (60, 16), PROBE_TRIANGLE_FLAT: (60, 16), PROBE_BBOX: (48, 8),
             PROBE_DDA: (48, 4 * DDA_PROBE_WIDTH), PROBE_TO_RGB: (12, 12), PROBE_RNG_F32: (12, 64),
             PROBE_RNG_NORM: (12, 64), PROBE_EXP_LOG: (8, 16), PROBE_TEXTURE: (8, 12),
             PROBE_RECIP: (4, 8), PROBE_RECIP_SWEEP: (8, 16), PROBE_TRIANGLE_EXACT: (60, 16),
             PROBE_QUOT: (8, 8), PROBE_QUOT_SWEEP: (8, 16)}


def probe(which, inp: np.ndarray, n: int, out_shape, out_dtype=np.float32, aux=None, device=-1):
    inp = np.ascontiguousarray(inp)
    out = np.zeros(out_shape, out_dtype)
    in_b, out_b = _PROBE_IO[which]
    if inp.nbytes < n * in_b or out.nbytes < n * out_b:
        raise ValueError(f"probe {which}: buffers too small for {n} items")
    auxp = None if aux is None else np.ascontiguousarray(aux).ctypes.data
    check(lib().zrt_probe(which, inp.ctypes.data, out.ctypes.data, n, auxp, device), "zrt_probe")
    return out


class Gltf:
    """stage1: glTF/GLB load through the C ABI (zrt_gltf_*)."""

    def __init__(self, path: str, num_threads: int = 0):
        h = C.c_void_p()
        check(lib().zrt_gltf_load(path.encode(), num_threads, C.byref(h)), f"zrt_gltf_load({path})")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.zrt_gltf_free(self._h)
            self._h = None

    def soup(self):
        ptrs = [C.c_void_p() for _ in range(4)]
        n = C.c_uint32(0)
        check(lib().zrt_gltf_soup(self._h, *[C.byref(p) for p in ptrs], C.byref(n)), "zrt_gltf_soup")
        k = n.value

        def arr(p, shape, ctype, dtype):
            if k == 0:
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape).copy()
        return (arr(ptrs[0], (k, 9), C.c_float, np.float32), arr(ptrs[1], (k, 9), C.c_float, np.float32),
                arr(ptrs[2], (k, 6), C.c_float, np.float32), arr(ptrs[3], (k,), C.c_uint32, np.uint32))

    def materials(self):
        s = Scene()
        check(lib().zrt_gltf_materials(self._h, C.byref(s)), "zrt_gltf_materials")
        desc = np.zeros((s.num_materials, 3, 7), np.int64)
        for i in range(s.num_materials):
            m = s.materials[i]
            for k, name in enumerate(("base_color", "emissive", "transparency")):
                t = getattr(m, name)
                desc[i, k] = (t.offset, t.w, t.h, t.u_min, t.u_max, t.v_min, t.v_max)
        tex = np.ctypeslib.as_array(s.texels, (s.num_texel_floats,)).copy()
        return desc, tex

    def camera(self, name=None, width=None, height=None) -> Camera:
        cam = Camera()
        check(lib().zrt_gltf_camera(self._h, None if name is None else name.encode(),
                                    -1 if width is None else width, -1 if height is None else height,
                                    C.byref(cam)), "zrt_gltf_camera")
        return cam
