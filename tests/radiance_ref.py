"""Scene.traceRayRecursive (stage3.zig:188-220) along caller-given rays, from
the CPU oracle -- the reference of the radiance-query tests
(test_radiance_host.py, test_radiance_gpu.py); not a test module itself.

A camera with origin = o, lower_left_corner = d and right = up = 0 makes
Camera.getRay (stage3.zig:27-35) return (o, normalize(d)) whatever the jitter,
so OracleScene.render_pixels(cam, spp, max_bounce, [i]) of that 1x1 camera is
the counter-RNG stream of "pixel" i along the ray: the linear radiance
(sample-ordered sum times 1 / spp), its RGB8 and the traversal counters.  One
call per ray, one thread.
"""
import numpy as np


def degenerate_camera(orc, o, d):
    """The 1x1 oracle camera whose every ray is (o, normalize(d))."""
    return orc.camera_from_dict({"w": 1, "h": 1, "origin": [float(x) for x in o], "llc": [float(x) for x in d],
                                 "right": [0.0, 0.0, 0.0], "up": [0.0, 0.0, 0.0]})


class RadianceRef:
    """The oracle's scene of (soup, res) and radiance(origins, dirs, ...) against it."""

    def __init__(self, orc, soup, res):
        self.orc = orc
        self.scene = orc.OracleScene(soup, tuple(int(r) for r in res))

    def radiance(self, origins, dirs, spp, max_bounce, seed=0, index_base=0):
        """((n, 3) float32 linear, (n, 3) uint8, the summed counters
        [segments, cells, tests, hits, samples]); ray i takes the stream key
        (index_base + i) mod 2^32."""
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        lin = np.zeros((n, 3), np.float32)
        rgb = np.zeros((n, 3), np.uint8)
        ctr = np.zeros(5, np.uint64)
        for i in range(n):
            cam = degenerate_camera(self.orc, o[i], d[i])
            key = (int(index_base) + i) & 0xFFFFFFFF
            r, l, c = self.scene.render_pixels(cam, spp, max_bounce, [key], seed=seed, num_threads=1)
            rgb[i], lin[i] = r[0], l[0]
            ctr += c
        return lin, rgb, ctr
