"""What traceRayRecursive computes between stage3.zig:199 and :206 at a ray's
first hit, plus the continuation origin of :209 / :216 -- the reference of
the surface-query tests (test_surface_host.py, test_surface_gpu.py); not a
test module itself.

Built from the trace reference's (t, u, v, ref) of the ray (trace_ref.RayRef:
no walking of its own), Geometry.indices (ref -> source triangle), the soup's
normals, uvs, material indices, texture descriptors and texel pool, numpy
float32 scalar arithmetic in the reference's order -- left to right, nothing
contracted, the third weight (1 - u) - v -- and the oracle's Texture.sample
(oracle.tex_sample).

The 16 words of a zrt_surface: position xyz, material | normal xyz,
transparency | base_color xyz, texcoord_s | emissive xyz, texcoord_t.  A miss
is fifteen zero words and material = 0xFFFFFFFF.
"""
import numpy as np

MISS = 0xFFFFFFFF
INF_BITS = 0x7F800000
F = np.float32
EPS = F(1.1920928955078125e-07)          # std.math.floatEps(f32)
MISS_WORDS = np.array([0, 0, 0, MISS] + [0] * 12, np.uint32)
FIELDS = ("position", "material", "normal", "transparency", "base_color", "texcoord_s", "emissive", "texcoord_t")


def sample(orc, soup, mat, slot, s, t):
    """material `mat`'s texture `slot` (0 base colour, 1 emissive: 3 channels;
    2 transparency: 1) sampled at (s, t)."""
    off, w, h, umin, umax, vmin, vmax = (int(x) for x in soup.tex_desc[mat, slot])
    chans = 3 if slot < 2 else 1
    data = np.asarray(soup.texels, np.float32)[off:off + w * h * chans]
    return orc.tex_sample(data, chans, w, h, umin, umax, vmin, vmax, float(s), float(t))


def surface_ref(ref, soup, o, d, hit_bits):
    """The 16 uint32 words of the ray's zrt_surface; `hit_bits`: the (t, u, v,
    ref) patterns of ref.trace_batch for this ray."""
    hit_bits = np.asarray(hit_bits, np.uint32)
    if int(hit_bits[3]) == MISS:
        assert int(hit_bits[0]) == INF_BITS
        return MISS_WORDS.copy()
    t, u, v = (F(x) for x in hit_bits[:3].view(np.float32))
    src = int(ref.indices[int(hit_bits[3])])
    n = np.asarray(soup.nrm, np.float32).reshape(-1, 9)[src]
    uv = np.asarray(soup.uv, np.float32).reshape(-1, 6)[src]
    mat = int(soup.mat[src])
    o = [F(x) for x in np.asarray(o, np.float32)]
    d = [F(x) for x in np.asarray(d, np.float32)]
    with np.errstate(all="ignore"):
        w0 = (F(1.0) - u) - v
        tc = [(uv[k] * w0 + uv[2 + k] * u) + uv[4 + k] * v for k in range(2)]         # stage3.zig:63-64
        nrm = [(n[k] * w0 + n[3 + k] * u) + n[6 + k] * v for k in range(3)]           # stage3.zig:59
        tt = t + EPS
        pos = [o[k] + d[k] * tt for k in range(3)]                                     # ray.at(t + eps)
    base = sample(ref.orc, soup, mat, 0, tc[0], tc[1])
    emis = sample(ref.orc, soup, mat, 1, tc[0], tc[1])
    tran = sample(ref.orc, soup, mat, 2, tc[0], tc[1])
    out = np.zeros(16, np.uint32)
    f = out.view(np.float32)
    f[0:3] = pos
    out[3] = mat
    f[4:7] = nrm
    f[7] = tran[0]
    f[8:11] = base
    f[11] = tc[0]
    f[12:15] = emis
    f[15] = tc[1]
    return out


def surface_batch(ref, soup, origins, dirs, bits):
    """(n, 16) uint32: surface_ref of every ray of a batch."""
    return np.stack([surface_ref(ref, soup, o, d, b) for o, d, b in zip(origins, dirs, bits)]) \
        if len(origins) else np.zeros((0, 16), np.uint32)


def cached_batch(cs):
    """surface_batch of a test case (its ref, soup, o, d and bits), computed
    once, kept on the case and left unchanged."""
    if not hasattr(cs, "_surface_words"):
        words = surface_batch(cs.ref, cs.soup, cs.o, cs.d, cs.bits)
        words.setflags(write=False)
        cs._surface_words = words
    return cs._surface_words


def surface_bits(res):
    """Context.surface's numpy result as the (n, 16) uint32 array of surface_batch."""
    n = len(res["material"])
    out = np.zeros((n, 16), np.uint32)
    f = out.view(np.float32)
    f[:, 0:3] = res["position"]
    out[:, 3] = res["material"]
    f[:, 4:7] = res["normal"]
    f[:, 7] = res["transparency"]
    f[:, 8:11] = res["base_color"]
    f[:, 11] = res["texcoord_s"]
    f[:, 12:15] = res["emissive"]
    f[:, 15] = res["texcoord_t"]
    return out
