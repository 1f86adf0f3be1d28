"""The noise_mode="keyed" stream of include/mgf.h (mgf_randn_keyed_f32) restated in numpy: Philox4x32-10 in exact integer arithmetic on the
counter {q, l, s_j, aux_j} under the key {key low, key high}, then Box-Muller in float64 from u = (float32(c) + 0.5f) * 2^-32 -- those two
float32 operations restated exactly (the conversion rounds to nearest even, the sum and the product by a power of two round once each)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of 32-bit words held in uint64; returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                        # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def philox4x32_10_scalar(ctr, key):
    """A second, scalar implementation in Python integers (the self-consistency partner of the array form)."""
    c, k = [int(x) & 0xFFFFFFFF for x in ctr], [int(x) & 0xFFFFFFFF for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def uniform_f32(c):
    """u = ((float) c + 0.5f) * 2^-32 as the kernel computes it, float32."""
    f = np.asarray(c, dtype=np.uint64).astype(np.float32)                 # round to nearest even, like the device's conversion
    return (f + np.float32(0.5)) * np.float32(2.3283064365386963e-10)


def normals_from_words(c):
    """[..., 4] float64 normals of the four output words (arrays of equal shape)."""
    z = []
    for h in (0, 1):
        u1 = np.minimum(uniform_f32(c[2 * h]), np.float32(0.99999994)).astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u1))
        a = np.float32(2.0) * uniform_f32(c[2 * h + 1])                   # the kernel's 2.f * u2 (exact: a power of two), then sincospif
        a = a.astype(np.float64)
        z += [r * np.cos(np.pi * a), r * np.sin(np.pi * a)]
    return np.stack(z, axis=-1)


def map_normals(side, layer, step, aux, key):
    """One sample's map of one layer: [side * side] float64."""
    quads = side * side // 4
    q = np.arange(quads, dtype=np.uint64)
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10(q, layer, int(step) & 0xFFFFFFFF, int(aux) & 0xFFFFFFFF, key & 0xFFFFFFFF, key >> 32)
    return normals_from_words(words).reshape(-1)


def randn_keyed_ref(sides, n, key, step, step_stride=0, step_add=1, step_max=2 ** 31 - 1, aux0=1, aux_add=0):
    """The whole buffer of mgf_randn_keyed_f32: flat float64, layer-major [layer][n][side * side].  step: the device counters as a sequence."""
    step = np.atleast_1d(np.asarray(step, dtype=np.int64))
    out = []
    for l, side in enumerate(sides):
        for j in range(n):
            s = min(int(step[j * step_stride]) + j * step_add, step_max)
            out.append(map_normals(side, l, s, aux0 + j * aux_add, key))
    return np.concatenate(out)
