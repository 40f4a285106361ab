"""Host reference of the project's random draws: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
as 1, 2, 3", SC'11, section 3.3 and the Random123 constants) vectorised in numpy, and what the kernels derive from its words.

One Philox round on a counter (c0, c1, c2, c3) with key (k0, k1):
    hi0:lo0 = M0 * c0,  hi1:lo1 = M1 * c2          (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
and between rounds the key is bumped by the Weyl constants (W0, W1).  Ten rounds, nine key bumps.

Counter conventions (include/jckgan.h): the step's small draws use counter = (index / 4 lo, hi, tensor id, step) with tensor id
8 (z), 9 (alpha), 10 (masks) and element index = 4 * counter + word; the image noise uses counter = (pixel lo, hi, tensor id, step)
with pixel = n * HW + px over the whole batch.  key = (seed lo, seed hi) everywhere."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # PHILOX_M4x32_0 / _1
W0, W1 = 0x9E3779B9, 0xBB67AE85          # golden ratio, sqrt(3) - 1
MASK = np.uint64(0xFFFFFFFF)
TENSOR_Z, TENSOR_ALPHA, TENSOR_MASKS = 8, 9, 10


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit words, key: two -> four uint32 arrays, broadcast against each other."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & MASK for x in key]
    c = list(np.broadcast_arrays(*c))
    s32 = np.uint64(32)
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # < 2^64: no wrap
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> s32) ^ c[3] ^ k[1], p0 & MASK]
    return [x.astype(np.uint32) for x in c]


def _words(index, tensor_id, step, seed):
    """the four output words of counter (index lo, index hi, tensor id, step) -> uint32 [4, len(index)]"""
    index = np.asarray(index, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.stack(philox4x32((index & MASK, index >> np.uint64(32), tensor_id, int(step) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32)))


def quad_words(n, tensor_id, step, seed):
    """words of elements 0 .. n-1 of a small draw: element 4 * i + k is word k of counter i -> uint32 [n]"""
    q = (n + 3) // 4
    o = _words(np.arange(q, dtype=np.uint64), tensor_id, step, seed)          # [4, q]
    return o.T.reshape(-1)[:n]


def u24(o):
    """float32(o >> 8): the top 24 bits, exact in float32"""
    return (np.asarray(o, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)


def alpha_from_words(o):
    """[0, 1): float32(o >> 8) * 2^-24 (exact)"""
    return u24(o) * np.float32(2.0 ** -24)


def u01_from_words(o):
    """(0, 1]: (float32(o >> 8) + 0.5f) * 2^-24 evaluated in float32 - from o >> 8 = 2^23 on the sum has no half bit left and
    rounds to even, so the top value is exactly 1.0"""
    s = u24(o) + np.float32(0.5)
    assert s.dtype == np.float32
    return s * np.float32(2.0 ** -24)


def alpha_ref(n, step, seed):
    return alpha_from_words(quad_words(n, TENSOR_ALPHA, step, seed))


def masks_ref(n, step, seed, keep_p):
    return (alpha_from_words(quad_words(n, TENSOR_MASKS, step, seed)) < np.float32(keep_p)).astype(np.float32)


def box_muller_z(o):
    """o: uint32 [4, q] -> (z float64 [4, q], radius float64 [4, q]) in the order r0*c0, r0*s0, r1*c1, r1*s1: radius
    sqrt(-2 ln u) in float64 from the float32 u of words 0 / 2, angle float32(6.2831855f * u) of words 1 / 3 as float32 rounds
    the product, its cos / sin in float64."""
    u = u01_from_words(o)
    r0, r1 = np.sqrt(-2.0 * np.log(u[0].astype(np.float64))), np.sqrt(-2.0 * np.log(u[2].astype(np.float64)))
    two_pi = np.float32(6.283185307179586)
    a0, a1 = (two_pi * u[1]).astype(np.float64), (two_pi * u[3]).astype(np.float64)
    assert (two_pi * u[1]).dtype == np.float32
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)]), np.stack([r0, r0, r1, r1])


def z_ref(n, step, seed):
    """-> (z float64 [n], radius float64 [n])"""
    q = (n + 3) // 4
    z, r = box_muller_z(_words(np.arange(q, dtype=np.uint64), TENSOR_Z, step, seed))
    return z.T.reshape(-1)[:n], r.T.reshape(-1)[:n]


def pixel_normals_ref(npix, tensor_id, step, seed, first=0):
    """Three normals of pixels first .. first + npix - 1 -> (float64 [npix, 3], radius float64 [npix, 3]):
    r = sqrt(-2 ln2 * log2 u) of words 0 / 2, angles of words 1 / 3 in revolutions; r0 cos(u1), r0 sin(u1), r1 cos(u3)."""
    o = _words(np.arange(first, first + npix, dtype=np.uint64), tensor_id, step, seed)
    u = u01_from_words(o).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(2.0) * np.log2(u[0])), np.sqrt(-2.0 * np.log(2.0) * np.log2(u[2]))
    t = 2.0 * np.pi
    return np.stack([r0 * np.cos(t * u[1]), r0 * np.sin(t * u[1]), r1 * np.cos(t * u[3])], axis=1), np.stack([r0, r0, r1], axis=1)
