"""tests/philox_ref.py against the published Random123 known answers (kat_vectors, philox4x32 10 rounds), and its derived
references against each other - the GPU tests of the draws (tests/test_rng_exact_gpu.py) stand on this module."""
import numpy as np

import philox_ref as P

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _scalar_philox(c, k, rounds=10):
    """plain Python integers, one block"""
    c, k = list(c), list(k)
    for r in range(rounds):
        if r:
            k = [(k[0] + P.W0) & 0xffffffff, (k[1] + P.W1) & 0xffffffff]
        p0, p1 = P.M0 * c[0], P.M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
    return tuple(c)


def test_known_answers():
    for c, k, want in KAT:
        got = tuple(int(x) for x in P.philox4x32(c, k))
        assert got == want, ([hex(x) for x in got], [hex(x) for x in want])
        assert _scalar_philox(c, k) == want
    # all three as one vectorised call
    cs, ks = np.array([c for c, _, _ in KAT], dtype=np.uint64).T, np.array([k for _, k, _ in KAT], dtype=np.uint64).T
    got = np.stack(P.philox4x32(cs, ks)).T
    assert got.tolist() == [list(w) for _, _, w in KAT]


def test_round_count_and_every_input_word_matter():
    """what the statistical tests cannot see: nine rounds, or any counter / key word left out, give other words"""
    c, k = KAT[2][0], KAT[2][1]
    base = tuple(int(x) for x in P.philox4x32(c, k))
    assert tuple(int(x) for x in P.philox4x32(c, k, rounds=9)) != base
    for i in range(4):
        c2 = list(c)
        c2[i] ^= 1
        assert tuple(int(x) for x in P.philox4x32(c2, k)) != base
    for i in range(2):
        k2 = list(k)
        k2[i] ^= 1
        assert tuple(int(x) for x in P.philox4x32(c, k2)) != base


def test_vectorised_words_against_the_scalar_transcription():
    seed, step = (0x1234 << 32) | 0x9abcdef0, 7
    o = P._words(np.array([0, 1, 5, 2 ** 32 + 3], dtype=np.uint64), 9, step, seed)
    for j, idx in enumerate([0, 1, 5, 2 ** 32 + 3]):
        want = _scalar_philox((idx & 0xffffffff, idx >> 32, 9, step), (seed & 0xffffffff, seed >> 32))
        assert tuple(int(x) for x in o[:, j]) == want
    q = P.quad_words(11, 9, step, seed)            # element 4 i + k = word k of counter i
    assert q.shape == (11,) and int(q[5]) == int(o[1, 1]) and int(q[3]) == int(o[3, 0]) and int(q[4]) == int(o[0, 1])


def test_uniforms():
    edge = np.array([0, 255, 256, (2 ** 23 - 1) << 8, 2 ** 31, (2 ** 24 - 2) << 8, 0xffffffff], dtype=np.uint32)
    a = P.alpha_from_words(edge)
    assert a.dtype == np.float32 and a[0] == 0.0 and a[1] == 0.0 and a[2] == np.float32(2.0 ** -24) and a[-1] == np.float32(1 - 2.0 ** -24)
    u = P.u01_from_words(edge)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)                 # the last value whose half bit survives
    assert u[4] == np.float32(0.5)                                          # 2^23 + 0.5 ties to even: 2^23
    assert u[5] == np.float32(1 - 2.0 ** -23) and u[6] == np.float32(1.0)   # 2^24 - 1 + 0.5 ties to even: 2^24 -> u = 1 exactly
    assert np.all(u > 0)


def test_derived_references_agree():
    seed, step, n = (77 << 32) | 5, 3, 1003
    w = P.quad_words(n, P.TENSOR_MASKS, step, seed)
    for keep in (0.75, 0.3):
        m = P.masks_ref(n, step, seed, keep)
        assert np.array_equal(m, (P.alpha_from_words(w) < np.float32(keep)).astype(np.float32))
        assert set(np.unique(m).tolist()) == {0.0, 1.0} and abs(m.mean() - keep) < 0.05
    # masks of tensor id 10 are NOT alpha (tensor id 9) thresholded: the ids separate the streams
    assert not np.array_equal(P.masks_ref(n, step, seed, 0.75), (P.alpha_ref(n, step, seed) < np.float32(0.75)).astype(np.float32))
    a = P.alpha_ref(n, step, seed)
    assert a.dtype == np.float32 and a.min() >= 0 and a.max() < 1 and abs(a.mean() - 0.5) < 0.05
    # ragged counts are prefixes
    assert np.array_equal(P.alpha_ref(n - 2, step, seed), a[:n - 2])
    z, r = P.z_ref(n, step, seed)
    z2, r2 = P.z_ref(n - 1, step, seed)
    assert np.array_equal(z2, z[:n - 1]) and np.array_equal(r2, r[:n - 1])
    # each Box-Muller pair lies on its circle: z0^2 + z1^2 = r^2
    q = (n // 4) * 4
    zz, rr = z[:q].reshape(-1, 4), r[:q].reshape(-1, 4)
    assert np.allclose(zz[:, 0] ** 2 + zz[:, 1] ** 2, rr[:, 0] ** 2, rtol=1e-12, atol=1e-300)
    assert np.allclose(zz[:, 2] ** 2 + zz[:, 3] ** 2, rr[:, 2] ** 2, rtol=1e-12, atol=1e-300)
    assert abs(z.mean()) < 0.15 and abs(z.var() - 1) < 0.2
    # the pixel normals use the same words one counter per pixel: with the z tensor id they are the first three of each z quad, up to
    # the float32 rounding of z's angle (2 pi u rounded to float32: <= 2^-22 rad)
    px, pr = P.pixel_normals_ref(n // 4, P.TENSOR_Z, step, seed)
    assert np.allclose(pr, rr[:, :3], rtol=1e-14)
    assert np.abs(px - zz[:, :3]).max() < 2.0 ** -21 * rr.max()
    # `first` offsets the pixel index
    a_, _ = P.pixel_normals_ref(10, 1, step, seed, first=2 ** 32 - 4)
    b_, _ = P.pixel_normals_ref(4, 1, step, seed, first=2 ** 32)
    assert np.array_equal(a_[4:8], b_)


def test_u_equal_one_gives_radius_zero():
    z, r = P.box_muller_z(np.array([[0xffffffff], [12345], [0xffffff00], [1 << 31]], dtype=np.uint32))
    assert r[0, 0] == 0.0 and z[0, 0] == 0.0 and z[1, 0] == 0.0 and r[2, 0] == 0.0 and z[3, 0] == 0.0
