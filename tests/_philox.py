"""Host restatement of the device noise generator (csrc/dsvi.hip: philox_round, normal_quad) in numpy
``uint64`` arithmetic, and its inverse (test infrastructure; tests/test_philox_reference.py pins it to the
Random123 known-answer vectors on the CPU, tests/test_gpu_rng_builders.py pins the kernels to it)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # Philox4x32 multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)      # key bumps (golden ratio, sqrt(3) - 1)
ROUNDS = 10
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
TWO_PI = 6.283185307179586
_U64 = (1 << 64) - 1


def philox4x32(ctr, key, rounds=ROUNDS):
    """Philox4x32-``rounds``: ``ctr`` (..., 4) and ``key`` (..., 2) hold 32-bit words; returns (..., 4) uint64
    words < 2^32.  Every product is a 32 x 32 -> 64 bit one, so uint64 never wraps."""
    c = np.asarray(ctr, dtype=np.uint64) & _LO
    k = np.asarray(key, dtype=np.uint64) & _LO
    c0, c1, c2, c3 = (c[..., q].copy() for q in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        h0, l0 = p0 >> _S32, p0 & _LO
        h1, l1 = p1 >> _S32, p1 & _LO
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + W0) & _LO, (k1 + W1) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def stream_words(n, seed, counter=0, offset=0):
    """The (ceil(n / 4), 4) Philox words behind elements 0 .. n-1 of the device stream: quad t uses counter
    words (t_lo, t_hi, base_lo, base_hi), base = counter + offset (mod 2^64), and key (seed_lo, seed_hi)."""
    nq = (int(n) + 3) // 4
    base = (int(counter) + int(offset)) & _U64
    seed = int(seed) & _U64
    t = np.arange(nq, dtype=np.uint64)
    ctr = np.empty((nq, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = t & _LO, t >> _S32
    ctr[:, 2], ctr[:, 3] = base & 0xFFFFFFFF, base >> 32
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32(ctr, key)


def normals_from_words(words):
    """Box-Muller as normal_quad: u_q = (c_q + 0.5) 2^-32, z = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3,
    r1 sin 2 pi u3), r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2); (nq, 4) words -> (nq, 4) float64."""
    u = (np.asarray(words, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = TWO_PI * u[:, 1], TWO_PI * u[:, 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def normals(n, seed, counter=0, offset=0):
    """Float64 elements 0 .. n-1 of the stream (element 4t + q is value q of quad t)."""
    return normals_from_words(stream_words(n, seed, counter, offset)).reshape(-1)[:int(n)]


def unit_from_normals(z):
    """Per pair (a, b) of ``z`` (length a multiple of 4): u0 = exp(-(a^2 + b^2) / 2), u1 = atan2(b, a) / 2 pi mod 1,
    as the real numbers u 2^32 - 0.5 whose nearest integers are the Philox words; (nq, 4) float64."""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    a, b = z[:, 0], z[:, 1]
    u_r = np.exp(-0.5 * (a * a + b * b))
    u_a = np.mod(np.arctan2(b, a) / TWO_PI, 1.0)
    return (np.stack([u_r, u_a], axis=-1) * 2.0 ** 32 - 0.5).reshape(-1, 4)


def words_from_normals(z, return_distance=False):
    """Inverse of normals_from_words: c = rint(u 2^32 - 0.5), (nq, 4) uint64.  With ``return_distance`` also
    the largest |u 2^32 - 0.5 - c| (0.5 would flip a word).  The angle word wraps modulo 2^32: an angle just
    below 2 pi may come out as u1 = 1 - tiny."""
    x = unit_from_normals(z)
    r = np.rint(x)
    w = np.mod(r, 2.0 ** 32).astype(np.uint64)
    if return_distance:
        return w, float(np.abs(x - r).max()) if x.size else 0.0
    return w
