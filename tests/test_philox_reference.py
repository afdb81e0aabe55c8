"""The host Philox / Box-Muller reference of tests/_philox.py, checked on the CPU: the Random123 known-answer
vectors, the counter / key mapping of the stream, and that the inverse recovers every word with a wide margin
(which is what lets tests/test_gpu_rng_builders.py compare the device stream bit for bit)."""
import numpy as np
import pytest

from tests import _philox as P

# Random123 kat_vectors, philox4x32 10: counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = P.philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [hex(int(w)) for w in got] == [hex(w) for w in want]


def test_known_answers_need_all_ten_rounds_and_vectorise():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64)
    key = np.array([k[1] for k in KAT], dtype=np.uint64)
    want = np.array([k[2] for k in KAT], dtype=np.uint64)
    assert np.array_equal(P.philox4x32(ctr, key), want)                 # one key per row
    for rounds in (7, 9, 11):
        assert not np.any(P.philox4x32(ctr, key, rounds=rounds) == want)


def test_stream_mapping_is_counter_t_base_and_key_seed():
    seed, counter, offset = 0x1234567890ABCDEF, 7 * 2 ** 32 + 5, 2 ** 33 + 9
    w = P.stream_words(4 * 5 + 1, seed, counter, offset)
    assert w.shape == (6, 4)
    base = counter + offset
    for t in (0, 1, 5):
        one = P.philox4x32(np.array([t, 0, base & 0xFFFFFFFF, base >> 32], dtype=np.uint64),
                           np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
        assert np.array_equal(w[t], one)
    assert np.array_equal(w, P.stream_words(21, seed, counter + offset, 0))
    assert np.array_equal(w[:2], P.stream_words(5, seed, base))         # a shorter stream is a prefix
    assert np.array_equal(P.stream_words(8, seed, 2 ** 64 - 1, 1), P.stream_words(8, seed, 0))   # base wraps
    other = np.concatenate([P.stream_words(21, seed, base + 1), P.stream_words(21, seed + 1, base),
                            P.stream_words(21, seed + 2 ** 32, base), P.stream_words(21, seed, base + 2 ** 32)])
    assert not (other[:, None, :] == w[None, :, :]).all(-1).any()       # no quad in common
    z = P.normals(21, seed, counter, offset)
    assert z.shape == (21,) and np.array_equal(z, P.normals_from_words(w).reshape(-1)[:21])


def test_box_muller_layout_and_moments():
    w = np.array([[0, 0, 2 ** 32 - 1, 2 ** 31]], dtype=np.uint64)
    z = P.normals_from_words(w)[0]
    r0 = np.sqrt(-2 * np.log(0.5 * 2.0 ** -32))                          # the largest radius: 6.76
    assert z[0] == pytest.approx(r0, rel=1e-15) and 6.7 < r0 < 6.8
    assert abs(z[1]) < 1e-8 and abs(z[2]) < 2e-5 and abs(z[3]) < 2e-5
    x = P.normals(1 << 18, 1234)
    assert abs(x.mean()) < 1e-2 and abs(x.std() - 1) < 1e-2
    assert abs(np.mean(x ** 3)) < 3e-2 and abs(np.mean(x ** 4) - 3) < 6e-2
    q = x.reshape(-1, 4)                                                  # no pair shares a uniform
    c = np.corrcoef(q.T)
    assert np.abs(c - np.eye(4)).max() < 1e-2
    assert abs(np.corrcoef(q[:, 0] ** 2 + q[:, 1] ** 2, q[:, 2] ** 2 + q[:, 3] ** 2)[0, 1]) < 1e-2


def test_inverse_recovers_every_word_under_libm_sized_perturbation():
    n = 1 << 20
    words = P.stream_words(n, 99, 3)
    z = P.normals_from_words(words).reshape(-1)
    back, dist = P.words_from_normals(z, return_distance=True)
    assert np.array_equal(back, words) and dist < 0.01
    g = np.random.default_rng(0)
    worst = dist
    for ulps in (64, -64, None):
        k = g.integers(-64, 65, n) if ulps is None else np.full(n, ulps)
        zp = (z.view(np.int64) + k).view(np.float64)                      # +-64 ulp, a stand-in for device libm
        assert np.abs(zp - z).max() <= 64 * np.spacing(6.7)
        back, dist = P.words_from_normals(zp, return_distance=True)
        worst = max(worst, dist)
        assert np.array_equal(back, words)
    print(f"worst distance from an integer: {worst:.3e}")
    assert worst < 0.01
    # and a flipped word is seen: one quad of another stream
    z2 = z.copy()
    z2[4:8] = P.normals(8, 100, 3)[4:8]
    assert (P.words_from_normals(z2) != words).any(-1).sum() == 1
