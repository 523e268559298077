"""lap_amd/sampling.py, the host restatement of the device sampler's noise (no GPU)."""
import numpy as np
import pytest

from lap_amd import sampling as S

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def _philox_scalar(ctr, key):
    """A second, independent restatement on Python integers."""
    c, k = [int(x) for x in ctr], [int(x) for x in key]
    for r in range(10):
        hi0, lo0 = divmod(0xD2511F53 * c[0], 1 << 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c[2], 1 << 32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + 0x9E3779B9) % (1 << 32), (k[1] + 0xBB67AE85) % (1 << 32)]
    return tuple(c)


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = S.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
        assert _philox_scalar(ctr, key) == want


def test_philox_agrees_with_second_restatement():
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, size=(1000, 2), dtype=np.uint64).astype(np.uint32)
    got = S.philox4x32_10(ctr, key)
    for i in range(1000):
        assert tuple(int(x) for x in got[i]) == _philox_scalar(ctr[i], key[i]), i


def test_gumbel_noise_is_a_pure_function_of_its_arguments():
    a = S.gumbel_noise(1234567890123, 3, 4, 1001)
    assert a.shape == (4, 1001) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a, S.gumbel_noise(1234567890123, 3, 4, 1001))
    assert not np.array_equal(a, S.gumbel_noise(1234567890124, 3, 4, 1001))              # low seed word
    assert not np.array_equal(a, S.gumbel_noise(1234567890123 + (1 << 32), 3, 4, 1001))  # high seed word
    assert not np.array_equal(a, S.gumbel_noise(1234567890123, 4, 4, 1001))
    assert all(not np.array_equal(a[0], a[b]) for b in range(1, 4))
    # the rows of a smaller call are the rows of a larger one; a shorter vocabulary is a prefix
    assert np.array_equal(S.gumbel_noise(1234567890123, 3, 2, 1001), a[:2])
    assert np.array_equal(S.gumbel_noise(1234567890123, 3, 4, 1000), a[:, :1000])
    # the definition, entry by entry: counter (j >> 1, b, t, 0), word j & 1
    for b, j in ((0, 0), (1, 1), (3, 1000), (2, 517)):
        w = _philox_scalar((j >> 1, b, 3, 0), (1234567890123 & 0xFFFFFFFF, 1234567890123 >> 32))[j & 1]
        assert a[b, j] == S.gumbel_from_word(np.uint32(w))


def test_extreme_words_stay_inside_the_open_interval():
    u = S.uniform_from_word(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32
    assert 0.0 < float(u[0]) == 2.0 ** -24 and float(u[1]) == 1.0 - 2.0 ** -24 < 1.0
    g = S.gumbel_from_word(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert np.isfinite(g).all() and -2.82 < float(g[0]) < -2.80 and 16.6 < float(g[1]) < 16.7
    # exact in float32: every word's u is ((word >> 9) + 0.5) / 2^23 in exact arithmetic
    w = np.random.default_rng(3).integers(0, 1 << 32, size=4096, dtype=np.uint64)
    assert np.array_equal(S.uniform_from_word(w.astype(np.uint32)).astype(np.float64), ((w >> np.uint64(9)).astype(np.float64) + 0.5) / 2.0 ** 23)


def test_temperature_rules():
    assert S.inverse_temperature(0.0) == 0.0 and S.inverse_temperature(-1.0) == 0.0
    assert S.inverse_temperature(0.7) == np.float32(1.0 / 0.7)
    for bad in (1e-45, float("nan")):
        with pytest.raises(ValueError):
            S.inverse_temperature(bad)
    lg = np.random.default_rng(5).standard_normal((3, 50)).astype(np.float32)
    lg[1, 7] = lg[1, 31] = 9.0          # greedy: the lowest index among ties
    assert np.array_equal(S.sample_from_logits(lg, 0.0, 11, 2), np.argmax(lg, -1))
    assert int(S.sample_from_logits(lg, -2.0, 11, 2)[1]) == 7


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_sample_from_logits_follows_the_softmax(T):
    """20,000 fixed (seed, step) pairs on an 8-entry distribution: chi-square against softmax(logits / T) below the 99.9 %
    quantile of 7 degrees of freedom (24.32)."""
    logits = np.array([[1.2, -0.3, 0.0, 2.1, 0.7, -1.5, 1.9, 0.4]], dtype=np.float32)
    n = 20000
    counts = np.zeros(8)
    for i in range(n):
        counts[int(S.sample_from_logits(logits, T, 1000 + i // 50, i % 50)[0])] += 1
    z = logits[0].astype(np.float64) / T
    p = np.exp(z - z.max())
    p /= p.sum()
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    print(f"T {T}: chi-square {chi2:.2f}")
    assert chi2 < 24.32


def test_server_flags_map_to_sample_kwargs():
    """--ar-temperature / --ar-sampler of `python -m lap_amd.serve_ws`: nothing at their defaults (the server as it was)."""
    from lap_amd.serve_ws import _ar_sample_kwargs

    assert _ar_sample_kwargs(0.0, "host") == {}
    assert _ar_sample_kwargs(0.7, "host") == {"sample_kwargs": {"temperature": 0.7}}
    assert _ar_sample_kwargs(0.7, "device") == {"sample_kwargs": {"temperature": 0.7, "sampler": "device"}}
    assert _ar_sample_kwargs(0.0, "device") == {"sample_kwargs": {"sampler": "device"}}
