"""
Plain-Python references for the bootstrap entries (include/mixemt_hip_bootstrap.h), shared by test_bootstrap_host.py and
test_gpu_bootstrap.py: Philox4x64-10, the multinomial draw rule of mxm_bootstrap_weights, and the quantile formula of
mxm_bootstrap_summary.  Nothing here touches the device or the library.
"""
import numpy

MASK = (1 << 64) - 1
M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def philox4x64(counter, key, rounds=10):
    """The four output words of Philox4x64 (Salmon et al., Random123) for a 4-word counter and a 2-word key."""
    x0, x1, x2, x3 = [int(v) & MASK for v in counter]
    k0, k1 = [int(v) & MASK for v in key]
    for _ in range(rounds):
        p0, p1 = M0 * x0, M1 * x2
        x0, x1, x2, x3 = (p1 >> 64) ^ x1 ^ k0, p1 & MASK, (p0 >> 64) ^ x3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x0, x1, x2, x3]


def stream(seed, s_id, b, n):
    """The n words replicate b of sample s_id draws from: word j mod 4 of counter (j / 4 + 1, b, s_id, 0), key (seed, 0)."""
    out = []
    for block in range((n + 3) // 4):
        out.extend(philox4x64([block + 1, b, s_id, 0], [seed, 0]))
    return out[:n]


def numpy_stream(seed, s_id, b, n):
    """The same words from numpy's generator (it advances the counter BEFORE it generates a block)."""
    # (uint64 arrays: a LIST holding a value of 2^63 or more would go through float64 on its way in)
    gen = numpy.random.Philox(counter=numpy.array([0, b, s_id, 0], dtype=numpy.uint64), key=numpy.array([seed, 0], dtype=numpy.uint64))
    return [int(v) for v in gen.random_raw(n)] if n else []


def mulhi(words, total):
    """(u * total) >> 64 for uint64 words and 0 < total < 2^31, in uint64 arithmetic that cannot overflow: with
    u = hi * 2^32 + lo the product's upper half is (hi * total + ((lo * total) >> 32)) >> 32 (hi * total < 2^63, the rest < 2^31)."""
    u = numpy.asarray(words, dtype=numpy.uint64)
    n = numpy.uint64(total)
    hi, lo = u >> numpy.uint64(32), u & numpy.uint64(0xFFFFFFFF)
    return ((hi * n + ((lo * n) >> numpy.uint64(32))) >> numpy.uint64(32)).astype(numpy.int64)


def resample(w, seed, s_id, b, words=None):
    """Replicate b of one sample: the counts [R_s] as float64.  t = (u * N) >> 64; the row = the number of rows whose
    inclusive prefix sum of w is <= t.  words: the replicate's stream (default: numpy's generator, which
    test_bootstrap_host.py holds against the plain-Python Philox above)."""
    w = numpy.asarray(w, dtype=numpy.float64)
    cum = numpy.cumsum(w.astype(numpy.int64))
    total = int(cum[-1])
    if words is None:
        gen = numpy.random.Philox(counter=numpy.array([0, b, s_id, 0], dtype=numpy.uint64), key=numpy.array([seed, 0], dtype=numpy.uint64))
        words = gen.random_raw(total)
    rows = numpy.searchsorted(cum, mulhi(words, total), side="right")
    return numpy.bincount(rows, minlength=len(w)).astype(numpy.float64)


def resample_all(w, seed, s_id, n_boot):
    return numpy.stack([resample(w, seed, s_id, b) for b in range(n_boot)])


def quantile(sorted_x, q):
    """x_(i) + g (x_(i+1) - x_(i)) at h = q (B - 1), i = floor(h), g = h - i, the upper index clamped; every operation
    rounded on its own (numpy float64 scalars)."""
    n = len(sorted_x)
    h = numpy.float64(q) * numpy.float64(n - 1)
    fl = numpy.floor(h)
    i = int(fl)
    i1 = min(i + 1, n - 1)
    g = h - fl
    return numpy.float64(sorted_x[i]) + g * (numpy.float64(sorted_x[i1]) - numpy.float64(sorted_x[i]))
