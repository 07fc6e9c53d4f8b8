"""Known-answer taps and tap families (test infrastructure: inputs and exact
expected outputs for tests/test_known_answer_ref.py,
tests/test_gpu_tap_domain.py and tests/test_gpu_plan_limits.py).

The filtered sample (include/lcfir.h): y[n] = sum_k h[k] x[n - half + k], half =
(T - 1) / 2, x = 0 outside [0, N).  Sparse taps make that sum one or two
terms, so the expected output needs no oracle:
  * a delay, h = e_k:                    y[n] = x[n + k - half];
  * a pair, h[half - d] = h[half + d] = 0.5: y[n] = (x[n - d] + x[n + d]) / 2
    (d = 0: the identity).
On the 16-bit grid (x = m / 32768, m != 0) both are exact f32 values and a
non-zero one is at least 2^-16 in magnitude, where f32 values are 2^-39 apart
(half: 9.1e-13; 2^-40 just below the power of two itself, half 4.5e-13).  An
f64 FFT's error is 2^-50 |h|_1 max|x| ~ 1e-15, hundreds of times smaller, so
every method must narrow to the expected bits.
"""
import numpy as np

ZERO_FLOOR = 1e-12  # the suite's floor under the ulp count (test_gpu_parity.max_ulps)
PAIR_DS = (0, 1, 2047)  # and half: pair_ds


def grid16(rng, nch, n):
    """[nch][n] float32 samples m / 32768, m uniform in +-[1, 32767], never 0."""
    m = rng.integers(1, 32768, size=(nch, n)) * rng.choice(np.array([-1, 1]), size=(nch, n))
    return (m / 32768.0).astype(np.float32)


def _shifted(x, s):
    """z[..., n] = x[..., n + s], zeros where n + s is outside [0, N)."""
    x = np.asarray(x)
    n = x.shape[-1]
    z = np.zeros_like(x)
    if s >= 0:
        if s < n:
            z[..., :n - s] = x[..., s:]
    elif -s < n:
        z[..., -s:] = x[..., :n + s]
    return z


def delay_taps(T, k):
    assert T % 2 == 1 and 0 <= k < T
    h = np.zeros(T)
    h[k] = 1.0
    return h


def expect_delay(x, T, k):
    assert x.dtype == np.float32
    return _shifted(x, k - (T - 1) // 2)


def pair_taps(T, d):
    half = (T - 1) // 2
    assert T % 2 == 1 and 0 <= d <= half
    h = np.zeros(T)
    h[half - d] += 0.5
    h[half + d] += 0.5
    return h


def expect_pair(x, T, d):
    """In f64, then cast: (m1 + m2) / 65536 has 17 bits, so the value is exact."""
    assert x.dtype == np.float32 and 0 <= d <= (T - 1) // 2
    x64 = x.astype(np.float64)
    y = 0.5 * _shifted(x64, -d) + 0.5 * _shifted(x64, d)
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    return y32


def delay_ks(T, extra=()):
    """The delays every form runs: both ends, the centre and its neighbours,
    plus `extra` (partition edges)."""
    half = (T - 1) // 2
    ks = {0, 1, half - 1, half, half + 1, T - 2, T - 1} | set(extra)
    return sorted(k for k in ks if 0 <= k < T)


def pair_ds(T):
    half = (T - 1) // 2
    return sorted(d for d in set(PAIR_DS) | {half} if d <= half)


def direct_ks(T):
    """Delays of the direct kernel's cases: the ends, both sides of its
    256-tap stage boundary and of the last whole 16-tap block."""
    b = 16 * (T // 16)
    return sorted(k for k in {0, T - 1, T - 2, 255, 256, b - 1, b} if 0 <= k < T)


def partition_taps(T, parts):
    """fft_partition_taps (fir_fft.hpp): ceil(T / parts) | 1."""
    return T if parts == 1 else (-(-T // parts)) | 1


def partition_edges(T, tp, parts):
    """The first and last tap of the filter and of every partition of tp taps."""
    e = {0, T - 1}
    for p in range(1, parts):
        e |= {p * tp - 1, p * tp}
    return sorted(k for k in e if 0 <= k < T)


def assert_known(y, want, exact_zero, where=""):
    """Every output of y against the exact expected array: the same bits
    wherever want != 0; where want == 0, y == 0 (exact_zero: the direct
    method) or |y| <= 1e-12.  The message lists the first failing (channel,
    index) pairs with the values."""
    y = np.asarray(y)
    want = np.asarray(want)
    assert y.dtype == np.float32 and want.dtype == np.float32 and y.shape == want.shape, (y.dtype, y.shape, want.shape)
    nz = want != 0
    bad = nz & (y.view(np.int32) != want.view(np.int32))
    if exact_zero:
        bad |= ~nz & ~(y == 0)
    else:
        bad |= ~nz & ~(np.abs(y.astype(np.float64)) <= ZERO_FLOOR)
    if bad.any():
        at = np.argwhere(bad)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        worst = float(np.nanmax(np.where(bad, err, 0.0)))
        first = [(tuple(int(v) for v in i), float(y[tuple(i)]), float(want[tuple(i)])) for i in at[:8]]
        raise AssertionError(f"{where}: {at.shape[0]} of {y.size} outputs differ, max |y - want| = {worst:.3e} "
                             f"(half-spacing 9.1e-13); first (index, got, want): {first}")


# ---- tap families -----------------------------------------------------------------
def blackman(T):
    if T == 1:
        return np.ones(1)
    k = np.arange(T)
    return 0.42 - 0.5 * np.cos(2 * np.pi * k / (T - 1)) + 0.08 * np.cos(4 * np.pi * k / (T - 1))


def antisym_taps(T):
    """Blackman-windowed Hilbert transformer (type III): 2 / (pi m) at odd m =
    k - half, 0 at even m; h[k] = -h[T - 1 - k] exactly (the upper half is
    computed, the lower is its negated mirror) and h[half] = 0."""
    half = (T - 1) // 2
    assert T % 2 == 1 and T >= 3
    m = np.arange(1, half + 1)
    upper = np.where(m % 2 == 1, 2.0 / (np.pi * m), 0.0) * blackman(T)[half + 1:]
    h = np.zeros(T)
    h[half + 1:] = upper
    h[:half] = -upper[::-1]
    return h


def one_sided_taps(T):
    """h[k] = r^k from h[0] = 1 down to h[T - 1] = 1e-12: nothing like a symmetry."""
    assert T % 2 == 1 and T >= 3
    return np.exp(np.arange(T) * (np.log(1e-12) / (T - 1)))


def threshold_taps(sym, ratio):
    """Symmetric taps plus delta = ratio |sym|_1 on the off-centre tap of
    smallest magnitude (so the sum keeps delta's bits): the antisymmetric l1
    part, sum |h[k] - h[T-1-k]| / 2, is delta."""
    sym = np.asarray(sym, np.float64)
    T = sym.size
    half = (T - 1) // 2
    assert np.array_equal(sym, sym[::-1]) and half >= 1
    j = int(np.argmin(np.abs(sym[:half])))
    h = sym.copy()
    h[j] += ratio * np.abs(sym).sum()
    return h


def sym_ratio(h):
    """fft_sym_eligible's quantities (fir_fft.hpp) in numpy.longdouble:
    (antisymmetric l1 part, l1 norm)."""
    h = np.asarray(h, np.longdouble)
    return np.abs((h - h[::-1]) * np.longdouble(0.5)).sum(), np.abs(h).sum()
