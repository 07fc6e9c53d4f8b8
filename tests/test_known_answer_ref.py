"""The known-answer helpers (tests/known_answer.py) against the oracle, on the
CPU: what tests/test_gpu_tap_domain.py and tests/test_gpu_plan_limits.py (the
shortest, the longest one-partition, the first two-partition and the longest
filters of the FFT method) expect of the kernels is what the
long-double oracle computes bit for bit, and what an f64 FFT convolution
narrows to; the threshold taps sit on the side of 2^-50 they claim; the
partition edges are fft_partition_taps' (fir_fft.hpp)."""
import numpy as np
import pytest

import known_answer as ka

N = 20_001
# 1, 3, 5: the shortest filters of tests/test_gpu_plan_limits.py (half 0, 1, 2)
TAPS = [1, 3, 5, 15, 801, 4001, 4003]
# its long tap counts, with the partitions they run in (fft_partition_count at L = 16 384 / 32 768):
# checked at sampled outputs
LIMIT_TAPS = [(10_921, 1), (10_923, 1), (10_925, 2), (21_845, 1), (21_847, 1), (21_849, 2)]
T_MAX = 1_048_575  # the FFT method's longest filter: 127 partitions at L = 16 384, 64 at 32 768


@pytest.fixture(scope="module")
def x():
    return ka.grid16(np.random.default_rng(16), 1, N)[0]


def _cases(T):
    """(name, taps, expected) builders of every delay and pair the GPU tests use at T taps."""
    ks = sorted(set(ka.delay_ks(T)) | set(ka.direct_ks(T)))
    return [(f"delay k={k}", ka.delay_taps(T, k), lambda x, k=k: ka.expect_delay(x, T, k)) for k in ks] + \
           [(f"pair d={d}", ka.pair_taps(T, d), lambda x, d=d: ka.expect_pair(x, T, d)) for d in ka.pair_ds(T)]


def test_grid16_is_the_16_bit_grid_without_zero():
    g = ka.grid16(np.random.default_rng(1), 3, 50_000)
    m = g.astype(np.float64) * 32768.0
    assert g.dtype == np.float32 and g.shape == (3, 50_000)
    assert np.array_equal(m, np.rint(m)) and np.abs(m).min() == 1 and np.abs(m).max() == 32767
    assert (m > 0).any() and (m < 0).any() and not np.array_equal(g[0], g[1])


def test_expected_arrays_follow_the_definition():
    """expect_* against the header's sum written out, zero padding included."""
    x = ka.grid16(np.random.default_rng(2), 1, 40)[0]
    for T in (1, 3, 15):
        half = (T - 1) // 2
        for name, taps, expect in _cases(T):
            want = np.zeros(x.size)
            for n in range(x.size):
                for k in range(T):
                    i = n - half + k
                    if 0 <= i < x.size:
                        want[n] += taps[k] * float(x[i])
            assert np.array_equal(expect(x).astype(np.float64), want), (T, name)


@pytest.mark.parametrize("T", TAPS)
def test_oracle_reproduces_expected_bits(oracle_mod, x, T):
    for name, taps, expect in _cases(T):
        want = expect(x)
        got = oracle_mod.filter_channel_mt(x, taps, 16, oracle_mod.MODE_LD)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (T, name)
        ka.assert_known(got, want, exact_zero=True, where=f"T={T} {name}")
        assert np.count_nonzero(want) > N // 4, (T, name)  # the shift leaves outputs to check


@pytest.mark.parametrize("T", TAPS)
def test_f64_fft_convolution_narrows_to_expected_bits(x, T):
    """A numpy f64 FFT convolution, the stand-in for the kernels' arithmetic:
    bit-exact wherever the expected output is not 0, within 1e-12 where it is."""
    half = (T - 1) // 2
    nfft = 1 << int(np.ceil(np.log2(N + T)))
    X = np.fft.rfft(x.astype(np.float64), nfft)
    worst = 0.0
    for name, taps, expect in _cases(T):
        want = expect(x)
        # y[n] = sum_k h[k] x[n - half + k]: the convolution with the reversed taps, read from half on
        y64 = np.fft.irfft(X * np.fft.rfft(taps[::-1], nfft), nfft)[half:half + N]
        err = float(np.abs(y64 - want.astype(np.float64)).max())
        worst = max(worst, err)
        got = y64.astype(np.float32)
        nz = want != 0
        assert np.array_equal(got[nz].view(np.int32), want[nz].view(np.int32)), f"T={T} {name}: max error {err:.3e}"
        assert np.all(np.abs(y64[~nz]) <= ka.ZERO_FLOOR), f"T={T} {name}: max error {err:.3e}"
        ka.assert_known(got, want, exact_zero=False, where=f"T={T} {name}")
    assert worst <= 9.1e-13 / 100, f"T={T}: f64 FFT max error {worst:.3e} against the 9.1e-13 half-spacing"


def _limit_cases(T, parts):
    """The delays and pairs test_gpu_plan_limits.py runs at T taps in `parts` partitions."""
    ks = ka.delay_ks(T, ka.partition_edges(T, ka.partition_taps(T, parts), parts))
    return [(f"delay k={k}", ka.delay_taps(T, k), lambda x, k=k: ka.expect_delay(x, T, k)) for k in ks] + \
           [(f"pair d={d}", ka.pair_taps(T, d), lambda x, d=d: ka.expect_pair(x, T, d)) for d in ka.pair_ds(T)]


def _sampled(n, half, count, seed):
    """Both ends, either side of the first and last full-length sum, random positions."""
    idx = np.r_[np.arange(8), np.arange(n - 8, n), half + np.arange(-2, 3), n - 1 - half + np.arange(-2, 3),
                np.random.default_rng(seed).integers(0, n, count)]
    return np.unique(idx[(idx >= 0) & (idx < n)])


@pytest.mark.parametrize("T,parts", LIMIT_TAPS)
def test_oracle_reproduces_expected_bits_at_the_plan_limits(oracle_mod, T, parts):
    """The long tap counts of test_gpu_plan_limits.py, at ~550 sampled outputs of a 60 001-sample channel."""
    n = 60_001
    x = ka.grid16(np.random.default_rng(T), 1, n)[0]
    idx = _sampled(n, (T - 1) // 2, 512, T)
    cases = _limit_cases(T, parts)
    # 7 delays (two partitions meet at the centre tap: their edges are half and half + 1) and 4 pairs
    assert len(cases) == 11 and (parts == 1 or ka.partition_taps(T, 2) == (T - 1) // 2 + 1)
    for name, taps, expect in cases:
        want = expect(x)
        got, _ = oracle_mod.filter_points(x, taps, idx, oracle_mod.MODE_LD)
        assert np.array_equal(got.view(np.int32), want[idx].view(np.int32)), (T, name)
        assert np.count_nonzero(want) > n // 4 and np.count_nonzero(want[idx]) > idx.size // 4, (T, name)


@pytest.mark.parametrize("T,parts", LIMIT_TAPS)
def test_f64_fft_convolution_narrows_at_the_plan_limits(T, parts):
    """test_f64_fft_convolution_narrows_to_expected_bits at the long tap counts, every output."""
    n = 60_001
    x = ka.grid16(np.random.default_rng(T), 1, n)[0]
    half = (T - 1) // 2
    nfft = 1 << 17
    assert nfft >= n + T
    X = np.fft.rfft(x.astype(np.float64), nfft)
    worst = 0.0
    for name, taps, expect in _limit_cases(T, parts):
        want = expect(x)
        y64 = np.fft.irfft(X * np.fft.rfft(taps[::-1], nfft), nfft)[half:half + n]
        worst = max(worst, float(np.abs(y64 - want.astype(np.float64)).max()))
        ka.assert_known(y64.astype(np.float32), want, exact_zero=False, where=f"T={T} {name}")
    assert worst <= 9.1e-13 / 100, f"T={T}: f64 FFT max error {worst:.3e} against the 9.1e-13 half-spacing"


@pytest.mark.parametrize("tp", [8257, 16385])
def test_oracle_reproduces_expected_bits_of_the_longest_filter(oracle_mod, tp):
    """1 048 575 taps: the three delays test_gpu_plan_limits.py runs per segment
    length (k = 0, T - 1 and 63 tp), at ~150 sampled outputs of a channel of
    the length that test uses."""
    T = T_MAX
    half = (T - 1) // 2
    n = T + ((16384 if tp == 8257 else 32768) - tp + 1) // 2  # T + B // 2
    x = ka.grid16(np.random.default_rng(n), 1, n)[0]
    idx = _sampled(n, half, 128, tp)
    for k in (0, T - 1, 63 * tp):
        want = ka.expect_delay(x, T, k)
        got, _ = oracle_mod.filter_points(x, ka.delay_taps(T, k), idx, oracle_mod.MODE_LD)
        assert np.array_equal(got.view(np.int32), want[idx].view(np.int32)), (T, k)
        assert np.count_nonzero(want) > n // 4 and np.count_nonzero(want[idx]) > idx.size // 4, (T, k)


def test_assert_known_sees_one_wrong_output():
    x = ka.grid16(np.random.default_rng(3), 2, 1000)
    want = ka.expect_delay(x, 15, 0)  # y[n] = x[n - 7]: the first 7 outputs of each channel are 0
    assert not want[:, :7].any() and want[:, 7:].all()
    ka.assert_known(want.copy(), want, exact_zero=True)
    for at, value, exact_zero in [((1, 500), np.nextafter(want[1, 500], np.float32(2)), False),
                                  ((0, 999), np.float32(0), False), ((1, 0), np.float32(1e-13), True),
                                  ((1, 6), np.float32(2e-12), False), ((0, 3), np.float32(np.nan), False),
                                  ((0, 998), np.float32(np.nan), False)]:
        y = want.copy()
        y[at] = value
        with pytest.raises(AssertionError, match="1 of 2000 outputs differ"):
            ka.assert_known(y, want, exact_zero=exact_zero)
    y = want.copy()
    y[1, 6] = 1e-13
    ka.assert_known(y, want, exact_zero=False)  # under the floor
    y[1, 6] = -0.0
    ka.assert_known(y, want, exact_zero=True)


def test_tap_families():
    for T in (15, 4003, 40001):
        half = (T - 1) // 2
        h = ka.antisym_taps(T)
        assert np.array_equal(h, -h[::-1]) and h[half] == 0.0 and h[half + 1] > 0.3
        anti, norm = ka.sym_ratio(h)
        assert anti == norm > 0  # all of it antisymmetric
        g = ka.one_sided_taps(T)
        assert g[0] == 1.0 and abs(g[-1] / 1e-12 - 1.0) < 1e-9 and np.all(np.diff(g) < 0)
        assert np.allclose(g[1:] / g[:-1], g[1], rtol=1e-12)


@pytest.mark.parametrize("T", [15, 4001])
def test_threshold_taps_sit_on_the_requested_side(oracle_mod, T):
    """fft_sym_eligible's rule (anti <= norm * 2^-50 in long double), recomputed."""
    sym = oracle_mod.design_lowcut(20.0, 48000.0, T)
    sym = 0.5 * (sym + sym[::-1])
    edge = np.longdouble(2.0) ** -50
    anti, norm = ka.sym_ratio(sym)
    assert anti == 0 and norm > 0
    for exp, eligible in [(-52, True), (-51, True), (-49, False), (-48, False)]:
        h = ka.threshold_taps(sym, 2.0 ** exp)
        assert np.count_nonzero(h != sym) == 1 and h[(T - 1) // 2] == sym[(T - 1) // 2]
        anti, norm = ka.sym_ratio(h)
        assert (anti <= norm * edge) == eligible, (exp, float(anti / norm))
        # delta survives the f64 sum: the ratio is the requested one to 1e-3
        assert abs(float(anti / norm) / 2.0 ** exp - 1.0) < 1e-3, (exp, float(anti / norm))


@pytest.mark.parametrize("T,parts,tp,edges", [
    (40_001, 5, 8001, [0, 8000, 8001, 16001, 16002, 24002, 24003, 32003, 32004, 40_000]),
    (100_001, 6, 16667, [0, 16666, 16667, 33333, 33334, 50000, 50001, 66667, 66668, 83334, 83335, 100_000]),
    # tests/test_gpu_plan_limits.py: the first two-partition plan of either segment length ...
    (10_925, 2, 5463, [0, 5462, 5463, 10_924]),
    (21_849, 2, 10_925, [0, 10_924, 10_925, 21_848]),
    # ... and the longest filter at either segment length (64 / 65 zero taps behind the last partition)
    (1_048_575, 127, 8257, sorted({0, 1_048_574} | {8257 * p - 1 for p in range(1, 127)} |
                                  {8257 * p for p in range(1, 127)})),
    (1_048_575, 64, 16_385, sorted({0, 1_048_574} | {16_385 * p - 1 for p in range(1, 64)} |
                                   {16_385 * p for p in range(1, 64)}))])
def test_partition_edges_restated(T, parts, tp, edges):
    """fft_partition_taps = ceil(T / parts) | 1, written out for both
    partitioned forms; the last partition is the short one."""
    assert ka.partition_taps(T, parts) == tp and tp % 2 == 1
    assert (parts - 1) * tp < T <= parts * tp
    assert ka.partition_edges(T, tp, parts) == edges
    assert ka.partition_taps(4001, 1) == 4001 and ka.partition_edges(4001, 4001, 1) == [0, 4000]
