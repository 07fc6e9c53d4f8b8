"""GPU value domain: non-finite, subnormal and power-of-two-scaled samples
through every kernel (a float32 source can hold any bit pattern).

The contract these tests pin (include/lcfir.h):
  * direct form: exact support.  Output n depends on x[n - half, n + half]
    alone, NaN and +-Inf included: `same()` as the oracle's strict-order fma
    chain (ORACLE_FMA) over whole channels, nothing else moves by a bit;
  * FFT forms: a non-finite sample makes the outputs of the segments whose
    input window holds it non-finite (at least every output whose support
    holds it), and changes nothing else: not the other segments, the other
    channels, their peaks, the buffer a fused normalize rescales, or the next
    call on the same ctx;
  * the peak is max |y| skipping NaN and taking Inf (oracle_max_mag's rule);
    a peak of Inf normalizes with gain 1 / Inf = 0 (finite -> 0, else NaN);
  * y(2^k x) = 2^k y(x) bit for bit wherever both sides are normal f32;
  * subnormal samples and outputs are honoured (no flush anywhere);
  * the f32 codec formats pass every bit pattern through, NaN payloads too.

`same(a, b)`: identical NaN masks and equal values elsewhere (Inf signs
included).  "Bit-identical" below is equality of the uint32 views.
"""
import numpy as np
import pytest

import pcm_ref
from test_gpu_parity import RMS_TOL, gpu_filter_channels, gpu_filter_window, max_ulps, rms

pytestmark = pytest.mark.gpu

FS = 48000.0
POISONS = {"nan": np.float32(np.nan), "pinf": np.float32(np.inf), "ninf": np.float32(-np.inf)}

# every FFT kernel and output form the suite distinguishes:
# name -> (taps, antisymmetric ramp, set_fft_tuning, family, kernel, one partition, zero phase)
FFT_FORMS = {
    "l16_zero_phase": (4001, 0.0, dict(seg_len=16384), "default", "l16", True, True),
    "l16_general": (4003, 0.0, dict(seg_len=16384, zero_phase=False), "default", "l16", True, False),
    "l16_two_parts": (19201, 0.0, dict(seg_len=16384), "default", "l16", False, None),
    "l32_reg": (4001, 0.0, dict(seg_len=32768), "default", "l32_reg", True, True),
    "l32_park": (4001, 0.0, dict(seg_len=32768), "lds", "l32_park", True, True),
    "l32_general": (8001, 1e-9, dict(seg_len=32768), "default", "l32_park", True, False),
    "l32_parts": (38401, 0.0, dict(seg_len=32768), "default", "l32_park", False, None),
}


@pytest.fixture(scope="module")
def lc():
    import lcfir
    assert lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


def same(a, b):
    """NaN masks identical, everything else equal (so Inf signs are checked)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bit_identical(a, b):
    return np.array_equal(bits(a), bits(b))


def same_bits(a, b):
    """same(), and the values that are not NaN agree bit for bit (-0.0, subnormals)."""
    nan = np.isnan(np.asarray(a, np.float32))
    return same(a, b) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def peak_rule(y):
    """oracle_max_mag: m = 0; a = |y[i]|; if (a > m) m = a -- NaN never wins, Inf does."""
    return np.fmax.reduce(np.abs(np.asarray(y, np.float32)).ravel(), initial=np.float32(0.0))


def int24_noise(rng, shape):
    return (rng.integers(-2**23, 2**23, size=shape) / 2.0**23).astype(np.float32)


def positions(n, half, B, nrand, seed):
    """Edge outputs, the outputs where the edge sums end, the direct form's
    tile seams, the FFT's segment seams and random positions."""
    rng = np.random.default_rng(seed)
    near = [0, half, n - 1 - half, n - 1, 4096, 8192] + ([B, 2 * B] if B else [])
    idx = np.r_[[np.arange(p - 24, p + 25) for p in near]].ravel()
    idx = np.r_[idx, rng.integers(0, n, nrand)]
    return np.unique(idx[(idx >= 0) & (idx < n)])


def make_fft(lc, oracle_mod, name):
    ntaps, ramp, tuning, family, kernel, one_part, zero_phase = FFT_FORMS[name]
    taps = oracle_mod.design_lowcut(20.0, FS, ntaps)
    if ramp:
        taps = taps + ramp * np.linspace(-1.0, 1.0, ntaps)  # antisymmetric part >> 2^-50 |h|_1
    flt = lc.Filter(taps, method="fft")
    flt.set_fft_tuning(**tuning)
    if family != "default":
        flt.set_fft_family(family)
    info, units = flt.fft_info, flt.fft_units
    assert info["seg_len"] == tuning["seg_len"] and units["kernel"] == kernel, (name, info, units)
    assert (info["parts"] == 1) == one_part, (name, info)
    if zero_phase is not None:
        assert info["zero_phase"] == zero_phase, (name, info)
    return flt, taps, units


def make_kernel(lc, oracle_mod, name):
    """An FFT form of FFT_FORMS or the 801-tap direct form: (filter, taps, B)."""
    if name == "direct":
        taps = oracle_mod.design_lowcut(20.0, FS, 801)
        return lc.Filter(taps, method="direct"), taps, 12_000
    flt, taps, units = make_fft(lc, oracle_mod, name)
    return flt, taps, units["outputs"]


# ---- 1. direct form: exact support of a non-finite sample --------------------
def direct_poison_sets(n, half):
    return [[0], [n - 1], [2000], [4095], [4096], [4096 + half + 1], [6000, 6005]]


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("ntaps", [15, 255, 97, 801])
def test_direct_exact_support(lc, oracle_mod, ntaps, poison):
    """One NaN / +Inf / -Inf sample (two, 5 apart) in channel 0 of 2, 10 001
    samples (more than two 4096-output tiles): channel 0 is same() as the
    oracle's fma chain over the whole channel -- the kernel rounds its last
    stage up to 16 taps (pad 1 at 15 and 255 taps, 15 at 97 and 801), and a
    zero tap times NaN or Inf is NaN, so the pad taps must never be multiplied
    (fir_direct.hpp fma_tail) -- channel 1 and its peak do not move, the fused
    peak skips NaN and takes Inf.  The same through filter_window_dev from the
    narrowest window and through apply_range_dev split at 4 096."""
    n = 10_001
    half = (ntaps - 1) // 2
    rng = np.random.default_rng(ntaps)
    x = int24_noise(rng, (2, n))
    taps = oracle_mod.design_lowcut(30.0, FS, ntaps)
    flt = lc.Filter(taps, method="direct")
    y_clean, pk_clean = gpu_filter_channels(lc, flt, x)
    assert bit_identical(y_clean[0], oracle_mod.filter_channel(x[0], taps, oracle_mod.MODE_FMA))
    for pos in direct_poison_sets(n, half):
        xp = x.copy()
        xp[0, pos] = POISONS[poison]
        ref = oracle_mod.filter_channel(xp[0], taps, oracle_mod.MODE_FMA)
        hit = ~np.isfinite(ref)
        support = np.zeros(n, bool)
        for p in pos:
            support[max(0, p - half):p + half + 1] = True
        assert np.array_equal(hit, support), pos  # the oracle: exactly the outputs whose taps reach it
        y, pk = gpu_filter_channels(lc, flt, xp)
        assert same(y[0], ref), (pos, np.nonzero(~(np.isnan(y[0]) == np.isnan(ref)))[0][:8])
        assert bit_identical(y[0][~hit], y_clean[0][~hit]), pos
        assert bit_identical(y[1], y_clean[1]) and pk[1] == pk_clean[1], pos
        for c in range(2):
            assert pk[c] == peak_rule(y[c]), (pos, c)
        # the outputs around the poison from the narrowest window that holds their support
        s, e = max(0, pos[0] - half - 40), min(n, pos[-1] + half + 41)
        x_lo, x_hi = max(0, s - half), min(n, e + half)
        dx = lc.DeviceBuffer.from_array(np.ascontiguousarray(xp[:, x_lo:x_hi]))
        dy = lc.DeviceBuffer(4 * 2 * (e - s))
        dpk = lc.DeviceBuffer(8)
        lc.peak_reset_dev(dpk, 2)
        flt.filter_window_dev(dx, x_lo, x_hi, x_hi - x_lo, n, 2, dy, s, e - s, s, e, dpk)
        lc.sync()
        yw, pkw = dy.download((2, e - s)), dpk.download(2)
        assert same(yw[0], ref[s:e]) and bit_identical(yw[1], y_clean[1][s:e]), pos
        assert pkw[0] == peak_rule(ref[s:e]) and pkw[1] == peak_rule(yw[1]), pos
        for b in (dx, dy, dpk):
            b.free()
        # two device ranges that meet at the first tile seam
        dx = lc.DeviceBuffer.from_array(xp[0])
        dy = lc.DeviceBuffer.from_array(np.zeros(n, np.float32))
        for s, e in [(0, 4096), (4096, n)]:
            flt.apply_range_dev(dx, n, dy, s, e)
        lc.sync()
        assert same(dy.download(n), ref), pos
        dx.free()
        dy.free()


def test_direct_finite_samples_overflow_to_inf(lc, oracle_mod):
    """Finite samples up to 3e38 whose outputs pass f32's range (noise at
    15 taps; at 801 a low-cut only gets there where a full-scale sample stands
    against a run of the opposite sign, so 2 000 samples are -2.7e38 .. -3e38
    with four +3e38 spikes, two of them at the tile seam; mirrored in channel
    1): the f64 chain stays finite and the narrowing gives +-Inf exactly where
    the oracle's does."""
    n = 10_001
    rng = np.random.default_rng(38)
    v = int24_noise(rng, (2, n)).astype(np.float64)
    v[:, 3000:5000] = -(0.9 + 0.1 * np.abs(v[:, 3000:5000]))
    v[:, [3500, 4095, 4096, 4600]] = 1.0
    v[1] = -v[1]
    x = (v * 3e38).astype(np.float32)
    assert np.isfinite(x).all() and np.abs(x).max() > 2.9e38
    for ntaps in (15, 801):
        taps = oracle_mod.design_lowcut(30.0, FS, ntaps)
        y, pk = gpu_filter_channels(lc, lc.Filter(taps, method="direct"), x)
        signs = set()
        for c in range(2):
            ref = oracle_mod.filter_channel(x[c], taps, oracle_mod.MODE_FMA)
            assert np.isinf(ref).sum() >= 4 and np.isfinite(ref).sum() > n // 2 and not np.isnan(ref).any()
            signs |= set(np.sign(ref[np.isinf(ref)]))
            assert same(y[c], ref), (ntaps, c)
            assert pk[c] == np.float32(np.inf)
        assert signs == {-1.0, 1.0}


# ---- 2. FFT forms: containment of a non-finite sample ------------------------
def hit_segments(flt, n, B, pos):
    """Segments of the grid anchored at output 0 whose input window holds a
    poisoned index, by the library's own window (lcfir_ctx_window)."""
    hit = []
    for s in range(-(-n // B)):
        lo, hi = flt.window(n, s * B, min(n, (s + 1) * B))
        if any(lo <= p < hi for p in pos):
            hit.append(s)
    return hit


def norm_call(lc, flt, x, prev, peak_val, force=False):
    """lcfir_filter_window_norm_dev over whole channels: (y, peaks, rescaled prev)."""
    nch, n = x.shape
    dx = lc.DeviceBuffer.from_array(x)
    dy = lc.DeviceBuffer(x.nbytes)
    dpk = lc.DeviceBuffer(4 * nch)
    lc.peak_reset_dev(dpk, nch)
    dprev = lc.DeviceBuffer.from_array(prev)
    dppk = lc.DeviceBuffer.from_array(np.array([peak_val], np.float32))
    flt.filter_window_norm_dev(dx, 0, n, n, n, nch, dy, 0, n, 0, n, dpk, 1, dprev, prev.size, dppk, 1, force)
    lc.sync()
    out = dy.download((nch, n)), dpk.download(nch), dprev.download(prev.size)
    for b in (dx, dy, dpk, dprev, dppk):
        b.free()
    return out


def scaled_ref(v, peak_val):
    """(float)((double)v * (1 / peak)) per element (peak_scale.hpp scale_one)."""
    with np.errstate(all="ignore"):
        gain = np.float64(1.0) / np.float64(np.float32(peak_val))
        return (v.astype(np.float64) * gain).astype(np.float32)


def special_values(rng, count):
    """Noise with NaN, +-Inf, -0.0, subnormals and 3e38 in the float4 body and the tail."""
    v = (rng.standard_normal(count) * 0.3).astype(np.float32)
    sp = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000],
                  np.uint32).view(np.float32)
    sp = np.r_[sp, np.float32(3e38), np.float32(-3e38)]
    v[100:100 + sp.size] = sp
    v[count - sp.size:] = sp[::-1]
    v[rng.integers(200, count - 200, 64)] = rng.choice(sp, 64)
    return v


def check_contained(lc, flt, taps, x, B, poison):
    """Assertions (a)-(e) of the containment contract for every poison position."""
    nch, n = x.shape
    half = (taps.size - 1) // 2
    y0, pk0 = gpu_filter_channels(lc, flt, x)
    assert np.isfinite(y0).all()
    ws, we = B // 2 + 11, 2 * B + 77  # a sub-range that starts and ends inside segments
    wlo, whi = flt.window(n, ws, we)
    yw0 = gpu_filter_window(lc, flt, x, ws, we, wlo, whi)
    assert bit_identical(yw0, y0[:, ws:we])
    nseg = -(-n // B)
    for pos in ([B + B // 2], [2 * B - 3], [0], [n - 1]):
        xp = x.copy()
        xp[1, pos] = POISONS[poison]
        hit = hit_segments(flt, n, B, pos)
        # one segment for B + B / 2 and 0, two for 2 B - 3 and n - 1 where half < B / 2; the
        # partitioned forms (half > B) read further and hit up to three
        assert pos[0] // B in hit and len(hit) < nseg, (pos, hit)
        if half < B // 2:
            assert hit == {B + B // 2: [1], 2 * B - 3: [1, 2], 0: [0], n - 1: [nseg - 2, nseg - 1]}[pos[0]], (pos, hit)
        y, pk = gpu_filter_channels(lc, flt, xp)
        # (a) the other channels, (b) the segments of channel 1 that are not hit
        assert bit_identical(y[0], y0[0]) and bit_identical(y[2], y0[2]), pos
        clean = np.ones(n, bool)
        for s in hit:
            clean[s * B:(s + 1) * B] = False
        assert clean.any() and bit_identical(y[1][clean], y0[1][clean]), (pos, hit)
        # (c) every output whose support holds the poison
        lo, hi = max(0, pos[0] - half), min(n, pos[0] + half + 1)
        assert not np.isfinite(y[1][lo:hi]).any(), (pos, np.nonzero(np.isfinite(y[1][lo:hi]))[0][:8] + lo)
        # (d) peaks: NaN skipped, Inf taken; the other channels' unchanged
        assert pk[1] == peak_rule(y[1]), (pos, pk)
        assert pk[0] == pk0[0] and pk[2] == pk0[2], pos
        # the same poisoned samples through a windowed call: the same bytes
        ywp = gpu_filter_window(lc, flt, xp, ws, we, wlo, whi)
        assert same_bits(ywp, y[:, ws:we]), pos
        # (e) no residue: clean calls straight after the poisoned ones
        y1, pk1 = gpu_filter_channels(lc, flt, x)
        assert bit_identical(y1, y0) and bit_identical(pk1, pk0), pos
        assert bit_identical(gpu_filter_window(lc, flt, x, ws, we, wlo, whi), yw0), pos
    return y0, pk0


@pytest.mark.parametrize("poison", ["nan", "pinf"])
@pytest.mark.parametrize("form", list(FFT_FORMS))
def test_fft_non_finite_sample_is_contained(lc, oracle_mod, form, poison):
    """One NaN / +Inf sample in channel 1 of 3, n = 4 B + 1 237.  The segment
    grid is anchored at output 0 (fir_fft.hpp fft_grid_start): segment s gives
    outputs [s B, (s + 1) B) and reads, over all partitions,
    [s B - half, s B - half + (P - 1) tp + L) with L = B + tp - 1 and P tp >= T
    (fft_window) -- the outputs' support [s B - half, (s + 1) B + half) widened by the
    P tp - T zero taps that pad the last partition, so the test takes the hit
    segments from lcfir_ctx_window, the code's own window.  Overlap-save turns
    a hit segment non-finite; nothing else may move: (a) the other channels,
    (b) the other segments, (c) every output whose support holds the sample is
    non-finite, (d) the fused peaks follow max |y| skipping NaN, (e) a clean
    call straight after, whole channels and a sub-range, gives the bytes of
    the clean call before (park slabs, f64 partial sums and LDS carry nothing
    over), (f) a previous buffer rescaled inside the launch (fused wherever the
    kernel carries a normalize) is rescaled byte-identically whether or not
    the current file is poisoned, a previous buffer of NaN, +-Inf, -0.0 and
    subnormals is rescaled as (float)((double)v * (1 / peak)), and the filter
    outputs do not depend on what that buffer holds."""
    import synth
    flt, taps, units = make_fft(lc, oracle_mod, form)
    B = units["outputs"]
    n, nch = 4 * B + 1237, 3
    assert n <= 130_000
    x = synth.file_buffer(nch, n, FS, file=21, bits=24)
    y0, pk0 = check_contained(lc, flt, taps, x, B, poison)
    # (f) the fused previous-file normalize
    rng = np.random.default_rng(B)
    fusable = units["nrm_floats"] > 0
    count, peak_val = 4099, 1.7  # float4 body and a 3-float tail; far below nseg x nch x nrm_floats
    assert not fusable or count <= units["nrm_floats"]
    xp = x.copy()
    xp[1, B + B // 2] = POISONS[poison]
    yp, pkp = gpu_filter_channels(lc, flt, xp)
    prev = (rng.standard_normal(count) * 0.3).astype(np.float32)
    special = special_values(rng, count)
    for xin, y_want, pk_want in ((x, y0, pk0), (xp, yp, pkp)):
        for buf, pv, force in ((prev, peak_val, False), (special, peak_val, False), (special, 0.6, True),
                               (special, np.inf, False)):
            st0 = flt.nrm_stats
            y, pk, r = norm_call(lc, flt, xin, buf, pv, force)
            st1 = flt.nrm_stats
            took = (st1["fused"] - st0["fused"], st1["separate"] - st0["separate"])
            assert took == ((1, 0) if fusable else (0, 1)), (form, took)
            assert same_bits(r, scaled_ref(buf, pv)), (form, pv)
            if buf is prev:
                assert bit_identical(r, scaled_ref(buf, pv))
            assert same_bits(y, y_want) and same_bits(pk, pk_want), (form, pv)
    # a quiet peak without force leaves even the special buffer alone, bit for bit
    y, pk, r = norm_call(lc, flt, x, special, 0.6, False)
    assert bit_identical(r, special) and bit_identical(y, y0)


def test_fft_no_residue_across_chunk_seams(lc, oracle_mod):
    """The partitioned L = 32 768 form with launches split into 65 536-output
    chunks (the f64 partial-sum scratch restarts at every seam and is reused
    by the next chunk in stream order): the same containment and no residue."""
    import synth
    flt, taps, units = make_fft(lc, oracle_mod, "l32_parts")
    flt.set_fft_tuning(seg_len=32768, chunk=65536)
    B = flt.fft_units["outputs"]
    assert B == units["outputs"]
    x = synth.file_buffer(3, 4 * B + 1237, FS, file=21, bits=24)
    y_one, pk_one = gpu_filter_channels(lc, make_fft(lc, oracle_mod, "l32_parts")[0], x)
    y0, pk0 = check_contained(lc, flt, taps, x, B, "nan")
    assert bit_identical(y0, y_one) and bit_identical(pk0, pk_one)


# ---- 3. homogeneity: scaling by a power of two is exact ----------------------
@pytest.fixture(scope="module")
def homogeneity_base(lc, oracle_mod):
    """y(x) and pk(x) of every kernel on the unscaled input, computed once."""
    import synth
    cache = {}

    def get(name):
        if name not in cache:
            flt, taps, B = make_kernel(lc, oracle_mod, name)
            x = synth.file_buffer(2, 2 * B + 999, FS, file=22, bits=24)
            y, pk = gpu_filter_channels(lc, flt, x)
            cache[name] = (flt, taps, B, x, y, pk)
        return cache[name]
    return get


@pytest.mark.parametrize("k", [-100, -24, 24, 100])
@pytest.mark.parametrize("kernel", list(FFT_FORMS) + ["direct"])
def test_power_of_two_scaling_is_exact(lc, oracle_mod, homogeneity_base, kernel, k):
    """Every kernel is f64 fma / mul / add of the samples, and scaling those by
    2^k is exact, so y(2^k x) = 2^k y(x) bit for bit wherever both sides are
    normal f32 (2^-126 <= |y(x)| 2^k <= 2^127; elsewhere the f32 result is
    subnormal or overflows and the two sides round differently by
    construction).  The synthetic int24 file through a 20 Hz low-cut keeps
    more than 99 % of its outputs in that range at every k (asserted; on the
    oracle's own output the share is 100 % at every k), so a kernel
    with an absolute floor or an absolute-error path anywhere fails.  The
    fused peak scales the same way.  At k = +-100 the scaled run is also held
    against the long-double oracle on the scaled input: <= 1 ulp (the 1e-12
    floor times 2^k) and RMS <= 1e-9 x 2^k."""
    flt, taps, B, x, y, pk = homogeneity_base(kernel)
    n = x.shape[1]
    with np.errstate(all="ignore"):
        xk, y_scaled, pk_scaled = np.ldexp(x, k), np.ldexp(y, k), np.ldexp(pk, k)
    assert np.array_equal(np.ldexp(xk.astype(np.float64), -k), x.astype(np.float64))  # exact in f32
    yk, pkk = gpu_filter_channels(lc, flt, xk)
    mag = np.ldexp(np.abs(y).astype(np.float64), k)
    cmp = (mag >= 2.0 ** -126) & (mag <= 2.0 ** 127)
    share = cmp.mean(axis=1)
    print(f"{kernel} k={k}: compared share per channel {share}")
    assert share.min() >= 0.99, share
    assert bit_identical(yk[cmp], y_scaled[cmp]), np.argwhere(cmp & (yk != y_scaled))[:8]
    assert bit_identical(pkk, pk_scaled)
    if abs(k) == 100:
        half = (taps.size - 1) // 2
        scale = 2.0 ** k
        for c in range(2):
            idx = positions(n, half, B, 512, 220 + c)
            ref, _ = oracle_mod.filter_points(xk[c], taps, idx, oracle_mod.MODE_LD)
            assert max_ulps(yk[c][idx], ref, floor=1e-12 * scale) <= 1, (kernel, c)
            assert rms(yk[c][idx], ref) <= RMS_TOL * scale, (kernel, c)


# ---- 4. subnormal samples in and out ------------------------------------------
def subnormal_input(rng, nch, n):
    """int24-valued noise x 2^-23 x 2^-120: full-range int24 in the first half
    (|x| up to 2^-120, mostly normal), +-2^12 in the second (|x| < 2^-131:
    subnormal samples and subnormal outputs)."""
    m = rng.integers(-2**23, 2**23, size=(nch, n))
    m[:, n // 2:] = rng.integers(-2**12, 2**12, size=(nch, n - n // 2))
    x = np.ldexp(m.astype(np.float64), -143).astype(np.float32)
    assert np.array_equal(np.ldexp(x.astype(np.float64), 143), m)  # every value exact
    return x


def is_subnormal(v):
    v = np.abs(np.asarray(v, np.float32))
    return (v > 0) & (v < np.float32(2.0 ** -126))


@pytest.mark.parametrize("ntaps", [15, 801])
def test_direct_subnormal_samples(lc, oracle_mod, ntaps):
    """Samples that span f32's subnormal boundary: the direct form is
    same() as the oracle's fma chain and bit-identical to it, subnormal
    outputs included (the reference output holds thousands, so a flush of the
    loads, the f32 -> f64 conversion or the narrowing cannot pass); the fused
    peak and peak_dev both give max |y| exactly."""
    n = 20_001
    x = subnormal_input(np.random.default_rng(ntaps + 4), 2, n)
    assert is_subnormal(x).sum() > n // 2 and (~is_subnormal(x) & (x != 0)).sum() > n // 2
    taps = oracle_mod.design_lowcut(30.0, FS, ntaps)
    flt = lc.Filter(taps, method="direct")
    y, pk = gpu_filter_channels(lc, flt, x)
    for c in range(2):
        ref = oracle_mod.filter_channel(x[c], taps, oracle_mod.MODE_FMA)
        assert is_subnormal(ref).sum() > n // 4 and (~is_subnormal(ref) & (ref != 0)).sum() > n // 4
        assert same(y[c], ref) and same_bits(y[c], ref), (ntaps, c)
        assert pk[c] == np.abs(ref).max() and pk[c] > 0
    # a channel of subnormal outputs only: its peak is a subnormal
    xs = np.ascontiguousarray(x[:, n // 2 + ntaps:])
    ys, pks = gpu_filter_channels(lc, flt, xs)
    assert is_subnormal(pks).all() and np.array_equal(pks, np.abs(ys).max(axis=1))
    dy = lc.DeviceBuffer.from_array(ys)
    dpk = lc.DeviceBuffer(8)
    lc.peak_reset_dev(dpk, 2)
    lc.peak_dev(dy, ys.shape[1], 2, ys.shape[1], dpk)
    lc.sync()
    assert bit_identical(dpk.download(2), pks)
    dy.free()
    dpk.free()


@pytest.mark.parametrize("form", ["l16_zero_phase", "l32_reg"])
def test_fft_subnormal_samples(lc, oracle_mod, form):
    """The same samples through the FFT (4 001 taps at both segment lengths):
    at most 1 f32 ulp -- a subnormal's ulp is 2^-149 -- from the long-double
    oracle at sampled positions, with no floor; fused peak and peak_dev equal
    max |y| exactly."""
    flt, taps, units = make_fft(lc, oracle_mod, form)
    B = units["outputs"]
    n = 2 * B + 999
    x = subnormal_input(np.random.default_rng(B + 4), 2, n)
    y, pk = gpu_filter_channels(lc, flt, x)
    dy = lc.DeviceBuffer.from_array(y)
    dpk = lc.DeviceBuffer(8)
    lc.peak_reset_dev(dpk, 2)
    lc.peak_dev(dy, n, 2, n, dpk)
    lc.sync()
    pk2 = dpk.download(2)
    dy.free()
    dpk.free()
    half = (taps.size - 1) // 2
    for c in range(2):
        idx = np.unique(np.r_[positions(n, half, B, 1024, 440 + c), np.arange(n - 600, n)])
        ref, _ = oracle_mod.filter_points(x[c], taps, idx, oracle_mod.MODE_LD)
        assert is_subnormal(ref).sum() > 300 and (~is_subnormal(ref) & (ref != 0)).sum() > 300
        assert max_ulps(y[c][idx], ref, floor=0.0) <= 1, (form, c)
        assert pk[c] == np.abs(y[c]).max() and pk2[c] == pk[c]


# ---- 5. post-pass and codec on the same values --------------------------------
def peak_inputs():
    rng = np.random.default_rng(55)
    n = 10_007
    tiny = np.ldexp(rng.integers(-2**20, 2**20, n).astype(np.float64), -149).astype(np.float32)
    cases = {}
    a = tiny.copy()
    a[[3, 4000, n - 1]] = np.nan
    a[5] = -0.0
    cases["subnormal_peak"] = a
    b = (rng.standard_normal(n) * 0.3).astype(np.float32)
    b[[0, 77, n - 2]] = np.nan
    b[[6, 5001]] = [3e38, -3.1e38]
    b[100:200] = tiny[100:200]
    cases["huge_peak"] = b
    c = b.copy()
    c[[9, 9000]] = [np.inf, -np.inf]
    cases["inf"] = c
    d = a.copy()
    d[n - 3] = -np.inf  # in the tail past the float4 body
    cases["neg_inf_in_tail"] = d
    cases["all_nan"] = np.full(n, np.nan, np.float32)
    return cases


@pytest.mark.parametrize("case", list(peak_inputs()))
def test_peak_of_special_values(lc, oracle_mod, case):
    """lcfir_peak_dev / lcfir_channel_peak on NaN, +-Inf, -0.0, subnormals and
    3e38 give oracle_max_mag (NaN skipped, Inf taken, a subnormal peak kept;
    0.0 for a channel of NaN), for a 16-byte aligned channel (the float4 body
    and its tail) and for 4-byte aligned ones."""
    v = peak_inputs()[case]
    n = v.size
    want = np.float32(oracle_mod.max_mag(v))
    assert want == peak_rule(v)
    assert lc.channel_peak(v) == want
    stride = n + 2  # channel 1 starts 4 (n + 2) bytes in: 4-byte aligned only
    buf = np.zeros(1 + 2 * stride, np.float32)
    buf[1:1 + n] = v
    buf[1 + stride:1 + stride + n] = v[::-1]
    dbuf = lc.DeviceBuffer.from_array(buf)
    dpk = lc.DeviceBuffer(16)
    lc.peak_reset_dev(dpk, 4)
    lc.peak_dev(dbuf.ptr + 4, stride, 2, n, dpk)  # both channels off the 16-byte grid
    dal = lc.DeviceBuffer.from_array(np.stack([v, v[::-1]]))
    lc.peak_dev(dal, n, 2, n, dpk.ptr + 8)  # channel 0 aligned, channel 1 at 4 n bytes
    lc.sync()
    assert bit_identical(dpk.download(4), np.full(4, want, np.float32))
    for b in (dbuf, dpk, dal):
        b.free()


@pytest.mark.parametrize("peak_bits,force", [(0x7F800000, False), (0x00000400, True), (0x00000400, False),
                                             (0x7F61B1E6, False)])
def test_normalize_and_scaled_encode_of_special_values(lc, peak_bits, force):
    """lcfir_normalize_dev on a buffer of NaN, +-Inf, -0.0, subnormals and 3e38
    with a peak of Inf (gain 1 / Inf = 0: finite samples become signed zeros,
    the rest NaN, as ProcessFile.cp:98-101 would), a subnormal peak with force
    (gain 2^139; without force it is left alone) and a peak of 3e38 (every
    finite output subnormal or 0): same() as (float)((double)v * (1 / peak)),
    bit for bit where not NaN; lcfir_encode_pcm_scaled_dev's s16le / s24be
    bytes equal normalize-then-encode, on the device and in numpy."""
    peak = np.array([peak_bits], np.uint32).view(np.float32)
    rng = np.random.default_rng(peak_bits & 0xFFFF)
    nch, frames = 2, 20_003
    x = np.stack([special_values(rng, frames), special_values(rng, frames)])
    scaled = bool((peak[0] > 1.0 or force) and peak[0] > 0.0)
    want = scaled_ref(x, peak[0]) if scaled else x
    if peak_bits == 0x7F800000:
        fin = np.isfinite(x)
        assert np.all(want[fin] == 0) and np.isnan(want[~fin]).all()
        assert np.array_equal(np.signbit(want[fin]), np.signbit(x[fin]))
    d_pk = lc.DeviceBuffer.from_array(np.r_[peak, np.float32(0.0)])
    d_y = lc.DeviceBuffer.from_array(x)
    lc.normalize_dev(d_y, frames, nch, frames, d_pk, 2, force)
    lc.sync()
    got = d_y.download((nch, frames))
    assert same(got, want) and same_bits(got, want)
    d_x = lc.DeviceBuffer.from_array(x)
    for fmt in ("s16le", "s24be"):
        nb = lc.pcm_bytes(fmt)
        d_fused = lc.DeviceBuffer(nb * nch * frames)
        d_ref = lc.DeviceBuffer(nb * nch * frames)
        lc.encode_pcm_scaled_dev(d_x, frames, nch, frames, fmt, d_pk, 2, force, d_fused)
        lc.encode_pcm_dev(d_y, frames, nch, frames, fmt, d_ref)
        lc.sync()
        fused = d_fused.download(nb * nch * frames, np.uint8).tobytes()
        assert fused == d_ref.download(nb * nch * frames, np.uint8).tobytes(), fmt
        with np.errstate(all="ignore"):
            assert fused == pcm_ref.np_encode(want, fmt), fmt
        d_fused.free()
        d_ref.free()
    assert bit_identical(d_x.download((nch, frames)), x)  # the fused pass leaves its input alone
    for b in (d_pk, d_y, d_x):
        b.free()


@pytest.mark.parametrize("fmt", ["f32le", "f32be"])
def test_f32_codec_passes_every_bit_pattern(lc, fmt):
    """f32le / f32be decode and encode move bits: 100 003 frames x 2 channels
    of random uint32 patterns, with signalling and quiet NaN payloads,
    subnormals, -0.0 and +-Inf forced in, come back bit for bit."""
    rng = np.random.default_rng(32)
    nch, frames = 2, 100_003
    v = rng.integers(0, 2**32, nch * frames, dtype=np.uint64).astype(np.uint32)
    forced = np.array([0x7F800001, 0xFFA00000, 0x7FC12345, 0xFFFFFFFF, 0x7FBFFFFF, 0x00000001, 0x807FFFFF,
                       0x80000000, 0x7F800000, 0xFF800000], np.uint32)
    v[:forced.size] = forced
    v[-forced.size:] = forced
    v[rng.integers(0, v.size, 1000)] = rng.choice(forced, 1000)
    raw = v.astype(">u4" if fmt.endswith("be") else "<u4").view(np.uint8)
    d_in = lc.DeviceBuffer.from_array(raw)
    stride = frames + 5
    d_out = lc.DeviceBuffer(4 * nch * stride)
    lc.decode_pcm_dev(d_in, fmt, nch, frames, d_out, stride)
    d_back = lc.DeviceBuffer(raw.size)
    lc.encode_pcm_dev(d_out, stride, nch, frames, fmt, d_back)
    lc.sync()
    got = d_out.download((nch, stride), np.uint32)[:, :frames]
    assert np.array_equal(got, v.reshape(frames, nch).T)
    assert np.array_equal(d_back.download(raw.size, np.uint8), raw)
    for b in (d_in, d_out, d_back):
        b.free()
