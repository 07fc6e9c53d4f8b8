"""GPU plan limits: every FFT kernel form at the tap counts where its plan
geometry ends, checked at every output.

lcfir_ctx_create and lcfir_ctx_set_method(FFT) take 1 to 1 048 575 taps
(fft_supported, kFftMaxTaps; even counts are refused).  The rest of the suite
runs the FFT kernels at 89 .. 100 001 taps, in the middle of each form's
range.  Here, the ends (fft_partition_count, fft_partition_taps, fir_fft.hpp):

  taps        tuning               plan
  1           L = 16 384 / 32 768  general table (T < 3 is never zero-phase), B = L
  3, 5        both L, both kernel  half = 1 (odd) / 2 (even): l16 zero-phase,
              families, and with   l32_reg, l32_park zero-phase, the general
              zero_phase off       tables; B = L - 2 / L - 4, no halo to speak of
  63, 65      AUTO                 63: the direct kernel; 65: the FFT (fft_preferred)
  10 921/923  L = 16 384           the longest one-partition filters of L = 16 384:
                                   B = 5 464 / 5 462, half 5 460 even / 5 461 odd
  10 925      L = 16 384           2 partitions of 5 463 taps (one zero tap of
                                   padding): kFftOutFirst straight into kFftOutLast
  21 845/847  L = 32 768           the longest one-partition filters of L = 32 768:
                                   B = 10 924 / 10 922, half 10 922 even / 10 923 odd
  21 849      L = 32 768           2 partitions of 10 925 taps
  1 048 575   L = 16 384           127 partitions of 8 257 taps, B = 8 128
              L = 32 768, AUTO     64 partitions of 16 385 taps, B = 16 384

(kFftMinB, B = 2 048, is not reachable: fft_partition_count moves to two
partitions long before a partition has kFftMaxPartTaps taps.)  Every case
asserts the plan it runs -- kernel, segment length, partitions, zero-phase form,
outputs per segment -- so a changed chooser fails here instead of moving a
case off its limit.

Checks (the conventions of test_gpu_tap_domain.py; bars unchanged):
  1. delays (h = e_k) on the general and partitioned plans, k at both ends,
     around the centre and at the first and last tap of each partition: y[n] =
     x[n + k - half] bit for bit (T = 1: the identity);
  2. pairs (h[half -+ d] = 0.5) on every zero-phase plan, then the general
     table on the same taps, bit for bit;
  3. dense parity with the long-double oracle (RMS <= 1e-9, <= 1 f32 ulp with
     the 1e-12 floor, fused peak == max |y|): the designed low-cut on every
     plan, standard_normal / sqrt(T) on the general ones.  The designed low-cut
     of 1 tap is [0] and of 3 taps ~1e-20 (the Blackman window's ends), which
     holds a kernel to nothing, so the zero-phase plans of 3 and 5 taps also
     run a symmetrised standard_normal;
  4. partition invariance: a channel as three ragged device ranges, cut off the
     segment seams, has the whole-channel bytes;
  5. the fused normalize on the one-partition plans: count = 1, the plan's own
     fused / separate switch (units x nrm_floats) and one float past it;
  6. AUTO at 63 / 65 taps: the method, then the fma chain bit for bit (direct)
     and the oracle at every output (FFT).

Shapes: two channels of different known_answer.grid16 data, n = max(2 B + B // 3
+ 1, T + B // 2): two seams and a partial tail, at most 76 459 samples below
the top row.  Outputs go through y_stride = n + 7 with a sentinel in the
padding that must survive.  The oracle runs at every output while one
channel's n x T <= test_gpu_persistent_rounds.WORK (everything here below the
top row: 1.1e9 at 21 849 taps, ~0.2 s on 16 threads).

The 1 048 575-tap row (n = 1.06 M) is one test per segment length, and cheap
on purpose: a plan's tables take ~1 s of host time per filter, so each test
builds four filters -- the delays k = 0, T - 1 and 63 tp (the first tap of the
middle partition of 127; of the last of 64, the one whose tail is the padding)
and the designed low-cut, held to the oracle at WORK // T = 1 144 positions
over the two channels: both ends, the neighbours of every seam, the rest
spread evenly.
"""
import time

import numpy as np
import pytest

import known_answer as ka
from test_gpu_parity import RMS_TOL, gpu_filter_channels, max_ulps, rms
from test_gpu_persistent_rounds import PAD, SENTINEL, WORK
from test_gpu_tap_domain import _geometry, _input, _known, _length

pytestmark = pytest.mark.gpu

FS = 48000.0
PERTURB = 1e-9  # test_gpu_persistent_rounds' l32_park_general: antisymmetric part >> 2^-50 |h|_1
T_MAX = 1_048_575

# id: taps, tuning (seg_len, zero_phase, family), perturbation, then the plan it must give
LIMITS = {}


def _limit(name, ntaps, seg_len, kernel, zero_phase, outputs, parts=1, family=None, perturb=0.0, general=False):
    LIMITS[name] = dict(ntaps=ntaps, seg_len=seg_len, kernel=kernel, zero_phase=zero_phase, outputs=outputs,
                        parts=parts, family=family, perturb=perturb, tune_zero_phase=not general)


_limit("t1_l16", 1, 16384, "l16", False, 16384)
_limit("t1_l32", 1, 32768, "l32_park", False, 32768)
for _T, _B16, _B32 in ((3, 16382, 32766), (5, 16380, 32764)):
    _limit(f"t{_T}_l16", _T, 16384, "l16", True, _B16)
    _limit(f"t{_T}_l16_lds", _T, 16384, "l16", True, _B16, family="lds")
    _limit(f"t{_T}_l16_general", _T, 16384, "l16", False, _B16, general=True)
    _limit(f"t{_T}_l32", _T, 32768, "l32_reg", True, _B32)
    _limit(f"t{_T}_l32_lds", _T, 32768, "l32_park", True, _B32, family="lds")
    _limit(f"t{_T}_l32_general", _T, 32768, "l32_park", False, _B32, general=True)
for _T, _B in ((10921, 5464), (10923, 5462)):
    _limit(f"t{_T}_l16", _T, 16384, "l16", True, _B)
    _limit(f"t{_T}_l16_perturbed", _T, 16384, "l16", False, _B, perturb=PERTURB)
_limit("t10925_l16_parts2", 10925, 16384, "l16", False, 10922, parts=2)
for _T, _B in ((21845, 10924), (21847, 10922)):
    _limit(f"t{_T}_l32", _T, 32768, "l32_reg", True, _B)
    _limit(f"t{_T}_l32_lds", _T, 32768, "l32_park", True, _B, family="lds")
    _limit(f"t{_T}_l32_perturbed", _T, 32768, "l32_park", False, _B, perturb=PERTURB)
_limit("t21849_l32_parts2", 21849, 32768, "l32_park", False, 21844, parts=2)
# the top row: its own tests below
TOP = {
    "top_l16": dict(ntaps=T_MAX, seg_len=16384, kernel="l16", zero_phase=False, outputs=8128, parts=127,
                    family=None, perturb=0.0, tune_zero_phase=True),
    "top_l32": dict(ntaps=T_MAX, seg_len=32768, kernel="l32_park", zero_phase=False, outputs=16384, parts=64,
                    family=None, perturb=0.0, tune_zero_phase=True),
}
TOP_TP = {"top_l16": 8257, "top_l32": 16385}

ZERO_PHASE = [n for n, f in LIMITS.items() if f["zero_phase"]]
NOT_ZERO_PHASE = [n for n, f in LIMITS.items() if not f["zero_phase"]]  # the general table, partitioned or not
ONE_PARTITION = [n for n, f in LIMITS.items() if f["parts"] == 1]
DENSE = [(n, "designed") for n in LIMITS] + [(n, "normal") for n in NOT_ZERO_PHASE] + \
        [(n, "symmetric") for n in ZERO_PHASE if LIMITS[n]["ntaps"] <= 5]


def test_the_tables_cover_the_limits():
    """The case lists are the ones the module's header promises (no GPU work)."""
    assert len(LIMITS) == 26 and len(ZERO_PHASE) == 14 and len(NOT_ZERO_PHASE) == 12 and len(ONE_PARTITION) == 24
    for name, f in {**LIMITS, **TOP}.items():
        tp = ka.partition_taps(f["ntaps"], f["parts"])
        assert f["outputs"] == f["seg_len"] - tp + 1, name
        assert not (f["zero_phase"] and f["parts"] > 1), name
    assert {f["kernel"] for f in LIMITS.values()} == {"l16", "l32_park", "l32_reg"}
    assert {LIMITS[n]["kernel"] for n in ZERO_PHASE} == {"l16", "l32_park", "l32_reg"}
    # both parities of half on every zero-phase kernel, at the short and at the long end
    for kernel in ("l16", "l32_park", "l32_reg"):
        halves = sorted({(LIMITS[n]["ntaps"] - 1) // 2 for n in ZERO_PHASE if LIMITS[n]["kernel"] == kernel})
        assert halves[:2] == [1, 2] and len(halves) == 4 and {h % 2 for h in halves[2:]} == {0, 1}, (kernel, halves)
    assert [ka.partition_taps(T_MAX, TOP[n]["parts"]) for n in TOP] == [TOP_TP[n] for n in TOP]


@pytest.fixture(scope="module")
def lc():
    import lcfir
    assert lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


def _plan(lc, taps, name, zero_phase=None):
    """A Filter of `taps` tuned as the limit `name`, the plan it claims
    asserted.  zero_phase: None = the form's own tuning; False = the general
    table at the form's segment length (a register-kernel form then runs the
    park-slab kernel)."""
    f = LIMITS.get(name) or TOP[name]
    assert taps.size == f["ntaps"], (name, taps.size)
    kernel, zp = f["kernel"], f["zero_phase"] if zero_phase is None else zero_phase
    if not zp and kernel == "l32_reg":
        kernel = "l32_park"
    flt = lc.Filter(taps, method="fft")
    flt.set_fft_tuning(seg_len=f["seg_len"], zero_phase=f["tune_zero_phase"] if zero_phase is None else zero_phase)
    if f["family"]:
        flt.set_fft_family(f["family"])
    info, units = flt.fft_info, flt.fft_units
    assert units["kernel"] == kernel, (name, units)
    assert info == {"seg_len": f["seg_len"], "parts": f["parts"], "zero_phase": zp}, (name, info)
    assert units["outputs"] == f["outputs"], (name, units)
    return flt, f["outputs"], ka.partition_taps(taps.size, f["parts"])


def _taps(oracle_mod, name, family="designed"):
    f = LIMITS.get(name) or TOP[name]
    T = f["ntaps"]
    if family == "designed":
        taps = oracle_mod.design_lowcut(20.0, FS, T)
        if f["perturb"]:
            taps = taps + f["perturb"] * np.linspace(-1.0, 1.0, T)
        return taps
    g = np.random.default_rng(T).standard_normal(T) / np.sqrt(T)
    return g if family == "normal" else 0.5 * (g + g[::-1])


def _live_family(name):
    """The taps of the checks that need outputs worth comparing: the designed
    low-cut, except at 1 and 3 taps, where it is (numerically) all zeros."""
    f = LIMITS[name]
    return "designed" if f["ntaps"] > 3 else "symmetric" if f["zero_phase"] else "normal"


def _x(T, B):
    x = _input(_length(T, B))
    assert x.shape[1] >= 2 * B + 2 and x.shape[1] % B  # two seams and a partial tail
    return x


def _run(lc, flt, x):
    """lcfir_filter_channels_dev into rows of n + PAD floats preset to
    SENTINEL: the padding intact, the fused peak == max |y| per channel."""
    nch, n = x.shape
    dx = lc.DeviceBuffer.from_array(x)
    dy = lc.DeviceBuffer.from_array(np.full((nch, n + PAD), SENTINEL, np.float32))
    dpk = lc.DeviceBuffer(4 * nch)
    lc.peak_reset_dev(dpk, nch)
    flt.filter_channels_dev(dx, n, nch, n, dy, n + PAD, dpk)
    lc.sync()
    rows = dy.download((nch, n + PAD))
    pk = dpk.download(nch)
    for b in (dx, dy, dpk):
        b.free()
    assert np.all(rows[:, n:] == SENTINEL), np.argwhere(rows[:, n:] != SENTINEL)[:8].tolist()
    y = np.ascontiguousarray(rows[:, :n])
    assert np.array_equal(pk, np.abs(y).max(axis=1)), (pk, np.abs(y).max(axis=1))
    return y, pk


def _oracle(oracle_mod, taps, x, y, where, idx=None):
    """Every output of every channel (idx: those positions) against the long-double oracle."""
    t0 = time.perf_counter()
    for c in range(x.shape[0]):
        if idx is None:
            assert x.shape[1] * taps.size <= WORK, where
            got, ref = y[c], oracle_mod.filter_channel_mt(x[c], taps, 16, oracle_mod.MODE_LD)
        else:
            got, ref = y[c][idx], oracle_mod.filter_points(x[c], taps, idx, oracle_mod.MODE_LD)[0]
        r, u = rms(got, ref), max_ulps(got, ref)
        print(f"{where} channel {c}: {got.size} of n={x.shape[1]} outputs, rms={r:.3e} max_ulps={u}")
        assert r <= RMS_TOL, (where, c, r)
        assert u <= 1, (where, c, u)
    print(f"{where}: oracle {time.perf_counter() - t0:.2f} s")


# ---- 1: delays on the general and partitioned plans ------------------------------------
@pytest.mark.parametrize("name", NOT_ZERO_PHASE)
def test_delays_general_plans(lc, name):
    f = LIMITS[name]
    T, parts = f["ntaps"], f["parts"]
    half = (T - 1) // 2
    tp = ka.partition_taps(T, parts)
    ks = ka.delay_ks(T, ka.partition_edges(T, tp, parts))
    assert {0, half, T - 1} <= set(ks) and (T > 1 or ks == [0])
    assert all(p * tp - 1 in ks and p * tp in ks for p in range(1, parts)) and (parts - 1) * tp < T
    failures = []
    for k in ks:
        flt, B, tp_plan = _plan(lc, ka.delay_taps(T, k), name, zero_phase=False)
        assert tp_plan == tp
        x = _x(T, B)
        y, _ = _run(lc, flt, x)
        _known(failures, y, ka.expect_delay(x, T, k), False, f"{name} delay k={k} (partition {k // tp}, tap {k % tp})")
        flt.close()
    assert not failures, _geometry(B, tp, parts, half) + "\n" + "\n".join(failures)


# ---- 2: pairs on the zero-phase plans, then the general table on the same taps ----------
@pytest.mark.parametrize("name", ZERO_PHASE)
def test_pairs_zero_phase_plans(lc, name):
    T = LIMITS[name]["ntaps"]
    half = (T - 1) // 2
    ds = ka.pair_ds(T)
    assert {0, 1, half} <= set(ds) and (2047 in ds) == (half >= 2047)
    failures = []
    for zero_phase in (None, False):
        for d in ds:
            flt, B, _ = _plan(lc, ka.pair_taps(T, d), name, zero_phase=zero_phase)
            x = _x(T, B)
            y, _ = _run(lc, flt, x)
            _known(failures, y, ka.expect_pair(x, T, d), False,
                   f"{name} pair d={d} {'general table' if zero_phase is False else 'zero-phase'}")
            flt.close()
    assert not failures, _geometry(B, T, 1, half) + "\n" + "\n".join(failures)


# ---- 3: dense oracle parity ---------------------------------------------------------------
@pytest.mark.parametrize("name,family", DENSE)
def test_dense_oracle_parity(lc, oracle_mod, name, family):
    taps = _taps(oracle_mod, name, family)
    if family == "symmetric":
        assert np.array_equal(taps, taps[::-1]) and np.abs(taps).min() > 1e-3
    flt, B, _ = _plan(lc, taps, name)
    x = _x(taps.size, B)
    y, _ = _run(lc, flt, x)
    assert np.isfinite(y).all()
    _oracle(oracle_mod, taps, x, y, f"{name} {family}")


# ---- 4: partition invariance --------------------------------------------------------------
@pytest.mark.parametrize("name", list(LIMITS))
def test_ragged_ranges_give_the_whole_channel_bytes(lc, oracle_mod, name):
    taps = _taps(oracle_mod, name, _live_family(name))
    flt, B, _ = _plan(lc, taps, name)
    x = _x(taps.size, B)
    nch, n = x.shape
    y, pk = _run(lc, flt, x)
    whole, pk_whole = gpu_filter_channels(lc, flt, x)  # y_stride = n
    assert np.array_equal(whole, y) and np.array_equal(pk_whole, pk)
    assert np.all(pk > 0.01)
    cuts = [0, B // 3 + 1, B + B // 2 + 3, n]
    assert all(c % B for c in cuts[1:]) and cuts == sorted(cuts) and cuts[1] < B < cuts[2] < 2 * B < n
    for c in range(nch):
        dx = lc.DeviceBuffer.from_array(x[c])
        dy = lc.DeviceBuffer.from_array(np.full(n, SENTINEL, np.float32))
        for s, e in zip(cuts[:-1], cuts[1:]):
            flt.apply_range_dev(dx, n, dy, s, e)
        lc.sync()
        got = dy.download(n)
        dx.free()
        dy.free()
        bad = np.nonzero(got.view(np.int32) != y[c].view(np.int32))[0]
        assert bad.size == 0, (name, c, bad.size, bad[:8].tolist(), cuts, B)


# ---- 5: the fused normalize on the one-partition plans ----------------------------------
def _window_rows(lc, flt, x, nrm=None):
    """lcfir_filter_window_dev over the whole channels (nrm: the (buffer,
    count, peaks, npeak, force) of lcfir_filter_window_norm_dev): rows of n +
    PAD floats and the peaks."""
    nch, n = x.shape
    dx = lc.DeviceBuffer.from_array(x)
    dy = lc.DeviceBuffer.from_array(np.full((nch, n + PAD), SENTINEL, np.float32))
    dpk = lc.DeviceBuffer(4 * nch)
    lc.peak_reset_dev(dpk, nch)
    if nrm is None:
        flt.filter_window_dev(dx, 0, n, n, n, nch, dy, 0, n + PAD, 0, n, dpk, peak_stride=1)
    else:
        flt.filter_window_norm_dev(dx, 0, n, n, n, nch, dy, 0, n + PAD, 0, n, dpk, 1, *nrm)
    lc.sync()
    rows, pk = dy.download((nch, n + PAD)), dpk.download(nch)
    for b in (dx, dy, dpk):
        b.free()
    return rows, pk


@pytest.mark.parametrize("name", ONE_PARTITION)
def test_fused_normalize_at_the_switch(lc, oracle_mod, name):
    """lcfir_filter_window_norm_dev against lcfir_filter_window_dev +
    lcfir_normalize_dev, byte for byte, with count = 1, at the plan's fused /
    separate switch (units x nrm_floats, test_gpu_fuzz._norm_params) and one
    float past it; nrm_stats says which way each call went (the park-slab
    kernel fuses nothing).  The rescaled buffer also equals (float)((double)v *
    (1.0 / (double)pk)) under the ProcessFile.cp:98-101 decision, and the
    guard floats around it stay."""
    taps = _taps(oracle_mod, name, _live_family(name))
    flt, B, _ = _plan(lc, taps, name)
    cap = flt.fft_units["nrm_floats"]
    blk = 2048 if flt.fft_units["kernel"] == "l32_reg" else 1024
    assert (cap > 0) == (flt.fft_units["kernel"] != "l32_park") and cap % blk == 0, flt.fft_units
    x = _x(taps.size, B)
    nch, n = x.shape
    units = -(-n // B) * nch
    assert units == 6
    boundary = units * (cap or 1024)
    rows0, pk0 = _window_rows(lc, flt, x)
    assert np.all(rows0[:, n:] == SENTINEL) and np.array_equal(pk0, np.abs(rows0[:, :n]).max(axis=1))
    assert flt.nrm_stats == {"fused": 0, "separate": 0}
    flt.close()
    for count, fusable in ((1, True), (boundary, True), (boundary + 1, False)):
        want_stats = {"fused": 1, "separate": 0} if cap and fusable else {"fused": 0, "separate": 1}
        prev = (np.random.default_rng(count).standard_normal(count + 8) * 0.3).astype(np.float32)
        for peaks, force in (([0.75, 1.7], False), ([0.5], False)):
            pkmax = np.float32(max(peaks))
            scaled = (pkmax > 1.0 or force) and pkmax > 0.0
            want = prev.copy()
            if scaled:
                want[4:4 + count] = (prev[4:4 + count].astype(np.float64) * (1.0 / np.float64(pkmax))).astype(np.float32)
            dppk = lc.DeviceBuffer.from_array(np.asarray(peaks, np.float32))
            # inside the filter call
            buf = lc.DeviceBuffer.from_array(prev)
            assert (buf.ptr + 16) % 16 == 0
            flt, _, _ = _plan(lc, taps, name)
            rows, pk = _window_rows(lc, flt, x, nrm=(buf.ptr + 16, count, dppk, len(peaks), force))
            case = (name, count, peaks, flt.nrm_stats)
            assert flt.nrm_stats == want_stats, case
            flt.close()
            assert np.array_equal(rows, rows0) and np.array_equal(pk, pk0), case
            got = buf.download(count + 8)
            # its own pass
            buf2 = lc.DeviceBuffer.from_array(prev)
            lc.normalize_dev(buf2.ptr + 16, count, 1, count, dppk, len(peaks), force)
            lc.sync()
            sep = buf2.download(count + 8)
            for b in (buf, buf2, dppk):
                b.free()
            assert np.array_equal(got[:4], prev[:4]) and np.array_equal(got[4 + count:], prev[4 + count:]), case
            assert np.array_equal(got, sep), case
            assert np.array_equal(got, want), case
            assert scaled == (not np.array_equal(got, prev)), case


# ---- 6: AUTO either side of fft_preferred ---------------------------------------------------
def test_auto_63_taps_runs_the_direct_kernel(lc, oracle_mod):
    taps = oracle_mod.design_lowcut(20.0, FS, 63)
    flt = lc.Filter(taps)  # AUTO
    assert flt.method == "direct"
    x = _x(65, 16320)  # the 65-tap case's channels
    y, _ = _run(lc, flt, x)
    for c in range(x.shape[0]):
        ref = oracle_mod.filter_channel(x[c], taps, oracle_mod.MODE_FMA)
        bad = np.nonzero(y[c].view(np.int32) != ref.view(np.int32))[0]
        assert bad.size == 0, (c, bad.size, bad[:8].tolist())
    _oracle(oracle_mod, taps, x, y, "auto 63 taps")


def test_auto_65_taps_runs_the_fft(lc, oracle_mod):
    taps = oracle_mod.design_lowcut(20.0, FS, 65)
    flt = lc.Filter(taps)  # AUTO, default tuning
    assert flt.method == "fft"
    info, units = flt.fft_info, flt.fft_units
    assert info == {"seg_len": 16384, "parts": 1, "zero_phase": True}, info
    assert units["kernel"] == "l16" and units["outputs"] == 16384 - 64, units
    x = _x(65, units["outputs"])
    y, _ = _run(lc, flt, x)
    _oracle(oracle_mod, taps, x, y, "auto 65 taps")


# ---- the 1 048 575-tap row ----------------------------------------------------------------
def _top_points(n, B, budget):
    """`budget` positions of a channel: 16 at either end, the neighbours of
    every segment seam (two each side while that takes at most half the budget,
    else one), the rest spread evenly.  (test_gpu_persistent_rounds._oracle_points
    has the same three parts, but its fixed part alone is 4 per seam + 192: past
    the budget at 129 seams.)"""
    nseg = -(-n // B)
    w = 2 if 4 * (nseg - 1) <= budget // 2 else 1
    seams = (np.arange(1, nseg)[:, None] * B + np.arange(-w, w)).ravel()
    must = np.unique(np.r_[np.arange(16), np.arange(n - 16, n), seams])
    assert must.size < budget and must.min() >= 0 and must.max() < n
    rest = np.linspace(0, n - 1, budget - must.size).round().astype(np.int64)
    return np.unique(np.r_[must, rest])


@pytest.mark.parametrize("name", list(TOP))
def test_longest_filter(lc, oracle_mod, name):
    """The longest filter the FFT method takes: 127 (64) launches into the f64
    partial sums, input offsets half - p tp from +524 287 down to -516 095
    (-507 968), 64 (65) zero taps behind the last partition.  Four filters:
    three delays bit for bit at every output, the designed low-cut against the
    oracle at WORK // T positions."""
    f = TOP[name]
    T, parts, tp, B = f["ntaps"], f["parts"], TOP_TP[name], f["outputs"]
    half = (T - 1) // 2
    assert parts * tp - T == (64 if name == "top_l16" else 65) and half - (parts - 1) * tp < -500_000
    x = _x(T, B)
    nch, n = x.shape
    assert n == T + B // 2 and nch == 2 and 63 * tp < T
    t0 = time.perf_counter()
    failures = []
    for k in (0, T - 1, 63 * tp):
        flt, B_plan, tp_plan = _plan(lc, ka.delay_taps(T, k), name)
        assert (B_plan, tp_plan) == (B, tp)
        y, _ = _run(lc, flt, x)
        _known(failures, y, ka.expect_delay(x, T, k), False, f"{name} delay k={k} (partition {k // tp}, tap {k % tp})")
        flt.close()
    print(f"{name}: three delays {time.perf_counter() - t0:.2f} s")
    assert not failures, _geometry(B, tp, parts, half) + "\n" + "\n".join(failures)
    taps = _taps(oracle_mod, name)
    flt, _, _ = _plan(lc, taps, name)
    y, _ = _run(lc, flt, x)
    assert np.isfinite(y).all()
    idx = _top_points(n, B, int(WORK // T) // nch)
    assert 500 <= idx.size <= 600 and idx.size * nch * T <= WORK
    _oracle(oracle_mod, taps, x, y, f"{name} designed", idx=idx)


def test_longest_filter_auto_segment_length(lc):
    """seg_len = 0 at 1 048 575 taps: the chooser takes L = 32 768 (fft_info only)."""
    flt = lc.Filter(ka.delay_taps(T_MAX, 0), method="fft")
    assert flt.fft_info == {"seg_len": 32768, "parts": 64, "zero_phase": False}, flt.fft_info
    assert flt.fft_units == {"outputs": 16384, "kernel": "l32_park", "nrm_floats": 0}, flt.fft_units


def test_one_tap_past_the_longest_filter_is_refused(lc):
    """1 048 577 taps: lcfir_ctx_set_method(FFT) returns LCFIR_EINVAL, so no
    plan is built and nothing is launched; AUTO resolves to the direct kernel."""
    taps = ka.delay_taps(T_MAX + 2, 0)
    with pytest.raises(lc.LcfirError) as e:
        lc.Filter(taps, method="fft")
    assert e.value.code == lc.EINVAL and "1048577" in str(e.value), str(e.value)
    flt = lc.Filter(taps)  # AUTO
    assert flt.method == "direct"
    with pytest.raises(lc.LcfirError) as e:
        flt.set_method("fft")
    assert e.value.code == lc.EINVAL
    assert flt.method == "direct"
    assert flt.fft_info == {"seg_len": 0, "parts": 0, "zero_phase": False}
    flt.close()
    with pytest.raises(lc.LcfirError) as e:  # even tap counts never reach a method
        lc.Filter(np.ones(T_MAX + 1), method="fft")
    assert e.value.code == lc.EINVAL
