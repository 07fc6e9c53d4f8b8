"""Multi-round launches of every FFT kernel form's persistent grid.

fft_launch_one / fft32_launch_one / fft32r_launch_one (fir_fft.hpp) launch
min(units, CUs) workgroups; workgroup b walks the units fft_unit32(rnd, b, grid,
units), rnd = 0, 1, ...  What a kernel does only from its second unit on -- the
sample prefetch inside the previous unit's final phase, the stage-1 LDS write
over what that final phase read (no barrier between them), the carried twiddle
powers wt[], the fused peak's pk_run / pk_ch / pk_pending across a channel
change, the park slab's reuse, the (channel, segment) addressing of the f64
partial sums, the fused normalize's slices of units u >= grid, fft_unit32's
swizzled full rounds and its identity tail -- needs units > CUs to run at all.

What the suite gave a second unit before this module (units = nch x
ceil(n / B) against the 256 CUs of an MI355X; B = L - taps_per_partition + 1):
  * test_many_channels[fft-4001]: 300 x 1 units, l32_reg (B = 28 768);
  * test_fft_auto_seg_len[12001-3000000-2]: 2 x 145 = 290 units, l32_reg;
  * the slow full-size cases (config 2: 2 x 1 002, config 3: 8 x 233, the
    config-4/5 batch and the > 2 GiB channel): 4 001 / 8 001 symmetric taps, all
    l32_reg.
Everything else stays in round 0: test_gpu_fuzz (n <= 300 001, nch <= 3, B >=
8 384: <= 108 units), test_fft_seg32_forms and
test_fft_partitioned_long_filters (300 000 samples x 2 channels, B >= 8 000:
<= 76 units), test_fft_auto_seg_len's other cases (<= 8 x 25 = 200),
test_partition_invariance, the edge / stride / value-domain / batch / CLI
tests (a few dozen units).  So l16 (fir_fft_f64_kernel:
Sym, F32, First/Add/Last and the kNrm variants), l32_park (fir_fft32_f64_kernel,
every form) and l32_reg's kNrm variant never ran past round 0 under a check.

Shapes come from the device and the plan: cus = multi_processor_count, B =
fft_units["outputs"], a case is (nch, nseg) with n = (nseg - 1) B + 777:
  tail1    nch = cus + 1, nseg = 1 (n = B - 5): one full round + a one-unit tail;
  exact2   nch = 8, nseg = cus / 4: units == 2 cus, base + g == units in round 1;
  rounds3  nch = 9, nseg = ceil((2 cus + cus // 3) / 9): two full rounds and a
           partial tail, every workgroup changing channel between its units;
  stay     nch = 2, nseg = cus + cus // 2 + 3: three units for most workgroups,
           the later ones on the same channel (pk_ch kept, nothing pending).
Every test asserts its precondition (kernel, segment length, partitions,
zero-phase form, units against cus, the rounds / swizzle / tail / channel
moves its case is named for: _walk restates fft_unit32) so it cannot degrade
to one round unnoticed.

Input: synth.file_buffer(nch, n, 48 kHz, file=60, int24), channel c scaled by
0.2 + 0.7 c / nch (distinct peaks: a peak committed to the wrong channel cannot
pass); channel nch // 2 is all zeros where nch >= 3 and must stay zeros with
peak 0.  (The two channels of `stay` both carry signal: zeroing one would blank
most of the later rounds, which is what that case is for.)

Checks per case:
  (a) outputs and peaks bit for bit against the same plan launched in single
      rounds (set_fft_tuning chunk = k B, max_units = cus // 2: every launch
      <= cus units, asserted) -- fir_fft.hpp's partition invariance, and the
      path the rest of the suite pins to the oracle;
  (b) the long-double oracle (RMS <= 1e-9, <= 1 f32 ulp, 1e-12 floor) at the
      two outputs each side of every segment seam, both channel ends, the
      half + 64 edge outputs and random positions;
  (c) pk[c] == max |y[c]| for every channel;
  (d) y_stride = n + 7 with a sentinel in the padding that must survive.

Oracle budget: filter_points (long double) measured 0.9e9 tap x point / s on
a CPU-only box at 4 001 .. 100 001 taps (1.8e9 at the channel ends, where the
taps are cut short).  A case spends at most WORK = 1.2e9 (about 1.3 s; 12 000
points at 100 001 taps, 300 000 at 4 001): as many evenly spaced
channels as fit (at least 4: the first, the last, two between), every seam
point always, the 64 outputs at either end and 64 random positions always, the
rest of the half + 64 edge outputs and 448 more random positions thinned
evenly to what is left.
"""
import numpy as np
import pytest

from test_gpu_parity import RMS_TOL, max_ulps, rms

pytestmark = pytest.mark.gpu

FS = 48000.0
FILE_ID = 60
PAD, SENTINEL = 7, -7.0
WORK = 1.2e9  # tap x point products of oracle work per case

# id: ntaps, antisymmetric perturbation, set_fft_tuning, family, then the plan it must give
FORMS = {
    "l16_sym": dict(ntaps=4001, tune=dict(seg_len=16384), kernel="l16", seg_len=16384, zero_phase=True, parts=1),
    "l16_general": dict(ntaps=4003, tune=dict(seg_len=16384, zero_phase=False), kernel="l16", seg_len=16384,
                        zero_phase=False, parts=1),
    "l16_parts": dict(ntaps=40001, tune=dict(seg_len=16384), kernel="l16", seg_len=16384, zero_phase=False,
                      parts=5),
    "l32_park_sym": dict(ntaps=8001, tune=dict(seg_len=32768), family="lds", kernel="l32_park", seg_len=32768,
                         zero_phase=True, parts=1),
    "l32_park_general": dict(ntaps=8001, perturb=1e-9, tune=dict(seg_len=32768), kernel="l32_park",
                             seg_len=32768, zero_phase=False, parts=1),
    "l32_park_parts": dict(ntaps=100001, tune=dict(seg_len=32768), kernel="l32_park", seg_len=32768,
                           zero_phase=False, parts=6),
    "l32_reg": dict(ntaps=4001, tune=dict(), kernel="l32_reg", seg_len=32768, zero_phase=True, parts=1),
}
CASES = ["tail1", "exact2", "rounds3", "stay"]


@pytest.fixture(scope="module")
def dev():
    import torch  # before lcfir: one HIP runtime in the process
    import lcfir
    assert torch.cuda.is_available() and lcfir.device_count() >= 1, "no GPU visible"
    return torch, lcfir, int(torch.cuda.get_device_properties(0).multi_processor_count)


def _taps(oracle_mod, form):
    f = FORMS[form]
    taps = oracle_mod.design_lowcut(20.0, FS, f["ntaps"])
    if f.get("perturb"):
        taps = taps + f["perturb"] * np.linspace(-1.0, 1.0, f["ntaps"])  # antisymmetric part >> 2^-50 |h|_1
    return taps


def _filter(lc, taps, form, **launch):
    """The form's Filter (launch: chunk / max_units on top of its tuning),
    with the plan it claims to run asserted."""
    f = FORMS[form]
    flt = lc.Filter(taps, method="fft")
    flt.set_fft_tuning(**f["tune"], **launch)
    if f.get("family"):
        flt.set_fft_family(f["family"])
    info, units = flt.fft_info, flt.fft_units
    assert units["kernel"] == f["kernel"], (form, units)
    assert info["seg_len"] == f["seg_len"] and info["zero_phase"] == f["zero_phase"], (form, info)
    assert info["parts"] == f["parts"] and (f["parts"] == 1 or info["parts"] >= 3), (form, info)
    return flt


def _shape(case, cus, B):
    """(nch, nseg, n) of a unit-count case."""
    if case == "tail1":
        return cus + 1, 1, B - 5
    if case == "exact2":
        if cus % 4:
            pytest.skip(f"{cus} CUs: no 8-channel grid of exactly 2 x CUs units")
        nch, nseg = 8, cus // 4
    elif case == "rounds3":
        nch = 9
        nseg = -(-(2 * cus + cus // 3) // nch)
        if (nch * nseg) % cus == 0:
            nseg += 1
    else:
        nch, nseg = 2, cus + cus // 2 + 3
    return nch, nseg, (nseg - 1) * B + 777


def _unit32(i, b, g, units):
    """fft_unit32 (fir_fft.hpp) restated."""
    base = i * g
    if g % 8 != 0 or base + g > units:
        return base + b
    return base + (b % 8) * (g // 8) + b // 8


def _walk(cus, units, nseg):
    """A launch of `units` units on `cus` CUs as the kernels walk it: rounds,
    swizzled rounds, units of the last round, and how many of the workgroups'
    unit-to-unit steps stay on a channel / move to another."""
    g = min(units, cus)
    rounds = -(-units // g)
    swizzled = sum(1 for i in range(rounds) if g % 8 == 0 and i * g + g <= units)
    stays = moves = 0
    seen = set()
    for b in range(g):
        prev = None
        for i in range(rounds + 1):
            u = _unit32(i, b, g, units)
            if u >= units:
                break
            seen.add(u)
            ch = u // nseg
            if prev is not None:
                stays += ch == prev
                moves += ch != prev
            prev = ch
    assert len(seen) == units
    return dict(rounds=rounds, swizzled=swizzled, tail=units - (rounds - 1) * g, stays=stays, moves=moves)


def _assert_case(case, cus, nch, nseg):
    """The property each case is named for, on this device."""
    units = nch * nseg
    w = _walk(cus, units, nseg)
    full = units // cus
    assert w["swizzled"] == (full if cus % 8 == 0 else 0), w
    if case == "tail1":
        assert units == cus + 1 and w["rounds"] == 2 and w["tail"] == 1 and w["moves"] == 1, w
    elif case == "exact2":
        assert units == 2 * cus and w["rounds"] == 2 and w["tail"] == cus, w
        assert w["swizzled"] == (2 if cus % 8 == 0 else 0), w
    elif case == "rounds3":
        assert 2 * cus < units < 3 * cus and units % cus and w["rounds"] == 3, w
        assert nseg < cus and w["moves"] >= cus, w  # round 0 -> 1 is + cus units: always another channel
    else:
        assert nch == 2 and units > 2 * cus and w["rounds"] >= 3, w
        assert w["stays"] > w["moves"] > 0, w
    return w


def _input(nch, n):
    import synth
    x = synth.file_buffer(nch, n, FS, file=FILE_ID, bits=24)
    scale = (0.2 + 0.7 * np.arange(nch) / nch).astype(np.float32)
    x = np.ascontiguousarray(x * scale[:, None], np.float32)
    zero_ch = nch // 2 if nch >= 3 else None
    if zero_ch is not None:
        x[zero_ch] = 0.0
    return x, zero_ch


def _launch(torch, flt, dx, nch, n, nrm=None):
    """Outputs [0, n) of every channel through lcfir_filter_window_dev (nrm:
    lcfir_filter_window_norm_dev's (buffer, count, peaks, npeak, force)) into
    rows of n + PAD floats preset to SENTINEL, per-channel peaks; returns the
    whole rows and the peaks."""
    dy = torch.full((nch, n + PAD), SENTINEL, dtype=torch.float32, device="cuda")
    dpk = torch.zeros(nch, dtype=torch.float32, device="cuda")
    if nrm is None:
        flt.filter_window_dev(dx, 0, n, n, n, nch, dy, 0, n + PAD, 0, n, dpk, peak_stride=1)
    else:
        flt.filter_window_norm_dev(dx, 0, n, n, n, nch, dy, 0, n + PAD, 0, n, dpk, 1, *nrm)
    torch.cuda.synchronize()
    return dy.cpu().numpy(), dpk.cpu().numpy()


def _single_round_launch(cus, B, nch, nseg):
    """chunk / max_units under which no launch of an nch x nseg grid has more
    than cus units (fft_launch: channel groups of max_units // chunk segments,
    at least one channel; fft_launch_group: chunks of whole segments)."""
    m = max(1, cus // 2)
    k = min(nseg, m)
    group = max(1, min(nch, m // k))
    assert group * k <= cus and k * B >= 4096  # a chunk below 4096 outputs is ignored (fft_chunk)
    return dict(chunk=k * B, max_units=m)


def _oracle_points(n, B, nseg, half, budget, rng):
    """Positions of one channel: every seam point, both ends and 64 random
    positions always; the other edge outputs and 448 more random positions
    thinned evenly to `budget`."""
    seams = (np.arange(1, nseg)[:, None] * B + np.arange(-2, 2)).ravel()
    must = np.r_[seams, np.arange(min(n, 64)), np.arange(max(0, n - 64), n), rng.integers(0, n, 64)]
    must = np.unique(must[(must >= 0) & (must < n)])
    edge = half + 64
    pool = np.r_[np.arange(min(n, edge)), np.arange(max(0, n - edge), n), rng.integers(0, n, 448)]
    pool = np.setdiff1d(pool, must)
    room = max(64, budget - must.size)
    if pool.size > room:
        pool = pool[np.unique(np.linspace(0, pool.size - 1, room).round().astype(np.int64))]
    return np.unique(np.r_[must, pool])


def _check_oracle(oracle_mod, taps, x, y, B, nseg, extra=()):
    """(b): y against the long-double oracle on as many evenly spaced channels
    as WORK pays for (at least the first, the last and two between)."""
    nch, n = x.shape
    half = (taps.size - 1) // 2
    points = int(WORK // taps.size)
    per_channel = min(n, 2 * (half + 64)) + 4 * (nseg - 1) + 512
    k = int(min(nch, max(4, points // per_channel)))
    chans = np.unique(np.linspace(0, nch - 1, k).round().astype(int))
    rng = np.random.default_rng(FILE_ID + nch + nseg)
    for c in chans:
        idx = _oracle_points(n, B, nseg, half, points // chans.size, rng)
        if len(extra):
            idx = np.unique(np.r_[idx, extra])
        ref, _ = oracle_mod.filter_points(x[c], taps, idx, oracle_mod.MODE_LD)
        assert rms(y[c][idx], ref) <= RMS_TOL, c
        assert max_ulps(y[c][idx], ref) <= 1, c
    return chans


_RUNS = {}  # the rounds3 runs the chunk and normalize tests build on


def _multi_round_run(dev, oracle_mod, form, case):
    """The multi-round launch of (form, case) with its preconditions asserted:
    taps, input, whole output rows, peaks, geometry."""
    if (form, case) in _RUNS:
        return _RUNS[form, case]
    torch, lc, cus = dev
    taps = _taps(oracle_mod, form)
    flt = _filter(lc, taps, form)
    B = flt.fft_units["outputs"]
    nch, nseg, n = _shape(case, cus, B)
    assert -(-n // B) == nseg and B >= 4096
    walk = _assert_case(case, cus, nch, nseg)
    x, zero_ch = _input(nch, n)
    dx = torch.from_numpy(x).cuda()
    rows, pk = _launch(torch, flt, dx, nch, n)
    print(f"\n{form} {case}: cus={cus} B={B} nch={nch} nseg={nseg} n={n} units={nch * nseg} {walk}")
    run = dict(taps=taps, x=x, dx=dx, rows=rows, pk=pk, B=B, nch=nch, nseg=nseg, n=n, zero_ch=zero_ch, cus=cus)
    if case == "rounds3" and form in ("l16_sym", "l16_general", "l16_parts", "l32_reg"):
        _RUNS[form, case] = run
    return run


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("form", list(FORMS))
def test_multi_round_launch(dev, oracle_mod, form, case):
    """One launch of more units than CUs: (a) bit-identical to single-round
    launches of the same plan, (b) the long-double oracle at every seam, the
    edges and random positions, (c) peaks, (d) no store outside the outputs;
    a channel of zeros stays zeros with peak 0."""
    torch, lc, cus = dev
    r = _multi_round_run(dev, oracle_mod, form, case)
    nch, nseg, n, B = r["nch"], r["nseg"], r["n"], r["B"]
    rows, pk, x = r["rows"], r["pk"], r["x"]
    y = rows[:, :n]
    assert np.all(rows[:, n:] == SENTINEL)  # (d)
    # (a) the same plan in launches of at most cus units each
    one = _filter(lc, r["taps"], form, **_single_round_launch(cus, B, nch, nseg))
    assert one.fft_units["outputs"] == B
    rows1, pk1 = _launch(torch, one, r["dx"], nch, n)
    assert np.all(rows1[:, n:] == SENTINEL)
    assert np.array_equal(rows, rows1)
    assert np.array_equal(pk, pk1)
    # (c)
    assert np.array_equal(pk, np.abs(y).max(axis=1))
    if r["zero_ch"] is not None:
        assert not y[r["zero_ch"]].any() and pk[r["zero_ch"]] == 0.0
        assert np.all(np.delete(pk, r["zero_ch"]) > 0.0)
    # (b)
    chans = _check_oracle(oracle_mod, r["taps"], x, y, B, nseg)
    assert {0, nch - 1} <= set(chans.tolist())


@pytest.mark.parametrize("form", ["l16_sym", "l16_parts"])
def test_chunks_of_several_rounds(dev, oracle_mod, form):
    """The rounds3 grid split into two launch chunks that are each still
    multi-round (seg0 != 0 in rounds >= 1 of the second; a partitioned filter
    restarts its f64 partial sums there): bytes and peaks of the unchunked
    launch, the oracle around the chunk seam and at every segment seam."""
    torch, lc, cus = dev
    r = _multi_round_run(dev, oracle_mod, form, "rounds3")
    nch, nseg, n, B = r["nch"], r["nseg"], r["n"], r["B"]
    k = -(-nseg // 2)
    assert k * nch > cus and (nseg - k) * nch > cus and k * B >= 4096
    flt = _filter(lc, r["taps"], form, chunk=k * B)
    rows, pk = _launch(torch, flt, r["dx"], nch, n)
    assert np.array_equal(rows, r["rows"]) and np.array_equal(pk, r["pk"])
    assert np.array_equal(pk, np.abs(rows[:, :n]).max(axis=1))
    _check_oracle(oracle_mod, r["taps"], r["x"], rows[:, :n], B, nseg, extra=k * B + np.arange(-8, 8))


@pytest.mark.parametrize("which", ["full", "short_tail", "early_units"])
@pytest.mark.parametrize("form", ["l16_sym", "l16_general", "l32_reg"])
def test_fused_normalize_in_later_rounds(dev, oracle_mod, form, which):
    """A previous file's normalize carried by the rounds3 launch: slices of
    units in every round (full: count = units x nrm_floats, the fusable limit),
    a last unit cut short with a 1..3-float tail (short_tail), and later
    rounds whose slices start past count and must touch nothing (early_units).
    Fused (nrm_stats), the filter's rows and peaks equal to the plain call's,
    the rescaled buffer equal to normalize_dev's and to (float)((double)v *
    (1.0 / (double)pk)) under the ProcessFile.cp:98-101 decision, the guard
    floats around the buffer untouched."""
    torch, lc, cus = dev
    r = _multi_round_run(dev, oracle_mod, form, "rounds3")
    nch, n, units = r["nch"], r["n"], r["nch"] * r["nseg"]
    probe = _filter(lc, r["taps"], form)
    cap = probe.fft_units["nrm_floats"]
    blk = 2048 if probe.fft_units["kernel"] == "l32_reg" else 1024
    assert cap > 0 and cap % blk == 0 and units > 2 * cus
    count = {"full": units * cap, "short_tail": units * cap - blk - 5, "early_units": int(1.3 * cus * blk) // 4 * 4 + 3}[which]
    per = -(-count // units)
    slice_ = -(-per // blk) * blk  # fft_launch_one: whole blocks per unit
    if which == "early_units":
        # round 1 starts inside the buffer; the last cus units (the whole last round) start past its end
        assert slice_ == blk and cus * slice_ < count < (units - cus) * slice_ and count % 4 == 3
    else:
        assert slice_ == cap and count % 4 == (0 if which == "full" else 3)
        assert (units - 1) * slice_ < count <= units * slice_  # the last unit of the last round has floats
    prev = (np.random.default_rng(count).standard_normal(count + 8) * 0.3).astype(np.float32)
    for peaks, force in (([0.75, 1.7], False), ([0.5], False)):
        pkmax = np.float32(max(peaks))
        scaled = (pkmax > 1.0 or force) and pkmax > 0.0
        want = prev.copy()
        if scaled:
            want[4:4 + count] = (prev[4:4 + count].astype(np.float64) * (1.0 / np.float64(pkmax))).astype(np.float32)
        dppk = torch.tensor(peaks, dtype=torch.float32, device="cuda")
        # fused into the filter launch
        buf = torch.from_numpy(prev.copy()).cuda()
        view = buf[4:4 + count]
        assert view.data_ptr() % 16 == 0
        flt = _filter(lc, r["taps"], form)
        rows, pk = _launch(torch, flt, r["dx"], nch, n, nrm=(view, count, dppk, len(peaks), force))
        assert flt.nrm_stats == {"fused": 1, "separate": 0}, (peaks, flt.nrm_stats)
        assert np.array_equal(rows, r["rows"]) and np.array_equal(pk, r["pk"]), peaks
        got = buf.cpu().numpy()
        # its own pass
        buf2 = torch.from_numpy(prev.copy()).cuda()
        lc.normalize_dev(buf2[4:4 + count], count, 1, count, dppk, len(peaks), force)
        torch.cuda.synchronize()
        sep = buf2.cpu().numpy()
        assert np.array_equal(got[:4], prev[:4]) and np.array_equal(got[4 + count:], prev[4 + count:]), peaks
        assert np.array_equal(got, sep), peaks
        assert np.array_equal(got, want), peaks
        assert scaled == (not np.array_equal(got, prev)), peaks
