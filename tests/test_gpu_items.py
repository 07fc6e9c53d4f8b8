"""GPU tests of item sets (lcfir_items_*): a batch of files of different
lengths filtered in one launch per group of equal unit count.

The expected value is always the existing per-file entry point on the same
build (lcfir_filter_channels_dev with its fused per-channel peaks,
lcfir_normalize_dev, lcfir_decode_pcm_dev, lcfir_encode_pcm_scaled_dev), never
the code under test, and the comparison is bit for bit: no tolerance.  A
sample of outputs also goes against the long-double oracle under the parity
tests' bar (<= 1 f32 ulp, RMS <= 1e-9), so the comparison is not GPU against
GPU only.  The oracle positions are drawn from every row's first and last
`half` outputs (always the first and last two and both ends of each region)
and from both sides of every segment seam: a few hundred per filter, since all
of them would be 2 x 19 200 long-double dot products of 38 401 taps per row.

Files per filter, U = the ctx's unit: n in {0, 1, half, U - 1, U, U + 1, 2U,
2U + 37, 3U - 1, U + 1 again}, channels cycling 1, 2, 3; seeded uniform noise
on +-0.4 of full scale with one file x4, one of zeros, one at 1e-3.  A low-cut
passes noise almost unchanged (its centre tap is ~1, the others sum to about
-1 but average a bounded random input away), so a file's peak is close to its
input's: ~0.4 for the plain files, ~1.6 for the x4 file -- the only one above
1, which the tests assert on the expected values.
"""
import ctypes

import numpy as np
import pytest

import pcm_ref

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-9
FORMATS = ["s16le", "s24le", "s32le", "f32le", "s16be", "s24be", "s32be", "f32be"]
# (name, taps, method, tuning, family, perturb)
FILTERS = [
    ("direct15", 15, "direct", None, None, 0.0),
    ("l16_201", 201, "fft", None, None, 0.0),
    ("reg_4001", 4001, "fft", None, None, 0.0),
    ("lds_4001", 4001, "fft", None, "lds", 0.0),
    ("park_general_8001", 8001, "fft", dict(seg_len=32768, zero_phase=False), None, 1e-9),
    ("parts_38401", 38401, "fft", None, None, 0.0),
]
LOUD, ZERO, QUIET = 6, 4, 5  # the files scaled x4, all zeros, at 1e-3


@pytest.fixture(scope="module")
def lc():
    import lcfir
    assert lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


def make_filter(lc, oracle_mod, ntaps, method, tuning, family, perturb):
    taps = oracle_mod.design_lowcut(20.0, 48000.0, ntaps)
    if perturb:
        taps = taps + perturb * np.linspace(-1.0, 1.0, ntaps)  # a visible antisymmetric part
    flt = lc.Filter(taps, method=method)
    if tuning:
        flt.set_fft_tuning(**tuning)
    if family:
        flt.set_fft_family(family)
    return taps, flt


def unit_of(flt):
    return flt.fft_units["outputs"] if flt.method == "fft" else 4096


def make_files(unit, half, seed):
    rng = np.random.default_rng(seed)
    ns = [0, 1, half, unit - 1, unit, unit + 1, 2 * unit, 2 * unit + 37, 3 * unit - 1, unit + 1]
    files = []
    for f, n in enumerate(ns):
        nch = 1 + f % 3
        x = (rng.integers(-2**23, 2**23, size=(nch, n)) / 2.0**23 * 0.4).astype(np.float32)
        if f == LOUD:
            x *= np.float32(4.0)
        elif f == ZERO:
            x[:] = 0.0
        elif f == QUIET:
            x *= np.float32(1e-3)
        files.append(np.ascontiguousarray(x))
    return files


def h2d(lc, ptr, a):
    a = np.ascontiguousarray(a)
    if a.nbytes:
        lc._check(lc.load().lcfir_memcpy_h2d(ptr, a.ctypes.data, a.nbytes, None))
        lc.sync()


def d2h(lc, ptr, shape, dtype=np.float32):
    out = np.empty(shape, dtype)
    if out.nbytes:
        lc._check(lc.load().lcfir_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None))
    return out


def per_file_reference(lc, flt, x):
    """The existing per-file pipeline: (y, per-channel fused peaks, y after
    lcfir_normalize_dev without force, y after it with force)."""
    nch, n = x.shape
    if n == 0:
        e = np.zeros((nch, 0), np.float32)
        return e, np.zeros(nch, np.float32), e, e
    dx = lc.DeviceBuffer.from_array(x)
    dy = lc.DeviceBuffer(x.nbytes)
    dpk = lc.DeviceBuffer(4 * nch)
    lc.peak_reset_dev(dpk, nch)
    flt.filter_channels_dev(dx, n, nch, n, dy, n, dpk)
    lc.sync()
    y = dy.download((nch, n))
    pk = dpk.download(nch)
    lc.normalize_dev(dy, n, nch, n, dpk, nch, False)
    lc.sync()
    y0 = dy.download((nch, n))
    dy.upload(y)
    lc.normalize_dev(dy, n, nch, n, dpk, nch, True)
    lc.sync()
    y1 = dy.download((nch, n))
    for b in (dx, dy, dpk):
        b.free()
    return y, pk, y0, y1


class Batch:
    """An item set with its files uploaded, and helpers to read it back."""

    def __init__(self, lc, flt, files):
        self.lc, self.files = lc, files
        self.n = [x.shape[1] for x in files]
        self.nch = [x.shape[0] for x in files]
        self.items = lc.ItemSet(flt, self.n, self.nch)
        self.dpk = lc.DeviceBuffer(4 * len(files))
        for f, x in enumerate(files):
            dx, _, stride = self.items.file(f)
            for c in range(x.shape[0] if x.size else 0):
                h2d(lc, dx + 4 * c * stride, x[c])  # only [0, n_f) of a row is ever written

    def run(self, peaks=True):
        self.lc.peak_reset_dev(self.dpk, len(self.files))
        self.items.filter_dev(self.dpk if peaks else None)
        self.lc.sync()

    def peaks(self):
        return self.dpk.download(len(self.files))

    def rows(self, f, which=1, full=False):
        """File f's rows of the input (0) or output (1) arena: [0, n_f), or whole rows."""
        ptr = self.items.file(f)[which]
        stride = self.items.file(f)[2]
        if ptr is None:
            return np.zeros((self.nch[f], 0), np.float32)
        a = d2h(self.lc, ptr, (self.nch[f], stride))
        return a if full else np.ascontiguousarray(a[:, :self.n[f]])

    def outputs(self):
        return [self.rows(f) for f in range(len(self.files))]

    def close(self):
        self.items.close()
        self.dpk.free()


@pytest.fixture(scope="module", params=FILTERS, ids=[f[0] for f in FILTERS])
def case(request, lc, oracle_mod):
    """Per filter, computed once and left unchanged: the files, the per-file
    reference results and the item set's results after one and two runs."""
    name, ntaps, method, tuning, family, perturb = request.param
    taps, flt = make_filter(lc, oracle_mod, ntaps, method, tuning, family, perturb)
    unit, half = unit_of(flt), (ntaps - 1) // 2
    files = make_files(unit, half, seed=ntaps)
    refs = [per_file_reference(lc, flt, x) for x in files]
    b = Batch(lc, flt, files)
    b.run()
    y_first, pk_first = b.outputs(), b.peaks()
    b.run()
    y_second, pk_second = b.outputs(), b.peaks()
    b.items.normalize_dev(b.dpk, False)
    lc.sync()
    y_norm0 = b.outputs()
    b.run()
    b.items.normalize_dev(b.dpk, True)
    lc.sync()
    y_norm1 = b.outputs()
    info = b.items.info()
    b.close()
    return dict(name=name, taps=taps, flt=flt, unit=unit, half=half, files=files, refs=refs, info=info,
                y=y_first, pk=pk_first, y2=y_second, pk2=pk_second, y_norm0=y_norm0, y_norm1=y_norm1)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_kernel_forms(case):
    """The six filters run the six forms the issue names."""
    flt, name = case["flt"], case["name"]
    if name == "direct15":
        assert flt.method == "direct" and case["unit"] == 4096
        return
    info, units = flt.fft_info, flt.fft_units
    want = {"l16_201": (16384, 1, True, "l16"), "reg_4001": (32768, 1, True, "l32_reg"),
            "lds_4001": (None, 1, True, None), "park_general_8001": (32768, 1, False, "l32_park"),
            "parts_38401": (None, 2, None, None)}[name]
    if want[0]:
        assert info["seg_len"] == want[0]
    assert info["parts"] == want[1]
    if want[2] is not None:
        assert info["zero_phase"] == want[2]
    if want[3]:
        assert units["kernel"] == want[3]
    if name == "lds_4001":
        assert units["kernel"] in ("l16", "l32_park")
    assert case["unit"] == units["outputs"]


def test_outputs_equal_per_file_calls(case):
    for f, (ref, y) in enumerate(zip(case["refs"], case["y"])):
        assert same_bits(y, ref[0]), (case["name"], f)


def test_peaks_equal_per_file_fused_peaks(case):
    want = np.array([r[1].max() if r[1].size and r[0].size else 0.0 for r in case["refs"]], np.float32)
    assert same_bits(case["pk"], want), (case["pk"], want)
    # the inputs exercise the decision: exactly the x4 file peaks above 1, the zero file at 0
    assert [f for f in range(len(want)) if want[f] > 1.0] == [LOUD]
    assert want[ZERO] == 0.0 and 0.0 < want[QUIET] < 1e-2


def test_second_run_gives_the_same_bytes(case):
    """With byte identity to the per-file calls this shows the rows' padding is
    still zero: a gap written by the first run would change the second run's
    tails."""
    for f, (a, b) in enumerate(zip(case["y"], case["y2"])):
        assert same_bits(a, b), (case["name"], f)
    assert same_bits(case["pk"], case["pk2"])


def test_group_count(case):
    unit = case["unit"]
    keys = {-(-x.shape[1] // unit) for x in case["files"] if x.size}
    assert case["info"]["groups"] == len(keys) == 3
    assert case["info"]["launches"] == 3
    assert case["info"]["rows"] == sum(x.shape[0] for x in case["files"] if x.size)


def test_normalize_equals_per_file_normalize(case):
    for f, ref in enumerate(case["refs"]):
        assert same_bits(case["y_norm0"][f], ref[2]), (case["name"], f, "no force")
        assert same_bits(case["y_norm1"][f], ref[3]), (case["name"], f, "force")
        changed = not same_bits(ref[2], ref[0])
        assert changed == (f == LOUD), f  # without force only the x4 file changes
    assert same_bits(case["refs"][ZERO][3], case["refs"][ZERO][0])  # the zero file never changes
    assert not same_bits(case["refs"][QUIET][3], case["refs"][QUIET][0])  # force rescales a quiet file


def max_ulps(a, b, floor=1e-12):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    close = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= floor
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.where(close, 0, np.abs(ia - ib)).max()) if a.size else 0


def test_outputs_against_the_oracle(case, oracle_mod):
    taps, unit, half = case["taps"], case["unit"], case["half"]
    rng = np.random.default_rng(len(taps))
    got, want = [], []
    for f, x in enumerate(case["files"]):
        n = x.shape[1]
        if n == 0:
            continue
        for c in range(x.shape[0]):
            head, tail = min(half, n), max(0, n - half)
            pos = [0, 1, head - 1, head, tail - 1, tail, n - 2, n - 1]
            pos += rng.integers(0, max(1, head), 4).tolist() + rng.integers(tail, n, 4).tolist()
            for seam in range(unit, n, unit):
                pos += [seam - 1, seam]
            idx = np.unique(np.clip(np.array(pos, np.int64), 0, n - 1))
            ref, _ = oracle_mod.filter_points(x[c], taps, idx, oracle_mod.MODE_LD)
            got.append(case["y"][f][c][idx])
            want.append(ref)
            if case["name"] == "direct15":
                fma, _ = oracle_mod.filter_points(x[c], taps, idx, oracle_mod.MODE_FMA)
                assert np.array_equal(case["y"][f][c][idx], fma), (f, c)
    got, want = np.concatenate(got), np.concatenate(want)
    assert 150 <= got.size <= 1000  # "a few hundred"
    d = got.astype(np.float64) - want
    assert float(np.sqrt(np.mean(d * d))) <= RMS_TOL
    assert max_ulps(got, want) <= 1


# ---- codec -------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec_case(lc, oracle_mod):
    """Mixed formats in one batch: the ten files cycle through all eight
    lcfir_pcm_format values; payloads concatenated with an odd gap between
    them, so most start unaligned."""
    taps, flt = make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
    files = make_files(4096, 7, seed=99)
    fmts = [FORMATS[f % len(FORMATS)] for f in range(len(files))]
    payloads = [pcm_ref.np_encode(x, fmt) for x, fmt in zip(files, fmts)]
    offs, blob = [], b"\xa5"
    for p in payloads:
        offs.append(len(blob))
        blob += p + b"\x5a" * 3
    return dict(flt=flt, files=files, fmts=fmts, payloads=payloads, offs=offs, blob=blob)


def test_decode_equals_per_file_decode(lc, codec_case):
    cc = codec_case
    files = cc["files"]
    b = Batch(lc, cc["flt"], [np.zeros_like(x) for x in files])  # rows start as zeros
    d_blob = lc.DeviceBuffer.from_array(np.frombuffer(cc["blob"], np.uint8))
    b.items.decode_pcm_dev(d_blob, cc["offs"], cc["fmts"])
    lc.sync()
    for f, x in enumerate(files):
        nch, n = x.shape
        rows = b.rows(f, which=0, full=True)
        if n == 0:
            continue
        d_in = lc.DeviceBuffer.from_array(np.frombuffer(cc["payloads"][f], np.uint8))
        d_out = lc.DeviceBuffer(4 * nch * n)
        lc.decode_pcm_dev(d_in, cc["fmts"][f], nch, n, d_out, n)
        lc.sync()
        want = d_out.download((nch, n))
        assert same_bits(rows[:, :n], want), f
        assert same_bits(want, pcm_ref.np_decode(cc["payloads"][f], cc["fmts"][f], nch)), f
        assert not rows[:, n:].any(), f  # the padding after decode is still zero
        d_in.free()
        d_out.free()
    # the whole input arena: nothing but the rows' [0, n_f) is non-zero
    plan = lc.ItemSet.plan(4096, b.n, b.nch)
    assert plan["arena_floats"] == b.items.info()["arena_floats"]
    live = next(f for f, x in enumerate(files) if x.size)
    base = b.items.file(live)[0] - 4 * int(plan["file_offset"][live])
    arena = d2h(lc, base, plan["arena_floats"])
    mask = np.zeros(arena.size, bool)
    for f, x in enumerate(files):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            mask[o:o + x.shape[1]] = True
    assert not arena[~mask].any()
    b.close()
    d_blob.free()


@pytest.mark.parametrize("force", [False, True])
def test_encode_scaled_equals_per_file_encode(lc, codec_case, force):
    cc = codec_case
    files = cc["files"]
    b = Batch(lc, cc["flt"], files)
    b.run()
    pk = b.peaks()
    assert pk[LOUD] > 1.0
    y = b.outputs()
    d_blob = lc.DeviceBuffer.from_array(np.full(len(cc["blob"]), 0x77, np.uint8))
    b.items.encode_pcm_scaled_dev(b.dpk, force, d_blob, cc["offs"], cc["fmts"])
    lc.sync()
    got = d_blob.download(len(cc["blob"]), np.uint8)
    written = np.zeros(got.size, bool)
    for f, x in enumerate(files):
        nch, n = x.shape
        if n == 0:
            continue
        nb = lc.pcm_bytes(cc["fmts"][f]) * nch * n
        d_y = lc.DeviceBuffer.from_array(y[f])
        d_pk = lc.DeviceBuffer.from_array(pk[f:f + 1])
        d_ref = lc.DeviceBuffer(nb)
        lc.encode_pcm_scaled_dev(d_y, n, nch, n, cc["fmts"][f], d_pk, 1, force, d_ref)
        lc.sync()
        want = d_ref.download(nb, np.uint8)
        o = cc["offs"][f]
        assert np.array_equal(got[o:o + nb], want), (f, cc["fmts"][f])
        written[o:o + nb] = True
        for d in (d_y, d_pk, d_ref):
            d.free()
    assert np.all(got[~written] == 0x77)  # nothing outside the payloads is touched
    for f in range(len(files)):
        assert same_bits(b.rows(f), y[f])  # the output rows are left unscaled
    b.close()
    d_blob.free()


# ---- graph capture -------------------------------------------------------------
def test_graph_capture_replays_the_same_bytes(lc, oracle_mod):
    """4 001 taps, three files: filter + peaks + normalize captured after an
    eager call on the stream (which sizes the ctx's scratch), replayed twice."""
    import torch
    taps, flt = make_filter(lc, oracle_mod, 4001, "fft", None, None, 0.0)
    unit = unit_of(flt)
    rng = np.random.default_rng(5)
    files = [(rng.standard_normal((nch, n)) * s).astype(np.float32)
             for nch, n, s in [(2, unit + 11, 0.1), (1, 777, 0.1), (3, 2 * unit + 5, 0.6)]]
    b = Batch(lc, flt, files)
    s = torch.cuda.Stream()
    pk = torch.zeros(3, dtype=torch.float32, device="cuda")

    def step():
        lc.peak_reset_dev(pk, 3, s.cuda_stream)
        b.items.filter_dev(pk, s.cuda_stream)

    step()
    torch.cuda.synchronize()
    want, want_pk = b.outputs(), pk.cpu().numpy().copy()
    for f, x in enumerate(files):
        assert same_bits(want[f], per_file_reference(lc, flt, x)[0]), f
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    for _ in range(2):
        for f in range(3):  # poison the outputs: the bytes must come from the replay
            _, dy, stride = b.items.file(f)
            h2d(lc, dy, np.full(files[f].shape[0] * stride, np.nan, np.float32))
        pk.fill_(7.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        for f in range(3):
            assert same_bits(b.rows(f), want[f]), f
        assert same_bits(pk.cpu().numpy(), want_pk)
    del g
    b.close()


# ---- arguments -----------------------------------------------------------------
def test_bad_arguments_are_reported(lc, oracle_mod):
    lib = lc.load()
    _, flt = make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
    n = np.array([100, 50], np.int64)
    nch = np.array([1, 2], np.int32)
    h = ctypes.c_void_p()
    assert lib.lcfir_items_create(flt.ctx, None, nch.ctypes.data, 2, ctypes.byref(h)) == lc.EINVAL
    assert lib.lcfir_last_error() and not h.value
    assert lib.lcfir_items_create(flt.ctx, n.ctypes.data, nch.ctypes.data, 2, None) == lc.EINVAL
    bad = np.array([100, -1], np.int64)
    assert lib.lcfir_items_create(flt.ctx, bad.ctypes.data, nch.ctypes.data, 2, ctypes.byref(h)) == lc.EINVAL
    assert b"negative" in lib.lcfir_last_error() and not h.value
    items = lc.ItemSet(flt, n, nch)
    dx, dy, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    for f in (-1, 2):
        rc = lib.lcfir_items_file(items._h, f, ctypes.byref(dx), ctypes.byref(dy), ctypes.byref(st))
        assert rc == lc.EINVAL and b"out of range" in lib.lcfir_last_error()
    assert lib.lcfir_items_file(items._h, 0, None, ctypes.byref(dy), ctypes.byref(st)) == lc.EINVAL
    assert lib.lcfir_items_file(None, 0, ctypes.byref(dx), ctypes.byref(dy), ctypes.byref(st)) == lc.EINVAL
    assert lib.lcfir_items_info(items._h, None, None, None, None) == lc.EINVAL
    assert lib.lcfir_items_filter_dev(None, None, None) == lc.EINVAL
    assert b"null" in lib.lcfir_last_error()
    assert lib.lcfir_items_normalize_dev(items._h, None, 0, None) == lc.EINVAL
    off = np.zeros(2, np.int64)
    fmt = np.array([1, 1], np.int32)
    d = lc.DeviceBuffer(1024)
    assert lib.lcfir_items_decode_pcm_dev(items._h, None, off.ctypes.data, fmt.ctypes.data, None) == lc.EINVAL
    assert lib.lcfir_items_decode_pcm_dev(items._h, d.ptr, None, fmt.ctypes.data, None) == lc.EINVAL
    assert lib.lcfir_items_encode_pcm_scaled_dev(items._h, None, 0, d.ptr, off.ctypes.data, fmt.ctypes.data,
                                                 None) == lc.EINVAL
    badfmt = np.array([1, 99], np.int32)
    assert lib.lcfir_items_decode_pcm_dev(items._h, d.ptr, off.ctypes.data, badfmt.ctypes.data, None) == lc.EINVAL
    assert b"format" in lib.lcfir_last_error()
    negoff = np.array([0, -4], np.int64)
    assert lib.lcfir_items_decode_pcm_dev(items._h, d.ptr, negoff.ctypes.data, fmt.ctypes.data, None) == lc.EINVAL
    with pytest.raises(ValueError):
        lc.ItemSet(flt, [1, 2], [1])
    # a batch without a single row is legal and launches nothing
    empty = lc.ItemSet(flt, [0, 5], [2, 0])
    assert empty.info() == {"groups": 0, "launches": 0, "rows": 0, "arena_floats": 0}
    assert empty.file(0) == (None, None, 0)
    empty.filter_dev(None)
    lc.sync()
    empty.close()
    items.close()
    d.free()
