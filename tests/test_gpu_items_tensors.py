"""GPU tests of the item set's tensor path: lcfir_items_gather_dev,
lcfir_items_scatter_scaled_dev (csrc/items.hpp: items_gather_kernel,
items_scatter_scaled_kernel) and batch.TensorBatch / batch.filter_tensors.

The expected value is always the per-file entry point on the same build
(tests/test_gpu_items.py's per_file_reference: lcfir_filter_channels_dev, then
lcfir_normalize_dev without and with force), bit for bit, no tolerance.

Forms, the smallest that reach each launch path of the per-group filter step:
the direct kernel (15 taps, unit 4 096), the L = 16 384 kernel (201 taps,
B = 16 184) and the register kernel (4 001 taps, B = 28 768).  Files per form,
B = the form's unit: n in {0, 1, 3, B - 1, B, B + 1, 2B + 5, 3B - 2}, channels
cycling 1, 2, 3 (three groups), one file x4 and one at 1e-3.  Sources and
destinations are carved out of one larger tensor each, file f starting
f % 4 floats past a 16-byte boundary, so both the float4 and the dword path
run on either side; file 4 (two channels) has a channel stride of n + 5; file
3 is passed as a 1-D tensor.
"""
import numpy as np
import pytest

import test_gpu_items as gi
from test_gpu_items import d2h, per_file_reference, same_bits

pytestmark = pytest.mark.gpu

# name: taps, method, the unit the plan must give
FORMS = {
    "direct15": (15, "direct", 4096),
    "l16_zero_201": (201, "fft", 16184),
    "reg_4001": (4001, "fft", 28768),
}
LOUD, QUIET, STRIDED, FLAT = 6, 5, 4, 3
SENTINEL = np.uint32(0xDEADBEEF)
GAP = 8  # floats between two files of a pool (>= the 1-3 floats either side of an unaligned row)
# a signalling NaN with a payload, -0.0, the smallest subnormal
SPECIALS = np.array([0x7FA00001, 0x80000000, 0x00000001], np.uint32)


@pytest.fixture(scope="module")
def lc():
    import torch  # before lcfir: one HIP runtime in the process
    import lcfir
    assert torch.cuda.is_available() and lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


def make_files(unit, seed):
    rng = np.random.default_rng(seed)
    ns = [0, 1, 3, unit - 1, unit, unit + 1, 2 * unit + 5, 3 * unit - 2]
    files = []
    for f, n in enumerate(ns):
        x = (rng.integers(-2**23, 2**23, size=(1 + f % 3, n)) / 2.0**23 * 0.4).astype(np.float32)
        if f == LOUD:
            x *= np.float32(4.0)
        elif f == QUIET:
            x *= np.float32(1e-3)
        files.append(np.ascontiguousarray(x))
    return files


class Pool:
    """One device tensor with a block per file: file f's channel 0 starts
    f % 4 floats past a 16-byte boundary, channels `stride` apart (n, or n + 5
    for the strided file), GAP floats or more between blocks."""

    def __init__(self, torch, files, fill_bits):
        self.torch = torch
        self.shapes = [x.shape for x in files]
        self.stride = [x.shape[1] + (5 if f == STRIDED else 0) for f, x in enumerate(files)]
        self.off, at = [], GAP
        for f, (nch, n) in enumerate(self.shapes):
            at = -(-at // 4) * 4 + f % 4
            self.off.append(at)
            at += (nch - 1) * self.stride[f] + n + GAP
        self.size = at + GAP
        self.t = torch.from_numpy(np.full(self.size, fill_bits, np.uint32).view(np.float32).copy()).cuda()
        assert self.t.data_ptr() % 16 == 0

    def view(self, f):
        nch, n = self.shapes[f]
        v = self.torch.as_strided(self.t, (nch, n), (self.stride[f], 1), self.off[f])
        return v[0] if f == FLAT else v

    def views(self):
        return [self.view(f) for f in range(len(self.shapes))]

    def fill(self, files_bits):
        """upload per-file uint32 [nch][n] arrays into their blocks"""
        host = self.t.cpu().numpy().view(np.uint32).copy()
        for f, b in enumerate(files_bits):
            for c in range(b.shape[0]):
                o = self.off[f] + c * self.stride[f]
                host[o:o + b.shape[1]] = b[c]
        self.t.copy_(self.torch.from_numpy(host.view(np.float32)))

    def spans(self):
        ptrs = [self.t.data_ptr() + 4 * o if n and nch else 0 for o, (nch, n) in zip(self.off, self.shapes)]
        return ptrs, [s if n and nch else 0 for s, (nch, n) in zip(self.stride, self.shapes)]

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)

    def row_mask(self):
        m = np.zeros(self.size, bool)
        for f, (nch, n) in enumerate(self.shapes):
            for c in range(nch):
                o = self.off[f] + c * self.stride[f]
                m[o:o + n] = True
        return m

    def rows(self, f):
        nch, n = self.shapes[f]
        b = self.bits()
        return np.stack([b[self.off[f] + c * self.stride[f]:][:n] for c in range(nch)]).view(np.float32) \
            if nch else np.zeros((0, n), np.float32)


def arena_bits(lc, items, plan, which):
    live = next(f for f in range(len(plan["file_stride"])) if plan["file_stride"][f])
    base = items.file(live)[which] - 4 * int(plan["file_offset"][live])
    return d2h(lc, base, int(plan["arena_floats"]), np.uint32)


@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def case(request, lc, oracle_mod):
    """Per form, computed once and left unchanged: the per-file references; the
    input arena after a gather of sources with special bit patterns; the
    destination pools after scatters without and with force and without peaks;
    TensorBatch's outputs and peaks without and with normalize; filter_tensors'."""
    import torch
    import batch
    name = request.param
    ntaps, method, unit_want = FORMS[name]
    taps, flt = gi.make_filter(lc, oracle_mod, ntaps, method, None, None, 0.0)
    unit = gi.unit_of(flt)
    assert unit == unit_want, (name, unit)
    files = make_files(unit, seed=ntaps)
    n, nch = [x.shape[1] for x in files], [x.shape[0] for x in files]
    refs = [per_file_reference(lc, flt, x) for x in files]
    plan = lc.ItemSet.plan(unit, n, nch)
    assert plan["groups"] == 3

    # 1: gather of sources that hold special bit patterns
    special = [x.view(np.uint32).copy() for x in files]
    for b in special:
        if b.shape[1] >= 3:
            for c in range(b.shape[0]):
                b[c, [0, b.shape[1] // 2, b.shape[1] - 1]] = np.roll(SPECIALS, c)
    src = Pool(torch, files, SENTINEL)
    src.fill(special)
    items = lc.ItemSet(flt, n, nch)
    assert items.info()["arena_floats"] == plan["arena_floats"]
    ptrs, strides = src.spans()
    items.gather_dev(ptrs, strides)
    lc.sync()
    x_special = arena_bits(lc, items, plan, 0)
    src_after_special = src.bits().copy()

    # 2, 3: the finite files through gather, filter + peaks, scatters into sentinel pools
    src.fill([x.view(np.uint32) for x in files])
    items.gather_dev(ptrs, strides)
    dpk = torch.zeros(len(files), dtype=torch.float32, device="cuda")
    items.filter_dev(dpk)
    y_arena_before = None
    dst = {}
    for key, peaks, force in [("plain", None, True), ("norm0", dpk, False), ("norm1", dpk, True)]:
        pool = Pool(torch, files, SENTINEL)
        dp, ds = pool.spans()
        if key == "norm0":
            lc.sync()
            y_arena_before = arena_bits(lc, items, plan, 1)
        items.scatter_scaled_dev(peaks, force, dp, ds)
        lc.sync()
        dst[key] = pool
    y_arena_after = arena_bits(lc, items, plan, 1)
    x_arena = arena_bits(lc, items, plan, 0)
    pk_items = dpk.cpu().numpy()
    items.close()

    # TensorBatch on the same source views
    out = {}
    for normalize in (False, True):
        tb = batch.TensorBatch(flt, src.views(), normalize=normalize)
        for _ in range(2):  # steps are repeatable
            tb.step()
        torch.cuda.synchronize()
        out[normalize] = ([y.cpu().numpy() for y in tb.outputs], tb.peaks.cpu().numpy()[:len(files)].copy(),
                          [tuple(y.shape) for y in tb.outputs])
        tb.close()
    one_shot = [y.cpu().numpy() for y in batch.filter_tensors(flt, src.views(), normalize=True)]
    return dict(name=name, flt=flt, files=files, refs=refs, plan=plan, special=special, src=src,
                x_special=x_special, src_after_special=src_after_special, dst=dst, x_arena=x_arena,
                y_arena_before=y_arena_before, y_arena_after=y_arena_after, pk_items=pk_items, out=out,
                one_shot=one_shot)


def file_peaks(refs):
    return np.array([r[1].max() if r[1].size and r[0].size else 0.0 for r in refs], np.float32)


def test_gather_moves_bit_patterns_and_leaves_the_padding_zero(case):
    plan, arena = case["plan"], case["x_special"]
    mask = np.zeros(arena.size, bool)
    seen = set()
    for f, b in enumerate(case["special"]):
        for c in range(b.shape[0] if b.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            assert np.array_equal(arena[o:o + b.shape[1]], b[c]), (case["name"], f, c)
            mask[o:o + b.shape[1]] = True
            seen |= set(b[c].tolist()) & set(SPECIALS.tolist())
    assert seen == set(SPECIALS.tolist())  # the three patterns were in the sources
    assert mask.sum() == sum(b.size for b in case["special"])
    assert not arena[~mask].any()  # zero bits everywhere else
    # the second gather (finite files) rewrote the rows and nothing else
    arena2 = case["x_arena"]
    assert not arena2[~mask].any()
    for f, x in enumerate(case["files"]):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            assert np.array_equal(arena2[o:o + x.shape[1]], x[c].view(np.uint32)), (f, c)
    # the sources are only read
    src = case["src"]
    assert np.all(case["src_after_special"][~src.row_mask()] == SENTINEL)


def test_both_paths_ran(case):
    """The pools put rows on and off 16-byte boundaries, and one file strided."""
    src = case["src"]
    ptrs, strides = src.spans()
    live = [p for p in ptrs if p]
    assert {p % 16 for p in live} == {0, 4, 8, 12}
    assert strides[STRIDED] == case["files"][STRIDED].shape[1] + 5 and case["files"][STRIDED].shape[0] == 2
    assert src.view(FLAT).dim() == 1 and src.view(STRIDED).stride(0) == strides[STRIDED]


def test_tensor_batch_equals_per_file_calls(case):
    want_pk = file_peaks(case["refs"])
    assert [f for f in range(len(want_pk)) if want_pk[f] > 1.0] == [LOUD] and 0.0 < want_pk[QUIET] < 1e-2
    for normalize, which in ((False, 2), (True, 3)):
        ys, pk, shapes = case["out"][normalize]
        assert same_bits(pk, want_pk), (case["name"], normalize, pk, want_pk)
        for f, (y, ref) in enumerate(zip(ys, case["refs"])):
            want = ref[which][0] if f == FLAT else ref[which]
            assert same_bits(y, want), (case["name"], normalize, f)
        assert shapes == [tuple(v.shape) for v in case["src"].views()]
    # the flag matters: without it only the loud file is rescaled
    changed = [f for f, r in enumerate(case["refs"]) if r[0].size and not same_bits(r[2], r[3])]
    assert LOUD not in changed and QUIET in changed
    assert same_bits(case["pk_items"], want_pk)


def test_scatter_equals_per_file_normalize_and_writes_nothing_else(case):
    for key, which in (("plain", 0), ("norm0", 2), ("norm1", 3)):
        pool = case["dst"][key]
        for f, ref in enumerate(case["refs"]):
            assert same_bits(pool.rows(f), ref[which]), (case["name"], key, f)
        outside = pool.bits()[~pool.row_mask()]
        assert outside.size >= GAP * len(case["files"]) and np.all(outside == SENTINEL), (case["name"], key)
    # the output arena is left unscaled by the scatters
    assert np.array_equal(case["y_arena_before"], case["y_arena_after"])


def test_filter_tensors_equals_tensor_batch(case):
    ys = case["out"][True][0]
    assert len(case["one_shot"]) == len(ys)
    for f, (a, b) in enumerate(zip(case["one_shot"], ys)):
        assert same_bits(a, b), (case["name"], f)


def test_bad_spans_and_capture_are_refused(lc, oracle_mod):
    import torch
    _, flt = gi.make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
    n, nch = [100, 0, 50], [1, 2, 2]
    items = lc.ItemSet(flt, n, nch)
    pool = torch.zeros(1024, dtype=torch.float32, device="cuda")
    base = pool.data_ptr()
    good = ([base, 0, base + 4 * 200], [100, 0, 50])
    dpk = torch.zeros(3, dtype=torch.float32, device="cuda")

    def refused(ptrs, strides, match, stream=0):
        for call in (lambda: items.gather_dev(ptrs, strides, stream),
                     lambda: items.scatter_scaled_dev(dpk, False, ptrs, strides, stream)):
            with pytest.raises(lc.LcfirError, match=match) as e:
                call()
            assert e.value.code == lc.EINVAL

    items.gather_dev(*good)  # file 1 has no rows: its null pointer is skipped
    items.scatter_scaled_dev(None, False, *good)
    lc.sync()
    refused([0, 0, good[0][2]], good[1], "file 0: null")
    refused(good[0], [100, 0, 49], "file 2: channel stride")
    refused([base + 2, 0, good[0][2]], good[1], "file 0: pointer not 4-byte aligned")
    dx, dy, st = items.file(2)
    assert st == 100 and items.file(0)[1] == dy - 4 * 100  # file 0's rows open the arenas
    refused([base, 0, dx], good[1], "file 2: .*overlaps")                    # inside the input arena
    refused([dy - 4 * 199, 0, good[0][2]], good[1], "file 0: .*overlaps")   # its last float is the output arena's first
    with pytest.raises(ValueError):
        items.gather_dev([base], [100])
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        lc.peak_reset_dev(dpk, 3, s.cuda_stream)
        refused(good[0], good[1], "captured", s.cuda_stream)
    del g
    torch.cuda.synchronize()
    items.gather_dev(*good)  # and the item set still serves eager calls
    lc.sync()
    items.close()
