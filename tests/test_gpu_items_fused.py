"""GPU tests of the fused item-set filter launch: one launch of the plan's FFT
kernel in its item form walks a per-unit table over every row of every group
(include/lcfir.h, lcfir_items_filter_dev; csrc/fir_fft.hpp, fft_unit_decode).
The two LDS-column kernels have the item form (fir_fft_f64_kernel,
fir_fft32_f64_kernel); a register-kernel plan (fir_fft32r_kernel) stays on the
per-group launches and is pinned here as a fallback.  The per-group path is an
item set's default, so every test asks for the fused one (set_fusion("auto")).

The expected value is always the per-file entry point on the same build,
lcfir_filter_channels_dev with its fused peaks, compared bit for bit with no
tolerance.  A sample of outputs -- row edges and both sides of every segment
seam -- is also held to the long-double oracle under the parity bar (<= 1 f32
ulp, RMS <= 1e-9), as tests/test_gpu_items.py does, whose helpers (files,
per-file reference, Batch) this module reuses.

Standard files per form, U = the plan's outputs per unit: n in {0, 1, half,
U - 1, U, U + 1, 2U, 2U + 37, 3U - 1, U + 1}, channels cycling 1, 2, 3, one
file x4, one of zeros, one at 1e-3: 33 units in three groups.

Multi-round files, from the device's CU count and the plan's B: lengths cycle
k B - r, k in {1, 2, 3, 5}, r in {0, 1, 37, B - 1}, channels cycle 1-3, filled
up with one-unit mono files to exactly 2 cus + cus // 3 units: two swizzled
rounds of the persistent grid and a partial tail, so a workgroup's consecutive
units lie in different rows, files and groups (asserted from the table).
The per-file references of these ~110 files go through one pair of device
buffers sized for the largest file.
"""
import numpy as np
import pytest

import test_gpu_items as gi
from test_gpu_items import Batch, d2h, h2d, max_ulps, per_file_reference, same_bits

pytestmark = pytest.mark.gpu

RMS_TOL = gi.RMS_TOL
SENTINEL = np.uint32(0xDEADBEEF)
AUTO, GROUPS = "auto", "groups"

# name: taps, tuning, family, perturb, then the plan it must give
FORMS = {
    "l16_zero_201": dict(ntaps=201, kernel=("l16",), seg_len=16384, zero_phase=True),
    "l16_general_201": dict(ntaps=201, perturb=1e-9, kernel=("l16",), seg_len=16384, zero_phase=False),
    # an odd half (2 001) in zero-phase form: the store path that splits pairs at both ends
    "lds_odd_half_4003": dict(ntaps=4003, family="lds", kernel=("l16", "l32_park"), seg_len=None, zero_phase=True),
    "lds_4001": dict(ntaps=4001, family="lds", kernel=("l16", "l32_park"), seg_len=None, zero_phase=True),
    "park_general_8001": dict(ntaps=8001, perturb=1e-9, tune=dict(seg_len=32768, zero_phase=False),
                              kernel=("l32_park",), seg_len=32768, zero_phase=False),
}
ROUND_FORMS = ["l16_zero_201", "park_general_8001"]


@pytest.fixture(scope="module")
def lc():
    import torch  # before lcfir: one HIP runtime in the process
    import lcfir
    assert torch.cuda.is_available() and lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def form_filter(lc, oracle_mod, name, **launch):
    """The form's taps and Filter (launch: chunk / max_units on top of its
    tuning), with the plan it claims to run asserted."""
    f = FORMS[name]
    tune = dict(f.get("tune") or {}, **launch)
    taps, flt = gi.make_filter(lc, oracle_mod, f["ntaps"], "fft", tune or None, f.get("family"),
                               f.get("perturb", 0.0))
    info, units = flt.fft_info, flt.fft_units
    assert units["kernel"] in f["kernel"], (name, units)
    assert info["parts"] == 1 and info["zero_phase"] == f["zero_phase"], (name, info)
    if f["seg_len"]:
        assert info["seg_len"] == f["seg_len"], (name, info)
    if name == "lds_odd_half_4003":
        assert ((f["ntaps"] - 1) // 2) % 2 == 1
    return taps, flt


def filter_references(lc, flt, files):
    """[(y, per-channel fused peaks)] of the per-file call alone, file by file
    through one pair of buffers sized for the largest file."""
    big = max(x.nbytes for x in files)
    dx, dy, dpk = lc.DeviceBuffer(big), lc.DeviceBuffer(big), lc.DeviceBuffer(4 * max(x.shape[0] for x in files))
    out = []
    for x in files:
        nch, n = x.shape
        dx.upload(x)
        lc.peak_reset_dev(dpk, nch)
        flt.filter_channels_dev(dx, n, nch, n, dy, n, dpk)
        lc.sync()
        out.append((dy.download((nch, n)), dpk.download(nch)))
    for d in (dx, dy, dpk):
        d.free()
    return out


def unit_total(unit, files):
    return sum(x.shape[0] * -(-x.shape[1] // unit) for x in files)


def arena(lc, b, unit, which=1):
    """(base address, plan) of the item set's input (0) or output (1) arena."""
    plan = lc.ItemSet.plan(unit, b.n, b.nch)
    assert plan["arena_floats"] == b.items.info()["arena_floats"]
    live = next(f for f, x in enumerate(b.files) if x.size)
    return b.items.file(live)[which] - 4 * int(plan["file_offset"][live]), plan


def oracle_points(oracle_mod, taps, unit, half, files, ys, rows=None):
    """(got, want) at row edges and both sides of every seam of the given
    (file, channel) rows (all rows by default), against the long-double oracle."""
    rng = np.random.default_rng(len(taps))
    got, want = [], []
    for f, x in enumerate(files):
        n = x.shape[1]
        for c in range(x.shape[0] if n else 0):
            if rows is not None and (f, c) not in rows:
                continue
            head, tail = min(half, n), max(0, n - half)
            pos = [0, 1, head - 1, head, tail - 1, tail, n - 2, n - 1]
            pos += rng.integers(0, max(1, head), 4).tolist() + rng.integers(tail, n, 4).tolist()
            for seam in range(unit, n, unit):
                pos += [seam - 1, seam]
            idx = np.unique(np.clip(np.array(pos, np.int64), 0, n - 1))
            ref, _ = oracle_mod.filter_points(x[c], taps, idx, oracle_mod.MODE_LD)
            got.append(ys[f][c][idx])
            want.append(ref)
    return np.concatenate(got), np.concatenate(want)


def assert_oracle(got, want):
    d = got.astype(np.float64) - want
    print(f"oracle: {got.size} points, rms {float(np.sqrt(np.mean(d * d))):.3e}, max ulps {max_ulps(got, want)}")
    assert float(np.sqrt(np.mean(d * d))) <= RMS_TOL
    assert max_ulps(got, want) <= 1


# ---- 1, 2: the forms, and no stray store ------------------------------------
@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def case(request, lc, oracle_mod):
    """Per form, computed once and left unchanged: the per-file references, two
    fused runs, a fused run into a sentinel-filled arena and a per-group run."""
    name = request.param
    taps, flt = form_filter(lc, oracle_mod, name)
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=len(taps))
    refs = [per_file_reference(lc, flt, x) for x in files]
    b = Batch(lc, flt, files)
    launches_default = b.items.filter_launches()
    b.items.set_fusion(AUTO)
    launches_auto = b.items.filter_launches()
    b.run()
    y1, pk1 = b.outputs(), b.peaks()
    base, plan = arena(lc, b, unit)
    total = int(plan["arena_floats"])
    h2d(lc, base, np.full(total, SENTINEL, np.uint32))
    b.run()
    y2, pk2 = b.outputs(), b.peaks()
    after = d2h(lc, base, total, np.uint32)
    b.items.set_fusion(GROUPS)
    launches_groups = b.items.filter_launches()
    b.run()
    yg, pkg = b.outputs(), b.peaks()
    b.items.set_fusion(AUTO)
    launches_back = b.items.filter_launches()
    info = b.items.info()
    b.close()
    return dict(name=name, taps=taps, flt=flt, unit=unit, half=half, files=files, refs=refs, plan=plan, info=info,
                launches_default=launches_default, launches_auto=launches_auto, launches_groups=launches_groups,
                launches_back=launches_back,
                y1=y1, pk1=pk1, y2=y2, pk2=pk2, after=after, yg=yg, pkg=pkg)


def test_one_launch_for_all_groups(case):
    units = unit_total(case["unit"], case["files"])
    assert units == 33 and case["info"]["groups"] == 3
    assert case["launches_default"] == (3, 0)  # an item set starts on the per-group path
    assert case["launches_auto"] == (1, units)
    assert case["launches_back"] == (1, units)


def test_outputs_and_peaks_equal_the_per_file_calls(case):
    for f, (ref, y) in enumerate(zip(case["refs"], case["y1"])):
        assert same_bits(y, ref[0]), (case["name"], f)
    want = np.array([r[1].max() if r[1].size and r[0].size else 0.0 for r in case["refs"]], np.float32)
    assert same_bits(case["pk1"], want), (case["pk1"], want)
    assert [f for f in range(len(want)) if want[f] > 1.0] == [gi.LOUD] and want[gi.ZERO] == 0.0


def test_second_run_gives_the_same_bytes(case):
    for f, (a, b) in enumerate(zip(case["y1"], case["y2"])):
        assert same_bits(a, b), (case["name"], f)
    assert same_bits(case["pk1"], case["pk2"])


def test_groups_mode_gives_the_same_bytes(case):
    assert case["launches_groups"] == (case["info"]["launches"], 0) and case["info"]["launches"] == 3
    for f, (a, b) in enumerate(zip(case["y1"], case["yg"])):
        assert same_bits(a, b), (case["name"], f)
    assert same_bits(case["pk1"], case["pkg"])


def test_no_store_outside_the_files_own_outputs(case):
    """The output arena was filled with a sentinel before the second fused
    run: every float outside [0, n_f) of every row, the rows' tails and the
    padding between groups included, still holds it."""
    plan, after = case["plan"], case["after"]
    own = np.zeros(after.size, bool)
    for f, x in enumerate(case["files"]):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            own[o:o + x.shape[1]] = True
    assert 0 < own.sum() < own.size  # there is padding to check
    assert np.all(after[~own] == SENTINEL), int((after[~own] != SENTINEL).sum())
    # and the rows themselves were all written (the zero file's too)
    got = after.view(np.float32)
    for f, x in enumerate(case["files"]):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            assert same_bits(got[o:o + x.shape[1]], case["refs"][f][0][c]), (f, c)


def test_outputs_against_the_oracle(case, oracle_mod):
    got, want = oracle_points(oracle_mod, case["taps"], case["unit"], case["half"], case["files"], case["y1"])
    assert 150 <= got.size <= 1000
    assert_oracle(got, want)


# ---- 3, 4: multi-round ragged launches, split launches --------------------------
def round_files(cus, B, seed):
    target = 2 * cus + cus // 3
    rng = np.random.default_rng(seed)
    ks, rs = [1, 2, 3, 5], [0, 1, 37, B - 1]
    shapes, units, i = [], 0, 0
    while True:
        k, r, nch = ks[i % 4], rs[(i + i // 4) % 4], 1 + i % 3
        if units + nch * k > target:
            break
        shapes.append((nch, k * B - r))
        units += nch * k
        i += 1
    while units < target:  # one-unit mono files up to the exact total
        shapes.append((1, B - rs[i % 4]))
        units += 1
        i += 1
    files = []
    for f, (nch, n) in enumerate(shapes):
        x = (rng.integers(-2**23, 2**23, size=(nch, n)) / 2.0**23 * 0.4).astype(np.float32)
        if f % 7 == 3:
            x *= np.float32(4.0)  # some files peak above 1
        files.append(np.ascontiguousarray(x))
    return files, target


def unit32(i, b, g, units):
    """fft_unit32 (fir_fft.hpp) restated."""
    base = i * g
    if g % 8 != 0 or base + g > units:
        return base + b
    return base + (b % 8) * (g // 8) + b // 8


@pytest.fixture(scope="module", params=ROUND_FORMS, ids=ROUND_FORMS)
def rounds(request, lc, oracle_mod, cus):
    name = request.param
    taps, flt = form_filter(lc, oracle_mod, name)
    B, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files, target = round_files(cus, B, seed=len(taps) + 1)
    refs = filter_references(lc, flt, files)
    b = Batch(lc, flt, files)
    b.items.set_fusion(AUTO)
    launches = b.items.filter_launches()
    b.run()
    y, pk = b.outputs(), b.peaks()
    # the same set in launches of at most cus // 2 entries
    flt.set_fft_tuning(**dict(FORMS[name].get("tune") or {}, max_units=cus // 2))
    launches_split = b.items.filter_launches()
    b.run()
    y_split, pk_split = b.outputs(), b.peaks()
    table = lc.ItemSet.unit_table(B, b.n, b.nch)
    plan = lc.ItemSet.plan(B, b.n, b.nch)
    b.close()
    return dict(name=name, taps=taps, B=B, half=half, files=files, target=target, refs=refs, launches=launches,
                y=y, pk=pk, launches_split=launches_split, y_split=y_split, pk_split=pk_split, table=table,
                plan=plan, n=b.n, nch=b.nch)


def test_rounds_shape(rounds, cus):
    """Two full rounds and a partial tail; a workgroup's consecutive units lie
    in different rows, files and groups."""
    t, plan, units = rounds["table"], rounds["plan"], rounds["target"]
    assert t.size == units == 2 * cus + cus // 3 and rounds["launches"] == (1, units)
    assert plan["groups"] == 4  # k = 1, 2, 3, 5
    row_file = {}
    for f in range(len(rounds["n"])):
        for c in range(rounds["nch"][f]):
            row_file[int(plan["file_offset"][f] + c * plan["file_stride"][f])] = f
    rows = files = groups = 0
    for wg in range(cus):
        walk = [unit32(i, wg, cus, units) for i in range(3)]
        walk = [u for u in walk if u < units]
        assert len(walk) >= 2
        for a, b in zip(walk[:-1], walk[1:]):
            fa, fb = row_file[int(t["off"][a])], row_file[int(t["off"][b])]
            rows += t["off"][a] != t["off"][b]
            files += fa != fb
            groups += plan["file_group"][fa] != plan["file_group"][fb]
    assert rows >= cus and files >= cus and groups >= cus // 2, (rows, files, groups)


def test_rounds_equal_the_per_file_calls(rounds):
    for f, (ref, y) in enumerate(zip(rounds["refs"], rounds["y"])):
        assert same_bits(y, ref[0]), (rounds["name"], f, rounds["files"][f].shape)
    want = np.array([r[1].max() for r in rounds["refs"]], np.float32)
    assert same_bits(rounds["pk"], want)
    assert (want > 1.0).any() and (want < 1.0).any()


def test_rounds_against_the_oracle(rounds, oracle_mod):
    rng = np.random.default_rng(3)
    all_rows = [(f, c) for f, x in enumerate(rounds["files"]) for c in range(x.shape[0])]
    pick = {all_rows[i] for i in rng.choice(len(all_rows), 16, replace=False)}
    got, want = oracle_points(oracle_mod, rounds["taps"], rounds["B"], rounds["half"], rounds["files"],
                              rounds["y"], rows=pick)
    assert got.size >= 150
    assert_oracle(got, want)


def test_split_launches(rounds, cus):
    units, per = rounds["target"], cus // 2
    assert rounds["launches_split"] == (-(-units // per), units) and rounds["launches_split"][0] >= 5
    for f, (a, b) in enumerate(zip(rounds["y"], rounds["y_split"])):
        assert same_bits(a, b), (rounds["name"], f)
    assert same_bits(rounds["pk"], rounds["pk_split"])


# ---- 5: fallbacks ----------------------------------------------------------------
FALLBACKS = ["direct15", "parts_38401", "register_kernel_4001", "chunk_below_longest_row",
             "seg_len_changed_after_create"]


@pytest.mark.parametrize("which", FALLBACKS)
def test_fallbacks_take_the_group_path(lc, oracle_mod, which):
    if which == "direct15":
        taps, flt = gi.make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
        assert flt.method == "direct"
    elif which == "parts_38401":
        taps, flt = gi.make_filter(lc, oracle_mod, 38401, "fft", None, None, 0.0)
        assert flt.fft_info["parts"] == 2
    elif which == "register_kernel_4001":
        taps, flt = gi.make_filter(lc, oracle_mod, 4001, "fft", None, None, 0.0)
        assert flt.fft_info["parts"] == 1 and flt.fft_units["kernel"] == "l32_reg"
    else:
        taps, flt = form_filter(lc, oracle_mod, "l16_zero_201")
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=len(taps) + 2)
    b = Batch(lc, flt, files)
    b.items.set_fusion(AUTO)
    if which == "chunk_below_longest_row":
        assert b.items.filter_launches() == (1, 33)
        flt.set_fft_tuning(chunk=2 * unit)  # the longest row has 3 U - 1 frames
        assert flt.fft_units["outputs"] == unit and max(b.n) > 2 * unit
    elif which == "seg_len_changed_after_create":
        assert b.items.filter_launches() == (1, 33)
        flt.set_fft_tuning(seg_len=32768)
        assert flt.fft_info["parts"] == 1 and flt.fft_units["outputs"] != unit
        flt.set_fft_family("lds")  # an LDS-column kernel again: only the B differs from the table's
        assert flt.fft_units["kernel"] == "l32_park" and flt.fft_units["outputs"] != unit
    assert b.items.filter_launches() == (b.items.info()["launches"], 0) == (3, 0)
    refs = [per_file_reference(lc, flt, x) for x in files]  # under the tuning the set now runs with
    b.run()
    for f, (ref, y) in enumerate(zip(refs, b.outputs())):
        assert same_bits(y, ref[0]), (which, f)
    want = np.array([r[1].max() if r[1].size and r[0].size else 0.0 for r in refs], np.float32)
    assert same_bits(b.peaks(), want)
    b.close()


def test_set_fusion_rejects_an_unknown_mode(lc, oracle_mod):
    _, flt = gi.make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
    items = lc.ItemSet(flt, [100], [1])
    lib = lc.load()
    assert lib.lcfir_items_set_fusion(items._h, 2) == lc.EINVAL
    assert lib.lcfir_items_set_fusion(None, 0) == lc.EINVAL
    assert lib.lcfir_items_filter_launches(items._h, None, None) == lc.EINVAL
    items.close()


# ---- 6: graph capture ------------------------------------------------------------
@pytest.mark.parametrize("name", ["l16_zero_201", "park_general_8001"])
def test_graph_capture_replays_the_fused_launch(lc, oracle_mod, name):
    """Filter + peaks captured after an eager call on the stream (which sizes
    the park kernel's slab), replayed twice into poisoned outputs."""
    import torch
    taps, flt = form_filter(lc, oracle_mod, name)
    unit = gi.unit_of(flt)
    rng = np.random.default_rng(5)
    files = [(rng.standard_normal((nch, n)) * s).astype(np.float32)
             for nch, n, s in [(2, unit + 11, 0.1), (1, 777, 0.1), (3, 2 * unit + 5, 0.6)]]
    b = Batch(lc, flt, files)
    b.items.set_fusion(AUTO)
    assert b.items.filter_launches() == (1, 2 * 2 + 1 + 3 * 3)
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


# ---- 7: isolation ----------------------------------------------------------------
def test_a_nan_stays_in_its_own_files_segments(lc, oracle_mod):
    """One NaN in one row: only the units of that row whose windows hold it
    turn non-finite; every other row's bytes are the clean run's."""
    taps, flt = form_filter(lc, oracle_mod, "l16_zero_201")
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=11)
    b = Batch(lc, flt, files)
    b.items.set_fusion(AUTO)
    assert b.items.filter_launches() == (1, 33)
    b.run()
    clean = b.outputs()
    F, C, P = 7, 1, unit + 5  # file 7: 2 U + 37 frames, 2 channels; the sample sits in segments 0 and 1's windows
    assert files[F].shape == (2, 2 * unit + 37) and P - half < unit and P + half >= unit and P + half < 2 * unit
    bad = [x.copy() for x in files]
    bad[F][C, P] = np.nan
    dx, _, stride = b.items.file(F)
    h2d(lc, dx + 4 * (C * stride + P), bad[F][C, P:P + 1])
    b.run()
    got = b.outputs()
    for f in range(len(files)):
        for c in range(files[f].shape[0]):
            if (f, c) != (F, C):
                assert same_bits(got[f][c], clean[f][c]), (f, c)
    row = got[F][C]
    assert np.isfinite(row[2 * unit:]).all() and same_bits(row[2 * unit:], clean[F][C][2 * unit:])
    assert not np.isfinite(row[:unit]).all() and not np.isfinite(row[unit:2 * unit]).all()
    # and the poisoned file is still the per-file call's: the same outputs are
    # NaN, every other output bit for bit.  (A NaN's own sign and payload are
    # not compared: which operand's NaN a commutative f64 operation passes on is
    # the compiler's choice per kernel instantiation, not part of the arithmetic
    # the identity argument covers.)
    want = per_file_reference(lc, flt, bad[F])[0]
    assert np.array_equal(np.isnan(got[F]), np.isnan(want))
    ok = ~np.isnan(want)
    assert same_bits(got[F][ok], want[ok])
    assert not np.isfinite(row[:2 * unit]).any()  # a segment whose window holds a NaN is non-finite throughout (lcfir.h)
    b.close()
