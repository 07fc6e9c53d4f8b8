"""GPU tests of the item sets' fused per-file peak (set_peak_fusion(True),
lcfir_items_set_peak_fusion): on a fused filter path the launches that round to
f32 -- the single launch, or a partitioned plan's last partition's -- raise
d_peak[f] themselves from every unit of file f, the slot coming from a second
per-unit table (lcfir_items_unit_files), and the ragged peak launch is not made
(include/lcfir.h; csrc/fir_fft.hpp, kItemPeak).

The expected value is always the per-file entry point on the same build,
lcfir_filter_channels_dev with its fused peaks, compared bit for bit with no
tolerance; the peaks also against the same item set with peak fusion off (the
separate ragged pass).  Files, references and the Batch helper are those of
tests/test_gpu_items.py, test_gpu_items_fused.py and test_gpu_items_parts.py,
imported.  The standard files are gi.make_files with file f additionally scaled
by 1 + f / 32, so every file with samples has a peak of its own and a peak
committed to another file's slot cannot pass.

No test here runs a register-kernel plan except the one fallback case that
pins such a plan to the per-group path, with the files the existing fallback
tests use.
"""
import numpy as np
import pytest

import test_gpu_items as gi
import test_gpu_items_fused as gf
import test_gpu_items_parts as gp
from test_gpu_items import Batch, d2h, h2d, per_file_reference, same_bits
from test_gpu_items_fused import arena, filter_references
from test_gpu_items_parts import file_peaks

pytestmark = pytest.mark.gpu

SENTINEL = gf.SENTINEL
PARTS, AUTO, GROUPS = "parts", "auto", "groups"
# form -> the module that defines it and the fusion mode that fuses it
FORMS = {"l16_zero_201": (gf, AUTO), "l16_general_201": (gf, AUTO), "lds_4001": (gf, AUTO),
         "park_general_8001": (gf, AUTO), "l16_parts2": (gp, PARTS), "park_parts2": (gp, PARTS)}
ROUND_FORMS = ["l16_zero_201", "park_general_8001", "l16_parts2"]
KEEP, KEPT = 3, np.float32(1e30)  # a slot prefilled above every peak


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
    """(taps, Filter, fusion mode, partitions, the form's own tuning)."""
    mod, mode = FORMS[name]
    taps, flt = mod.form_filter(lc, oracle_mod, name, **launch)
    return taps, flt, mode, flt.fft_info["parts"], dict(mod.FORMS[name].get("tune") or {})


def scaled_files(unit, half, seed):
    files = gi.make_files(unit, half, seed)
    return [np.ascontiguousarray(x * np.float32(1.0 + f / 32.0)) for f, x in enumerate(files)]


def fused_batch(lc, flt, files, mode):
    b = Batch(lc, flt, files)
    b.items.set_fusion(mode)
    assert b.items.filter_launches()[1] == gf.unit_total(gi.unit_of(flt), files) > 0  # a fused path
    assert b.items.peak_launches() == 1  # the switch starts off
    b.items.set_peak_fusion(True)
    assert b.items.peak_launches() == 0
    return b


def run_unfused(b):
    """The same item set's outputs and peaks with the separate peak pass."""
    b.items.set_peak_fusion(False)
    assert b.items.peak_launches() == 1
    b.run()
    out = b.outputs(), b.peaks()
    b.items.set_peak_fusion(True)
    assert b.items.peak_launches() == 0
    return out


def walk_pairs(cus, units, per=None):
    """Consecutive units (u, v) of every workgroup of the launches over a table
    of `units` entries in slices of `per` (fft_launch_items, fft_unit32)."""
    per = per or units
    for u0 in range(0, units, per):
        nu = min(per, units - u0)
        g = min(nu, cus)
        for wg in range(g):
            walk, i = [], 0
            while True:
                u = gf.unit32(i, wg, g, nu)
                if u >= nu:
                    break
                walk.append(u0 + u)
                i += 1
            yield from zip(walk[:-1], walk[1:])


# ---- 1: standard files, per form ---------------------------------------------------
@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def case(request, lc, oracle_mod):
    name = request.param
    taps, flt, mode, parts, _ = form_filter(lc, oracle_mod, name)
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = scaled_files(unit, half, seed=len(taps))
    refs = [per_file_reference(lc, flt, x) for x in files]
    b = fused_batch(lc, flt, files, mode)
    launches = b.items.filter_launches()
    b.run()
    y1, pk1 = b.outputs(), b.peaks()
    y0, pk0 = run_unfused(b)
    # again into a sentinel-filled output arena, one slot prefilled above every peak
    base, plan = arena(lc, b, unit)
    total = int(plan["arena_floats"])
    h2d(lc, base, np.full(total, SENTINEL, np.uint32))
    lc.peak_reset_dev(b.dpk, len(files))
    h2d(lc, b.dpk.data_ptr() + 4 * KEEP, np.array([KEPT], np.float32))
    b.items.filter_dev(b.dpk)
    lc.sync()
    y2, pk2 = b.outputs(), b.peaks()
    after = d2h(lc, base, total, np.uint32)
    b.close()
    return dict(name=name, parts=parts, unit=unit, files=files, refs=refs, plan=plan, launches=launches,
                y1=y1, pk1=pk1, y0=y0, pk0=pk0, y2=y2, pk2=pk2, after=after)


def test_outputs_and_peaks_equal_the_per_file_calls(case):
    assert case["launches"] == (case["parts"], gf.unit_total(case["unit"], case["files"]))
    for f, (ref, y) in enumerate(zip(case["refs"], case["y1"])):
        assert same_bits(y, ref[0]), (case["name"], f)
    want = file_peaks(case["refs"])
    print("peaks", case["pk1"], "want", want)
    assert same_bits(case["pk1"], want), (case["pk1"], want)
    assert same_bits(case["pk1"], case["pk0"]), (case["pk1"], case["pk0"])
    for f, y in enumerate(case["y0"]):
        assert same_bits(y, case["refs"][f][0]), (case["name"], f)
    # the empty file and the zero file: exactly 0; every other file a peak of its own
    assert case["files"][0].size == 0 and want[0] == 0.0 and want[gi.ZERO] == 0.0
    live = [f for f in range(len(want)) if f not in (0, gi.ZERO)]
    assert len({want[f].tobytes() for f in live}) == len(live) and all(want[f] > 0 for f in live)


def test_a_prefilled_slot_keeps_its_value_and_a_second_run_gives_the_same_bytes(case):
    for f, (a, b) in enumerate(zip(case["y1"], case["y2"])):
        assert same_bits(a, b), (case["name"], f)
    want = case["pk1"].copy()
    assert KEPT > want.max() and case["files"][KEEP].size > 0
    want[KEEP] = KEPT
    assert same_bits(case["pk2"], want), (case["pk2"], want)


def test_no_store_outside_the_files_own_outputs(case):
    plan, after = case["plan"], case["after"]
    own = np.zeros(after.size, bool)
    for f, x in enumerate(case["files"]):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            own[o:o + x.shape[1]] = True
    assert 0 < own.sum() < own.size  # there is padding to check
    assert np.all(after[~own] == SENTINEL), int((after[~own] != SENTINEL).sum())


# ---- 2: multi-round launches, split launches ----------------------------------------
@pytest.fixture(scope="module", params=ROUND_FORMS, ids=ROUND_FORMS)
def rounds(request, lc, oracle_mod, cus):
    name = request.param
    taps, flt, mode, parts, tune = form_filter(lc, oracle_mod, name)
    B = gi.unit_of(flt)
    files, target = gf.round_files(cus, B, seed=len(taps) + 1)
    refs = filter_references(lc, flt, files)
    b = fused_batch(lc, flt, files, mode)
    launches = b.items.filter_launches()
    b.run()
    y, pk = b.outputs(), b.peaks()
    _, pk0 = run_unfused(b)
    flt.set_fft_tuning(**dict(tune, max_units=cus // 2))
    launches_split, peak_launches_split = b.items.filter_launches(), b.items.peak_launches()
    b.run()
    y_split, pk_split = b.outputs(), b.peaks()
    unit_file = lc.ItemSet.unit_files(B, b.n, b.nch)
    b.close()
    return dict(name=name, parts=parts, files=files, target=target, refs=refs, launches=launches, y=y, pk=pk,
                pk0=pk0, launches_split=launches_split, peak_launches_split=peak_launches_split, y_split=y_split,
                pk_split=pk_split, unit_file=unit_file)


def test_rounds_change_file_between_a_workgroups_units(rounds, cus):
    uf, units = rounds["unit_file"], rounds["target"]
    assert uf.size == units == 2 * cus + cus // 3 and rounds["launches"] == (rounds["parts"], units)
    pairs = list(walk_pairs(cus, units))
    assert len(pairs) == units - cus
    changes = sum(int(uf[a] != uf[b]) for a, b in pairs)
    assert changes >= cus, (changes, cus)
    split = list(walk_pairs(cus, units, cus // 2))
    assert split == []  # slices of cus // 2 entries: one unit per workgroup, the flush alone commits


def test_rounds_equal_the_per_file_calls(rounds):
    for f, (ref, y) in enumerate(zip(rounds["refs"], rounds["y"])):
        assert same_bits(y, ref[0]), (rounds["name"], f, rounds["files"][f].shape)
    want = np.array([r[1].max() for r in rounds["refs"]], np.float32)
    assert same_bits(rounds["pk"], want)
    assert same_bits(rounds["pk"], rounds["pk0"])
    assert (want > 1.0).any() and (want < 1.0).any()


def test_split_launches_slice_both_tables_alike(rounds, cus):
    units, per = rounds["target"], cus // 2
    assert rounds["launches_split"] == (rounds["parts"] * -(-units // per), units)
    assert rounds["launches_split"][0] >= 5 * rounds["parts"] and rounds["peak_launches_split"] == 0
    for f, (a, b) in enumerate(zip(rounds["y"], rounds["y_split"])):
        assert same_bits(a, b), (rounds["name"], f)
    assert same_bits(rounds["pk"], rounds["pk_split"])


# ---- 3: a workgroup that stays in its file ------------------------------------------
def test_consecutive_units_of_one_file_stage_nothing(lc, oracle_mod, cus):
    """Two mono files of cus + cus // 2 + 3 segments each and one 3-channel file
    of 2 segments: more than cus workgroup steps go from a unit to another unit
    of the same file (the running peak is kept, nothing staged), the others
    change file; the 3-channel file's peak is the maximum over its rows."""
    taps, flt, mode, _, _ = form_filter(lc, oracle_mod, "l16_zero_201")
    B = gi.unit_of(flt)
    S = cus + cus // 2 + 3
    rng = np.random.default_rng(17)

    def noise(nch, n, scale):
        x = (rng.integers(-2**23, 2**23, size=(nch, n)) / 2.0**23 * 0.4).astype(np.float32)
        return np.ascontiguousarray(x * np.asarray(scale, np.float32).reshape(-1, 1))

    files = [noise(1, S * B - 5, [1.0]), noise(3, 2 * B - 7, [0.5, 1.25, 0.75]), noise(1, S * B - 11, [0.875])]
    refs = filter_references(lc, flt, files)
    b = fused_batch(lc, flt, files, mode)
    uf = lc.ItemSet.unit_files(B, b.n, b.nch)
    units = 2 * S + 6
    assert uf.size == units and uf.tolist() == [1] * 6 + [0] * S + [2] * S
    pairs = list(walk_pairs(cus, units))
    stays = sum(int(uf[a] == uf[c]) for a, c in pairs)
    assert stays >= cus and len(pairs) - stays >= cus, (stays, len(pairs))
    b.run()
    for f, (ref, y) in enumerate(zip(refs, b.outputs())):
        assert same_bits(y, ref[0]), f
    pk = b.peaks()
    want = np.array([r[1].max() for r in refs], np.float32)
    assert same_bits(pk, want), (pk, want)
    assert int(np.argmax(refs[1][1])) == 1 and len(set(refs[1][1].tolist())) == 3  # over its rows: the middle one
    _, pk0 = run_unfused(b)
    assert same_bits(pk, pk0)
    b.close()


# ---- 4: value domain ------------------------------------------------------------------
BIG = np.float32(3e38)


@pytest.mark.parametrize("name", ["l16_zero_201", "park_parts2"])
def test_nan_is_skipped_and_inf_is_taken(lc, oracle_mod, name):
    """One NaN sample, one +Inf sample, and finite samples whose output
    overflows f32, in one row of one file.  A non-finite SAMPLE turns every
    output of the segments that read it into NaN (the f64 transform mixes Inf
    into Inf - Inf), so the per-file call's peak of such a file is the maximum
    over its other, non-NaN outputs, for +Inf as for NaN (0.5684154 on
    l16_zero_201, not Inf).  An Inf OUTPUT comes from
    the narrowing: sample P = +3e38 among samples of -3e38 gives a finite f64
    sum of 1.74 (201 taps) or 1.76 (38 401 taps) times the f32 maximum at
    output P alone, which rounds to +Inf; that file's peak is Inf."""
    taps, flt, mode, _, _ = form_filter(lc, oracle_mod, name)
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = scaled_files(unit, half, seed=11)
    b = fused_batch(lc, flt, files, mode)
    b.run()
    clean, pk_clean = b.outputs(), b.peaks()
    F, C, P = 7, 1, unit + 5  # file 7: 2 U + 37 frames, 2 channels
    n = 2 * unit + 37
    assert files[F].shape == (2, n)
    dx, _, stride = b.items.file(F)
    row = files[F][C]
    nan_row, inf_row, over_row = row.copy(), row.copy(), row.copy()
    nan_row[P], inf_row[P] = np.nan, np.inf
    over_row[max(0, P - half):min(n, P + half + 1)] = -BIG
    over_row[P] = BIG
    for what, bad_row in (("nan", nan_row), ("inf_sample", inf_row), ("overflow", over_row)):
        h2d(lc, dx + 4 * C * stride, bad_row)
        b.run()
        got, pk = b.outputs(), b.peaks()
        y0, pk0 = run_unfused(b)
        bad = files[F].copy()
        bad[C] = bad_row
        ref = per_file_reference(lc, flt, bad)
        print(name, what, "peak", pk[F], "unfused", pk0[F], "per-file", ref[1], "clean", pk_clean[F])
        assert same_bits(pk, pk0), (pk, pk0)
        assert same_bits(pk[F:F + 1], ref[1].max(keepdims=True)), (pk[F], ref[1])
        for f in range(len(files)):
            if f != F:
                assert same_bits(got[f], clean[f]) and same_bits(pk[f:f + 1], pk_clean[f:f + 1]), f
        assert same_bits(got[F][0], clean[F][0]) and not np.isfinite(got[F][C]).all()
        for want in (y0[F], ref[0]):
            assert np.array_equal(np.isnan(got[F]), np.isnan(want))
            ok = ~np.isnan(want)
            assert ok.any() and same_bits(got[F][ok], want[ok])
        # NaN skipped, Inf taken: the maximum over the file's non-NaN outputs
        assert pk[F] == np.abs(got[F][ok]).max()
        if what == "overflow":
            assert not np.isnan(got[F]).any() and got[F][C][P] == np.float32(np.inf)
            assert pk[F] == np.float32(np.inf)
        else:
            assert np.isnan(got[F][C]).any() and np.isfinite(pk[F]) and pk[F] > 0
        # the normalize that follows: the unfused path's bytes
        b.items.normalize_dev(b.dpk, False)
        lc.sync()
        n_fused = b.outputs()
        b.items.set_peak_fusion(False)
        b.run()
        b.items.normalize_dev(b.dpk, False)
        lc.sync()
        n_unfused = b.outputs()
        b.items.set_peak_fusion(True)
        for f in range(len(files)):
            assert np.array_equal(np.isnan(n_fused[f]), np.isnan(n_unfused[f])), f
            okf = ~np.isnan(n_fused[f])
            assert same_bits(n_fused[f][okf], n_unfused[f][okf]), f
    b.close()


# ---- 5: graph capture -----------------------------------------------------------------
def test_graph_capture_replays_the_fused_peak(lc, oracle_mod):
    """peak_reset + filter_dev captured after one eager step, replayed three
    times with one file's input rescaled between replays: the peaks follow."""
    import torch
    taps, flt, mode, _, _ = form_filter(lc, oracle_mod, "l16_zero_201")
    unit = gi.unit_of(flt)
    rng = np.random.default_rng(5)
    files = [(rng.standard_normal((nch, n)) * s).astype(np.float32)
             for nch, n, s in [(2, unit + 11, 0.1), (1, 777, 0.1), (3, 2 * unit + 5, 0.6)]]
    b = fused_batch(lc, flt, files, mode)
    s = torch.cuda.Stream()
    pk = torch.zeros(3, dtype=torch.float32, device="cuda")

    def step():
        lc.peak_reset_dev(pk, 3, s.cuda_stream)
        b.items.filter_dev(pk, s.cuda_stream)

    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    seen = []
    for scale in (1.0, 3.0, 0.25):
        cur = [x.copy() for x in files]
        cur[2] = np.ascontiguousarray(files[2] * np.float32(scale))
        dx, _, stride = b.items.file(2)
        for c in range(3):
            h2d(lc, dx + 4 * c * stride, cur[2][c])
        pk.fill_(7.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        refs = [per_file_reference(lc, flt, x) for x in cur]
        for f in range(3):
            assert same_bits(b.rows(f), refs[f][0]), (scale, f)
        got = pk.cpu().numpy()
        assert same_bits(got, file_peaks(refs)), (scale, got)
        seen.append(got[2])
    assert seen[1] > seen[0] > seen[2] > 0
    del g
    b.close()


# ---- 6: fallbacks with peak fusion on -------------------------------------------------
FALLBACKS = ["groups_mode", "direct15", "parts_under_auto", "register_kernel_4001"]


@pytest.mark.parametrize("which", FALLBACKS)
def test_fallbacks_keep_the_separate_peak_launch(lc, oracle_mod, which):
    mode = AUTO
    if which == "groups_mode":
        taps, flt = gf.form_filter(lc, oracle_mod, "l16_zero_201")
        mode = GROUPS
    elif which == "direct15":
        taps, flt = gi.make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
        assert flt.method == "direct"
    elif which == "parts_under_auto":
        taps, flt = gp.form_filter(lc, oracle_mod, "l16_parts2")
    else:
        taps, flt = gi.make_filter(lc, oracle_mod, 4001, "fft", None, None, 0.0)
        assert flt.fft_info["parts"] == 1 and flt.fft_units["kernel"] == "l32_reg"
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=len(taps) + 2)  # the existing fallback tests' files
    b = Batch(lc, flt, files)
    b.items.set_fusion(mode)
    b.items.set_peak_fusion(True)
    assert b.items.filter_launches() == (b.items.info()["launches"], 0)  # the per-group path
    assert b.items.peak_launches() == 1
    refs = [per_file_reference(lc, flt, x) for x in files]
    b.run()
    for f, (ref, y) in enumerate(zip(refs, b.outputs())):
        assert same_bits(y, ref[0]), (which, f)
    assert same_bits(b.peaks(), file_peaks(refs))
    # and without a d_peak the call is what it was
    b.run(peaks=False)
    assert same_bits(b.peaks(), np.zeros(len(files), np.float32))
    b.close()


def test_set_peak_fusion_rejects_other_values(lc, oracle_mod):
    taps, flt = gf.form_filter(lc, oracle_mod, "l16_zero_201")
    items = lc.ItemSet(flt, [100, 40000], [1, 2])
    items.set_fusion(AUTO)
    lib = lc.load()
    assert items.peak_launches() == 1
    for bad in (2, -1, 3):
        assert lib.lcfir_items_set_peak_fusion(items._h, bad) == lc.EINVAL
        assert items.peak_launches() == 1  # a refused value changes nothing
    with pytest.raises(lc.LcfirError) as e:
        items.set_peak_fusion(2)
    assert e.value.code == lc.EINVAL
    assert lib.lcfir_items_set_peak_fusion(items._h, 1) == lc.OK and items.peak_launches() == 0
    assert lib.lcfir_items_set_peak_fusion(items._h, 2) == lc.EINVAL and items.peak_launches() == 0
    items.set_peak_fusion(False)
    assert items.peak_launches() == 1
    assert lib.lcfir_items_set_peak_fusion(None, 1) == lc.EINVAL
    assert lib.lcfir_items_peak_launches(items._h, None) == lc.EINVAL
    items.close()
