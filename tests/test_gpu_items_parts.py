"""GPU tests of the fused partitioned item-set filter (set_fusion("parts"),
LCFIR_ITEMS_FUSION_PARTS): a filter of P > 1 partitions on an LDS-column kernel
runs P launches -- first, add ... add, last -- of the kernel's item form over
the per-unit table, for every row of every group, with the f64 partial sums in
an arena-shaped slice of the stream's scratch (include/lcfir.h,
lcfir_items_filter_dev; csrc/fir_fft.hpp, fft_unit_decode, fft_launch_items).

The expected value is always the per-file entry point on the same build,
lcfir_filter_channels_dev with its fused peaks, compared bit for bit with no
tolerance; a sample of outputs -- row edges and both sides of every segment
seam -- is also held to the long-double oracle under the parity bar (<= 1 f32
ulp, RMS <= 1e-9).  Files, references and the Batch helper are those of
tests/test_gpu_items.py and tests/test_gpu_items_fused.py, imported.

Forms (taps from design_lowcut(20, 48000, ntaps); the plan each must give is
asserted from fft_info / fft_units):

  l16_parts2   14 339 taps, seg_len 16 384: l16,      2 parts, B =  9 214 (odd half)
  l16_parts3   20 001 taps, seg_len 16 384: l16,      3 parts, B =  9 718
  park_parts2  38 401 taps, default:        l32_park, 2 parts, B = 13 568 (the 96 kHz default filter)
  park_parts3  45 001 taps, seg_len 32 768: l32_park, 3 parts, B = 17 768

No test here runs a register-kernel plan except the one fallback case that
pins such a plan to the per-group path.
"""
import numpy as np
import pytest

import test_gpu_items as gi
import test_gpu_items_fused as gf
from test_gpu_items import Batch, d2h, h2d, per_file_reference, same_bits
from test_gpu_items_fused import arena, assert_oracle, filter_references, oracle_points, unit_total

pytestmark = pytest.mark.gpu

SENTINEL = gf.SENTINEL
PARTS, AUTO, GROUPS = "parts", "auto", "groups"

# name: taps, tuning, then the plan it must give
FORMS = {
    "l16_parts2": dict(ntaps=14339, tune=dict(seg_len=16384), kernel="l16", seg_len=16384, parts=2, B=9214),
    "l16_parts3": dict(ntaps=20001, tune=dict(seg_len=16384), kernel="l16", seg_len=16384, parts=3, B=9718),
    "park_parts2": dict(ntaps=38401, tune=None, kernel="l32_park", seg_len=32768, parts=2, B=13568),
    "park_parts3": dict(ntaps=45001, tune=dict(seg_len=32768), kernel="l32_park", seg_len=32768, parts=3, B=17768),
}
ROUND_FORMS = ["l16_parts2", "park_parts2"]


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
    tune = dict(f["tune"] or {}, **launch)
    taps, flt = gi.make_filter(lc, oracle_mod, f["ntaps"], "fft", tune or None, None, 0.0)
    info, units = flt.fft_info, flt.fft_units
    assert units["kernel"] == f["kernel"], (name, units)
    assert info["parts"] == f["parts"] and info["seg_len"] == f["seg_len"], (name, info)
    assert units["outputs"] == f["B"], (name, units)
    return taps, flt


def file_peaks(refs):
    return np.array([r[1].max() if r[1].size and r[0].size else 0.0 for r in refs], np.float32)


# ---- 1, 2, 3: bytes, oracle, sentinel -------------------------------------------
@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def case(request, lc, oracle_mod):
    """Per form, computed once and left unchanged: the per-file references, two
    fused partitioned runs (the second into a sentinel-filled arena), the two
    normalize passes and a per-group run."""
    name = request.param
    taps, flt = form_filter(lc, oracle_mod, name)
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=len(taps))
    refs = [per_file_reference(lc, flt, x) for x in files]
    b = Batch(lc, flt, files)
    launches_default = b.items.filter_launches()
    b.items.set_fusion(PARTS)
    launches_parts = b.items.filter_launches()
    base_in, plan = arena(lc, b, unit, which=0)
    base, _ = arena(lc, b, unit)
    total = int(plan["arena_floats"])
    x_before = d2h(lc, base_in, total, np.uint32)
    b.run()
    y1, pk1 = b.outputs(), b.peaks()
    h2d(lc, base, np.full(total, SENTINEL, np.uint32))
    b.run()
    y2, pk2 = b.outputs(), b.peaks()
    after = d2h(lc, base, total, np.uint32)
    x_after = d2h(lc, base_in, total, np.uint32)
    b.items.normalize_dev(b.dpk, False)
    lc.sync()
    y_norm0 = b.outputs()
    b.run()
    b.items.normalize_dev(b.dpk, True)
    lc.sync()
    y_norm1 = b.outputs()
    b.items.set_fusion(GROUPS)
    launches_groups = b.items.filter_launches()
    b.run()
    yg, pkg = b.outputs(), b.peaks()
    info = b.items.info()
    b.close()
    return dict(name=name, taps=taps, flt=flt, unit=unit, half=half, files=files, refs=refs, plan=plan, info=info,
                parts=FORMS[name]["parts"], launches_default=launches_default, launches_parts=launches_parts,
                launches_groups=launches_groups, y1=y1, pk1=pk1, y2=y2, pk2=pk2, after=after, x_before=x_before,
                x_after=x_after, y_norm0=y_norm0, y_norm1=y_norm1, yg=yg, pkg=pkg)


def test_one_launch_per_partition_for_all_groups(case):
    units = unit_total(case["unit"], case["files"])
    assert units > 0 and case["info"]["groups"] == case["info"]["launches"] >= 3
    assert case["launches_default"] == (case["info"]["launches"], 0)  # an item set starts on the per-group path
    assert case["launches_parts"] == (case["parts"], units)
    assert case["launches_groups"] == (case["info"]["launches"], 0)


def test_outputs_and_peaks_equal_the_per_file_calls(case):
    for f, (ref, y) in enumerate(zip(case["refs"], case["y1"])):
        assert same_bits(y, ref[0]), (case["name"], f)
    want = file_peaks(case["refs"])
    assert same_bits(case["pk1"], want), (case["pk1"], want)
    assert [f for f in range(len(want)) if want[f] > 1.0] == [gi.LOUD] and want[gi.ZERO] == 0.0


def test_groups_mode_gives_the_same_bytes(case):
    for f, (a, b) in enumerate(zip(case["y1"], case["yg"])):
        assert same_bits(a, b), (case["name"], f)
    assert same_bits(case["pk1"], case["pkg"])


def test_second_run_gives_the_same_bytes(case):
    for f, (a, b) in enumerate(zip(case["y1"], case["y2"])):
        assert same_bits(a, b), (case["name"], f)
    assert same_bits(case["pk1"], case["pk2"])


def test_normalize_equals_the_per_file_pipeline(case):
    for f, ref in enumerate(case["refs"]):
        assert same_bits(case["y_norm0"][f], ref[2]), (case["name"], f, "no force")
        assert same_bits(case["y_norm1"][f], ref[3]), (case["name"], f, "force")
    loud = case["refs"][gi.LOUD]
    assert not same_bits(loud[2], loud[0])  # the decision is exercised


def test_outputs_against_the_oracle(case, oracle_mod):
    got, want = oracle_points(oracle_mod, case["taps"], case["unit"], case["half"], case["files"], case["y1"])
    assert 150 <= got.size <= 1000
    assert_oracle(got, want)


def test_no_store_outside_the_files_own_outputs(case):
    """The output arena was filled with a sentinel before the second run: every
    float outside [0, n_f) of every row still holds it, every row was written,
    and the input arena is what it was."""
    plan, after = case["plan"], case["after"]
    own = np.zeros(after.size, bool)
    for f, x in enumerate(case["files"]):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            own[o:o + x.shape[1]] = True
    assert 0 < own.sum() < own.size  # there is padding to check
    assert np.all(after[~own] == SENTINEL), int((after[~own] != SENTINEL).sum())
    got = after.view(np.float32)
    for f, x in enumerate(case["files"]):
        for c in range(x.shape[0] if x.shape[1] else 0):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            assert same_bits(got[o:o + x.shape[1]], case["refs"][f][0][c]), (f, c)
    assert np.array_equal(case["x_before"], case["x_after"])
    assert case["x_before"].any()  # the files are in it


# ---- 4: multi-round ragged launches, split launches ------------------------------
@pytest.fixture(scope="module", params=ROUND_FORMS, ids=ROUND_FORMS)
def rounds(request, lc, oracle_mod, cus):
    name = request.param
    taps, flt = form_filter(lc, oracle_mod, name)
    B = gi.unit_of(flt)
    files, target = gf.round_files(cus, B, seed=len(taps) + 1)
    refs = filter_references(lc, flt, files)
    b = Batch(lc, flt, files)
    b.items.set_fusion(PARTS)
    launches = b.items.filter_launches()
    b.run()
    y, pk = b.outputs(), b.peaks()
    # the same set in launches of at most cus // 2 entries per partition
    flt.set_fft_tuning(**dict(FORMS[name]["tune"] or {}, max_units=cus // 2))
    launches_split = b.items.filter_launches()
    b.run()
    y_split, pk_split = b.outputs(), b.peaks()
    table = lc.ItemSet.unit_table(B, b.n, b.nch)
    plan = lc.ItemSet.plan(B, b.n, b.nch)
    b.close()
    return dict(name=name, parts=FORMS[name]["parts"], B=B, files=files, target=target, refs=refs,
                launches=launches, y=y, pk=pk, launches_split=launches_split, y_split=y_split, pk_split=pk_split,
                table=table, plan=plan, n=b.n, nch=b.nch)


def test_rounds_shape(rounds, cus):
    """Two full rounds and a partial tail; a workgroup's consecutive units lie
    in different rows, files and groups."""
    t, plan, units = rounds["table"], rounds["plan"], rounds["target"]
    assert t.size == units == 2 * cus + cus // 3 and rounds["launches"] == (rounds["parts"], units)
    assert plan["groups"] == 4  # k = 1, 2, 3, 5
    row_file = {}
    for f in range(len(rounds["n"])):
        for c in range(rounds["nch"][f]):
            row_file[int(plan["file_offset"][f] + c * plan["file_stride"][f])] = f
    rows = files = groups = 0
    for wg in range(cus):
        walk = [gf.unit32(i, wg, cus, units) for i in range(3)]
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


def test_split_launches(rounds, cus):
    units, per = rounds["target"], cus // 2
    assert rounds["launches_split"] == (rounds["parts"] * -(-units // per), units)
    assert rounds["launches_split"][0] >= 5 * rounds["parts"]
    for f, (a, b) in enumerate(zip(rounds["y"], rounds["y_split"])):
        assert same_bits(a, b), (rounds["name"], f)
    assert same_bits(rounds["pk"], rounds["pk_split"])


# ---- 5: the scratch carries nothing ----------------------------------------------
@pytest.mark.parametrize("name", ["l16_parts2", "park_parts3"])
def test_a_nan_stays_in_its_own_row_and_leaves_with_it(lc, oracle_mod, name):
    """One NaN in one row: every other row's bytes are the clean run's, and the
    poisoned file is the per-file call's.  With the sample restored the clean
    bytes come back in every row: the NaNs the partial sums held in the scratch
    are overwritten by the first partition's launch, never added to."""
    taps, flt = form_filter(lc, oracle_mod, name)
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=11)
    b = Batch(lc, flt, files)
    b.items.set_fusion(PARTS)
    assert b.items.filter_launches() == (FORMS[name]["parts"], unit_total(unit, files))
    b.run()
    clean = b.outputs()
    F, C, P = 7, 1, unit + 5  # file 7: 2 U + 37 frames, 2 channels
    assert files[F].shape == (2, 2 * unit + 37)
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
    # (a NaN's own sign and payload are not compared: which operand's NaN a
    # commutative f64 operation passes on is the compiler's choice per kernel
    # instantiation, not part of the arithmetic the identity argument covers)
    want = per_file_reference(lc, flt, bad[F])[0]
    assert np.isnan(want[C]).any() and not np.isnan(want[0]).any()
    assert np.array_equal(np.isnan(got[F]), np.isnan(want))
    ok = ~np.isnan(want)
    assert same_bits(got[F][ok], want[ok])
    h2d(lc, dx + 4 * (C * stride + P), files[F][C, P:P + 1])
    b.run()
    for f, (a, y) in enumerate(zip(clean, b.outputs())):
        assert same_bits(a, y), f
    b.close()


# ---- 6: graph capture ------------------------------------------------------------
def test_graph_capture_replays_the_partition_launches(lc, oracle_mod):
    """Filter + peaks captured after an eager call on the stream (which sizes
    the partial-sum scratch), replayed twice into poisoned outputs; a capture
    on a stream no eager call has sized is refused."""
    import torch
    taps, flt = form_filter(lc, oracle_mod, "l16_parts3")
    unit = gi.unit_of(flt)
    rng = np.random.default_rng(5)
    files = [(rng.standard_normal((nch, n)) * s).astype(np.float32)
             for nch, n, s in [(2, unit + 11, 0.1), (1, 777, 0.1), (3, 2 * unit + 5, 0.6)]]
    b = Batch(lc, flt, files)
    b.items.set_fusion(PARTS)
    assert b.items.filter_launches() == (3, 2 * 2 + 1 + 3 * 3)
    pk = torch.zeros(3, dtype=torch.float32, device="cuda")

    def step(s):
        lc.peak_reset_dev(pk, 3, s.cuda_stream)
        b.items.filter_dev(pk, s.cuda_stream)

    # a stream without an eager call: the capture may not allocate the scratch
    cold = torch.cuda.Stream()
    refused = None
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=cold):
        try:
            step(cold)
        except lc.LcfirError as e:
            refused = e
    del g0
    torch.cuda.synchronize()
    assert refused is not None and refused.code == lc.EINVAL
    assert "scratch" in str(refused) and "graph capture" in str(refused), str(refused)

    s = torch.cuda.Stream()
    step(s)
    torch.cuda.synchronize()
    want, want_pk = b.outputs(), pk.cpu().numpy().copy()
    for f, x in enumerate(files):
        assert same_bits(want[f], per_file_reference(lc, flt, x)[0]), f
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step(s)
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


# ---- 7: fallbacks under "parts" --------------------------------------------------
FALLBACKS = ["direct15", "register_kernel_4001", "chunk_below_longest_row", "seg_len_changed_after_create"]


@pytest.mark.parametrize("which", FALLBACKS)
def test_fallbacks_take_the_group_path(lc, oracle_mod, which):
    if which == "direct15":
        taps, flt = gi.make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
        assert flt.method == "direct"
    elif which == "register_kernel_4001":
        taps, flt = gi.make_filter(lc, oracle_mod, 4001, "fft", None, None, 0.0)
        assert flt.fft_info["parts"] == 1 and flt.fft_units["kernel"] == "l32_reg"
    else:
        taps, flt = form_filter(lc, oracle_mod, "l16_parts2")
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=len(taps) + 2)
    b = Batch(lc, flt, files)
    b.items.set_fusion(PARTS)
    if which == "chunk_below_longest_row":
        assert b.items.filter_launches() == (2, 33)
        flt.set_fft_tuning(seg_len=16384, chunk=2 * unit)  # the longest row has 3 U - 1 frames
        assert flt.fft_units["outputs"] == unit and flt.fft_info["parts"] == 2 and max(b.n) > 2 * unit
    elif which == "seg_len_changed_after_create":
        assert b.items.filter_launches() == (2, 33)
        flt.set_fft_tuning(seg_len=32768)
        flt.set_fft_family("lds")  # an LDS-column kernel: only the B differs from the table's
        assert flt.fft_units["kernel"] == "l32_park" and flt.fft_units["outputs"] != unit
    assert b.items.filter_launches() == (b.items.info()["launches"], 0) == (3, 0)
    refs = [per_file_reference(lc, flt, x) for x in files]  # under the tuning the set now runs with
    b.run()
    for f, (ref, y) in enumerate(zip(refs, b.outputs())):
        assert same_bits(y, ref[0]), (which, f)
    assert same_bits(b.peaks(), file_peaks(refs))
    b.close()


def test_a_single_partition_plan_runs_autos_launch(lc, oracle_mod):
    taps, flt = gf.form_filter(lc, oracle_mod, "l16_zero_201")
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=len(taps) + 3)
    b = Batch(lc, flt, files)
    b.items.set_fusion(AUTO)
    assert b.items.filter_launches() == (1, 33)
    b.items.set_fusion(PARTS)
    assert b.items.filter_launches() == (1, 33)
    refs = [per_file_reference(lc, flt, x) for x in files]
    b.run()
    for f, (ref, y) in enumerate(zip(refs, b.outputs())):
        assert same_bits(y, ref[0]), f
    assert same_bits(b.peaks(), file_peaks(refs))
    b.close()


# ---- 8: the other modes are what they were ---------------------------------------
def test_auto_and_the_unknown_mode_are_unchanged(lc, oracle_mod):
    taps, flt = form_filter(lc, oracle_mod, "park_parts2")
    unit, half = gi.unit_of(flt), (len(taps) - 1) // 2
    files = gi.make_files(unit, half, seed=1)
    n, nch = [x.shape[1] for x in files], [x.shape[0] for x in files]
    items = lc.ItemSet(flt, n, nch)
    launches = items.info()["launches"]
    items.set_fusion(AUTO)
    assert items.filter_launches() == (launches, 0)  # a partitioned plan under AUTO: the per-group path
    items.set_fusion(PARTS)
    assert items.filter_launches() == (2, unit_total(unit, files))
    items.set_fusion(GROUPS)
    assert items.filter_launches() == (launches, 0)
    lib = lc.load()
    assert lib.lcfir_items_set_fusion(items._h, 2) == lc.EINVAL
    assert items.filter_launches() == (launches, 0)  # a refused mode changes nothing
    assert lib.lcfir_items_set_fusion(items._h, 3) == lc.OK
    assert items.filter_launches() == (2, unit_total(unit, files))
    assert lib.lcfir_items_set_fusion(items._h, 4) == lc.EINVAL and lib.lcfir_items_set_fusion(items._h, -1) == lc.EINVAL
    items.close()
