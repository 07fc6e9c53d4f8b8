"""GPU tests of LCFIR_ITEMS_FUSION_LANES (set_fusion("lanes")): the per-group
path's launches dealt to the caller's stream and three streams of the ctx's,
forked and joined inside lcfir_items_filter_dev.  The mode changes where the
launches are queued, never what they compute, so everything is compared bit
for bit: with the same item set under "groups", and with the per-file entry
point (lcfir_filter_channels_dev and its fused peaks).

Forms: the register kernel (4 001 taps), the L = 16 384 kernel (201 taps) and
the smallest partitioned park plan of tests/test_gpu_items_parts.py (38 401
taps, two partitions: a group is two launches, which stay in order on one
lane, and every lane needs a partial-sum scratch of its own).  Files, B = the
plan's unit: one per key 1 ... 6 (k B - r) and two more in keys 1 and 2, so six
groups: the lanes wrap, and lanes 0 and 1 carry two group launches each.
"""
import numpy as np
import pytest

import test_gpu_items as gi
import test_gpu_items_fused as gf
from test_gpu_items import Batch, d2h, h2d, same_bits

pytestmark = pytest.mark.gpu

SENTINEL = gf.SENTINEL
# name: taps, then the plan it must give (kernel, partitions)
FORMS = {"reg_4001": (4001, "l32_reg", 1), "l16_zero_201": (201, "l16", 1), "park_parts2": (38401, "l32_park", 2)}


@pytest.fixture(scope="module")
def lc():
    import torch  # before lcfir: one HIP runtime in the process
    import lcfir
    assert torch.cuda.is_available() and lcfir.device_count() >= 1, "no GPU visible"
    return lcfir


def make_files(unit, seed):
    rng = np.random.default_rng(seed)
    ns = [unit - 1, 2 * unit, 3 * unit - 5, 4 * unit - 1, 5 * unit, 6 * unit - 7, 1, 2 * unit - 3]
    return [np.ascontiguousarray((rng.integers(-2**23, 2**23, size=(1 + f % 3, n)) / 2.0**23 * 0.4)
                                 .astype(np.float32)) for f, n in enumerate(ns)]


def form_filter(lc, oracle_mod, name):
    ntaps, kernel, parts = FORMS[name]
    taps, flt = gi.make_filter(lc, oracle_mod, ntaps, "fft", None, None, 0.0)
    assert flt.fft_units["kernel"] == kernel and flt.fft_info["parts"] == parts, (name, flt.fft_units, flt.fft_info)
    return flt


def run_into_sentinel(lc, b, base, total):
    h2d(lc, base, np.full(total, SENTINEL, np.uint32))
    b.run()
    return b.outputs(), b.peaks(), d2h(lc, base, total, np.uint32)


@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def case(request, lc, oracle_mod):
    """Per form, computed once and left unchanged: the per-file references,
    the item set's runs under "groups" and "lanes" (each into a
    sentinel-filled output arena, "lanes" twice), two item sets of the ctx on
    two streams back to back, and a run on a fresh ctx after the first is
    closed."""
    import torch
    name = request.param
    flt = form_filter(lc, oracle_mod, name)
    unit = gi.unit_of(flt)
    files = make_files(unit, seed=FORMS[name][0])
    refs = gf.filter_references(lc, flt, files)
    b = Batch(lc, flt, files)
    base, plan = gf.arena(lc, b, unit)
    total = int(plan["arena_floats"])
    launches_groups = b.items.filter_launches()
    groups = run_into_sentinel(lc, b, base, total)
    b.items.set_fusion("lanes")
    launches_lanes = b.items.filter_launches()
    lanes = run_into_sentinel(lc, b, base, total)
    lanes2 = run_into_sentinel(lc, b, base, total)
    info = b.items.info()

    # two item sets of this ctx, each on a stream of its own, back to back
    files2 = files[::-1]
    b2 = Batch(lc, flt, files2)
    b2.items.set_fusion("lanes")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pk1 = torch.zeros(len(files), dtype=torch.float32, device="cuda")
    pk2 = torch.zeros(len(files), dtype=torch.float32, device="cuda")
    for bb in (b, b2):  # the outputs must come from the two calls below
        bb_base, _ = gf.arena(lc, bb, unit)
        h2d(lc, bb_base, np.full(total, SENTINEL, np.uint32))
    torch.cuda.synchronize()
    b.items.filter_dev(pk1, s1.cuda_stream)
    b2.items.filter_dev(pk2, s2.cuda_stream)
    torch.cuda.synchronize()
    two = (b.outputs(), pk1.cpu().numpy(), b2.outputs(), pk2.cpu().numpy())

    # under capture the mode is refused (the stream has run eagerly: only the fork is in the way)
    refused = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s1):
        lc.peak_reset_dev(pk1, len(files), s1.cuda_stream)
        try:
            b.items.filter_dev(pk1, s1.cuda_stream)
        except lc.LcfirError as e:
            refused = e
    del g
    torch.cuda.synchronize()
    b.items.set_fusion(4)  # the mode by its number
    after_capture = run_into_sentinel(lc, b, base, total)

    # close everything of this ctx, then a fresh one: the lanes and their scratch went in order
    b.close()
    b2.close()
    flt.close()
    flt2 = form_filter(lc, oracle_mod, name)
    b3 = Batch(lc, flt2, files)
    b3.items.set_fusion("lanes")
    b3.run()
    fresh = (b3.outputs(), b3.peaks())
    b3.close()
    flt2.close()
    return dict(name=name, unit=unit, files=files, refs=refs, plan=plan, info=info, groups=groups, lanes=lanes,
                lanes2=lanes2, launches_groups=launches_groups, launches_lanes=launches_lanes, two=two,
                refused=refused, after_capture=after_capture, fresh=fresh)


def file_peaks(refs):
    return np.array([r[1].max() if r[1].size and r[0].size else 0.0 for r in refs], np.float32)


def assert_equals_refs(ys, pk, refs, what):
    for f, (y, ref) in enumerate(zip(ys, refs)):
        assert same_bits(y, ref[0]), (what, f)
    assert same_bits(pk, file_peaks(refs)), (what, pk)


def test_six_groups_on_four_lanes(case):
    assert case["info"]["groups"] == case["info"]["launches"] == 6
    assert case["launches_lanes"] == case["launches_groups"] == (6, 0)


def test_lanes_equal_groups_and_the_per_file_calls(case):
    assert_equals_refs(case["groups"][0], case["groups"][1], case["refs"], (case["name"], "groups"))
    for key in ("lanes", "lanes2", "after_capture"):
        assert_equals_refs(case[key][0], case[key][1], case["refs"], (case["name"], key))
        # the whole arena, ringing tails and untouched gaps included, is what "groups" leaves
        assert np.array_equal(case[key][2], case["groups"][2]), (case["name"], key)


def test_nothing_outside_the_groups_rows_is_written(case):
    plan = case["plan"]
    written = np.zeros(int(plan["arena_floats"]), bool)
    for f, x in enumerate(case["files"]):
        g = int(plan["file_group"][f])
        for c in range(x.shape[0]):
            o = int(plan["file_offset"][f] + c * plan["file_stride"][f])
            written[o:o + int(plan["group_n"][g])] = True
    assert (~written).sum() > 0  # there is padding to look at
    for key in ("groups", "lanes", "lanes2"):
        assert np.all(case[key][2][~written] == SENTINEL), (case["name"], key)
        assert not np.any(case[key][2][written] == SENTINEL), (case["name"], key)


def test_two_item_sets_on_two_streams(case):
    y1, pk1, y2, pk2 = case["two"]
    assert_equals_refs(y1, pk1, case["refs"], (case["name"], "stream 1"))
    assert_equals_refs(y2, pk2, case["refs"][::-1], (case["name"], "stream 2"))


def test_capture_is_refused(case, lc):
    e = case["refused"]
    assert e is not None and e.code == lc.EINVAL and "captured" in str(e), str(e)


def test_a_fresh_ctx_after_close(case):
    assert_equals_refs(case["fresh"][0], case["fresh"][1], case["refs"], (case["name"], "fresh ctx"))


def test_unknown_modes_stay_unknown(lc, oracle_mod):
    _, flt = gi.make_filter(lc, oracle_mod, 15, "direct", None, None, 0.0)
    items = lc.ItemSet(flt, [100, 5000], [1, 2])
    items.set_fusion("lanes")
    items.set_fusion(4)
    for bad in (2, 5, -1):
        with pytest.raises(lc.LcfirError) as e:
            items.set_fusion(bad)
        assert e.value.code == lc.EINVAL
    # the direct method runs under the mode too (two groups, two lanes)
    x = [np.linspace(-0.3, 0.3, 100, dtype=np.float32)[None], np.ones((2, 5000), np.float32) * np.float32(0.25)]
    b = Batch(lc, flt, x)
    b.run()
    want = b.outputs(), b.peaks()
    b.items.set_fusion("lanes")
    b.run()
    for f in range(2):
        assert same_bits(b.outputs()[f], want[0][f]), f
    assert same_bits(b.peaks(), want[1])
    b.close()
    items.close()
