"""CPU tests of lcfir_items_plan, the pure layout rule of an item set
(include/lcfir.h): the library's plan against a restatement of the rule in
numpy, for the unit sizes the kernels have (4 096 outputs for the direct
form, 16 384 - 200 and 32 768 - 4 000 for two FFT plans) and frame counts
either side of every unit boundary."""
import itertools

import numpy as np
import pytest

import lcfir

UNITS = [4096, 16184, 28768]
MAX_ROWS = 65535


def restate(unit, n, nch):
    """The rule, straight from the header: key ceil(n / unit), groups in
    ascending key, files in input order, stride N_g rounded up to 4 floats,
    groups packed back to back from offset 0."""
    n, nch = np.asarray(n, np.int64), np.asarray(nch, np.int64)
    key = -(-n // unit)
    live = (n > 0) & (nch > 0)
    keys = sorted(set(key[live].tolist()))
    group = np.full(n.size, -1, np.int64)
    off = np.zeros(n.size, np.int64)
    stride = np.zeros(n.size, np.int64)
    gn, gfirst, grows = [], [], []
    arena = rows = launches = 0
    for g, k in enumerate(keys):
        members = [f for f in range(n.size) if live[f] and key[f] == k]
        n_g = int(n[members].max())
        s_g = (n_g + 3) // 4 * 4
        gn.append(n_g)
        gfirst.append(rows)
        grows.append(int(nch[members].sum()))
        in_launch = 0
        launches += 1
        for f in members:
            if in_launch + nch[f] > MAX_ROWS:
                launches += 1
                in_launch = 0
            in_launch += int(nch[f])
            group[f], off[f], stride[f] = g, arena, s_g
            arena += int(nch[f]) * s_g
            rows += int(nch[f])
    return {"file_group": group, "file_offset": off, "file_stride": stride, "group_n": np.array(gn, np.int64),
            "group_first_row": np.array(gfirst, np.int64), "group_rows": np.array(grows, np.int64),
            "groups": len(keys), "launches": launches, "rows": rows, "arena_floats": arena}


def check(unit, n, nch):
    n, nch = np.asarray(n, np.int64), np.asarray(nch, np.int32)
    got = lcfir.ItemSet.plan(unit, n, nch)
    want = restate(unit, n, nch)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    live = (n > 0) & (nch > 0)
    key = -(-n // unit)
    # groups equal the distinct keys, in ascending order
    assert got["groups"] == len(set(key[live].tolist()))
    gkeys = [set(key[(got["file_group"] == g)].tolist()) for g in range(got["groups"])]
    assert all(len(s) == 1 for s in gkeys)
    assert [s.pop() for s in gkeys] == sorted(set(key[live].tolist()))
    assert np.all(got["file_group"][~live] == -1)
    # alignment: every row starts a multiple of 4 floats into the arena
    assert np.all(got["file_offset"][live] % 4 == 0) and np.all(got["file_stride"][live] % 4 == 0)
    # stride >= N_g >= n
    for f in np.nonzero(live)[0]:
        n_g = got["group_n"][got["file_group"][f]]
        assert got["file_stride"][f] >= n_g >= n[f]
        assert got["file_stride"][f] - n_g < 4
    # no two rows overlap, none leaves the arena, and the arena has no slack
    spans = sorted((int(got["file_offset"][f]), int(got["file_offset"][f] + nch[f] * got["file_stride"][f]))
                   for f in np.nonzero(live)[0])
    for (a0, a1), (b0, b1) in zip(spans[:-1], spans[1:]):
        assert a1 <= b0
    if spans:
        assert spans[0][0] == 0 and spans[-1][1] == got["arena_floats"]
        assert sum(b - a for a, b in spans) == got["arena_floats"]
    else:
        assert got["arena_floats"] == 0
    assert got["rows"] == int(nch[live].sum())
    return got


@pytest.mark.parametrize("unit", UNITS)
def test_plan_unit_boundaries(unit):
    frames = [0, 1, unit - 1, unit, unit + 1, 2 * unit, 3 * unit - 1]
    # every frame count with every channel count, then duplicates in another order
    pairs = list(itertools.product(frames, [0, 1, 2, 3]))
    pairs += [(unit + 1, 2), (1, 1), (3 * unit - 1, 3), (unit, 1), (unit + 1, 1)]
    n, nch = [p[0] for p in pairs], [p[1] for p in pairs]
    got = check(unit, n, nch)
    # keys present: 1 (1, unit - 1, unit), 2 (unit + 1, 2 unit), 3 (3 unit - 1)
    assert got["groups"] == 3 and got["launches"] == 3
    assert got["group_n"].tolist() == [unit, 2 * unit, 3 * unit - 1]


@pytest.mark.parametrize("unit", UNITS)
def test_plan_random_batches(unit):
    rng = np.random.default_rng(unit)
    for _ in range(20):
        nf = int(rng.integers(1, 60))
        n = rng.integers(0, 5 * unit, nf)
        n[rng.integers(0, nf, 3)] = rng.choice([0, unit, 2 * unit, unit - 1])
        nch = rng.integers(0, 4, nf)
        check(unit, n, nch)


def test_plan_is_deterministic_and_order_preserving():
    unit = 4096
    n = [5000, 100, 5001, 200, 4999, 8192]
    nch = [1, 2, 1, 2, 1, 1]
    got = check(unit, n, nch)
    # group 0 (one unit): files 1, 3 in input order; group 1 (two units): 0, 2, 4, 5
    assert got["file_group"].tolist() == [1, 0, 1, 0, 1, 1]
    assert got["file_offset"][1] < got["file_offset"][3] < got["file_offset"][0] < got["file_offset"][2] \
        < got["file_offset"][4] < got["file_offset"][5]
    again = lcfir.ItemSet.plan(unit, n, nch)
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(again[k])) for k in got)


def test_plan_cuts_large_groups_between_files():
    """A synthetic 70 000-row group: 23 334 three-channel files of one unit.
    65 535 is a multiple of 3, so a second case with a two-channel file in
    front makes the cut fall inside a file unless the planner moves it."""
    unit = 4096
    for lead in ([], [2]):
        nch = np.array(lead + [3] * 23334, np.int32)
        n = np.full(nch.size, 1000, np.int64)
        got = check(unit, n, nch)
        assert got["groups"] == 1 and got["rows"] == int(nch.sum()) >= 70000
        assert got["launches"] == 2
        # replay the cut: whole files only, consecutive, each launch <= 65 535 rows
        in_launch, launches = 0, 1
        for c in nch:
            if in_launch + c > MAX_ROWS:
                launches, in_launch = launches + 1, 0
            in_launch += int(c)
            assert in_launch <= MAX_ROWS
        assert launches == got["launches"]


def test_plan_empty_and_all_empty():
    got = check(4096, [], [])
    assert got["groups"] == 0 and got["launches"] == 0 and got["rows"] == 0
    got = check(4096, [0, 10, 0], [2, 0, 0])
    assert got["groups"] == 0 and got["arena_floats"] == 0


def test_plan_rejects_bad_arguments():
    lib = lcfir.load()
    n = np.array([10], np.int64)
    c = np.array([1], np.int32)
    args = [None] * 10
    assert lib.lcfir_items_plan(0, 1, n.ctypes.data, c.ctypes.data, *args) == lcfir.EINVAL
    assert b"unit" in lib.lcfir_last_error()
    assert lib.lcfir_items_plan(4096, 1, None, c.ctypes.data, *args) == lcfir.EINVAL
    assert lib.lcfir_items_plan(4096, -1, n.ctypes.data, c.ctypes.data, *args) == lcfir.EINVAL
    bad = np.array([-1], np.int64)
    assert lib.lcfir_items_plan(4096, 1, bad.ctypes.data, c.ctypes.data, *args) == lcfir.EINVAL
    assert b"negative" in lib.lcfir_last_error()
    many = np.array([65536], np.int32)
    assert lib.lcfir_items_plan(4096, 1, n.ctypes.data, many.ctypes.data, *args) == lcfir.EINVAL
    assert b"channels" in lib.lcfir_last_error()
    huge = np.array([2**62, 2**62], np.int64)
    two = np.array([3, 3], np.int32)
    assert lib.lcfir_items_plan(4096, 2, huge.ctypes.data, two.ctypes.data, *args) == lcfir.EINVAL
    # every output is optional
    assert lib.lcfir_items_plan(4096, 1, n.ctypes.data, c.ctypes.data, *args) == lcfir.OK


def test_item_calls_reject_null_handles():
    lib = lcfir.load()
    out = lcfir.ctypes.c_void_p()
    n = np.array([10], np.int64)
    c = np.array([1], np.int32)
    assert lib.lcfir_items_create(None, n.ctypes.data, c.ctypes.data, 1, lcfir.ctypes.byref(out)) == lcfir.EINVAL
    assert b"ctx" in lib.lcfir_last_error() and not out.value
    assert lib.lcfir_items_create(None, n.ctypes.data, c.ctypes.data, 1, None) == lcfir.EINVAL
    assert lib.lcfir_items_filter_dev(None, None, None) == lcfir.EINVAL
    assert lib.lcfir_items_normalize_dev(None, None, 0, None) == lcfir.EINVAL
    assert lib.lcfir_items_decode_pcm_dev(None, None, None, None, None) == lcfir.EINVAL
    assert lib.lcfir_items_encode_pcm_scaled_dev(None, None, 0, None, None, None, None) == lcfir.EINVAL
    assert lib.lcfir_items_destroy(None) == lcfir.OK
