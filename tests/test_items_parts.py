"""CPU tests of the fused partitioned item-set mode's host side: the mode's
value in the header and the binding, batch.ItemBatch's handling of the name,
and the launch-count rule of lcfir_items_filter_launches restated over
lcfir_items_unit_table for the forms tests/test_gpu_items_parts.py runs."""
import os
import re

import numpy as np
import pytest

import batch
import check_resources
import lcfir
from test_items_batch import StubBackend, make_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMARKS = os.path.join(ROOT, "audio-fir-filter_amd", "liblcfir.remarks")
# (taps, outputs per unit B, partitions) of the four partitioned forms
FORMS = {"l16_parts2": (14339, 9214, 2), "l16_parts3": (20001, 9718, 3),
         "park_parts2": (38401, 13568, 2), "park_parts3": (45001, 17768, 3)}


def test_the_header_defines_the_mode_as_3():
    text = open(os.path.join(ROOT, "include", "lcfir.h")).read()
    modes = dict(re.findall(r"^#define LCFIR_ITEMS_FUSION_(\w+) (\d+)$", text, re.M))
    assert modes == {"AUTO": "0", "GROUPS": "1", "PARTS": "3"}  # 2 stays unknown


def test_the_binding_names_the_mode():
    assert lcfir.ITEMS_FUSION["parts"] == 3
    assert lcfir.ITEMS_FUSION == {"auto": 0, "groups": 1, "parts": 3}


class FusionStub(StubBackend):
    def set_fusion(self, mode):
        self.calls.append(("fusion", mode))


@pytest.mark.parametrize("mode", ["auto", "groups", "parts"])
def test_item_batch_passes_the_mode_on(mode):
    be = FusionStub()
    ib = batch.ItemBatch(be, make_files(), fusion=mode)
    assert ib.fusion == mode and be.calls[0] == ("fusion", mode)  # before the arena is loaded
    ib.step()
    assert [c for c in be.calls if isinstance(c, tuple) and c[0] == "fusion"] == [("fusion", mode)]


@pytest.mark.parametrize("bad", ["part", "PARTS", "", "2", "fused"])
def test_item_batch_rejects_an_unknown_name(bad):
    be = FusionStub()
    with pytest.raises(ValueError) as e:
        batch.ItemBatch(be, make_files(), fusion=bad)
    assert all(f"'{name}'" in str(e.value) for name in ("auto", "groups", "parts")), str(e.value)
    assert be.calls == []  # nothing was planned or set


def standard_lengths(unit, half):
    """The frame counts and channel counts of test_gpu_items.make_files."""
    ns = [0, 1, half, unit - 1, unit, unit + 1, 2 * unit, 2 * unit + 37, 3 * unit - 1, unit + 1]
    return ns, [1 + f % 3 for f in range(len(ns))]


def launches(parts, units, max_units):
    """lcfir_items_filter_launches on the fused partitioned path: one launch
    per partition and slice of at most max_units table entries."""
    per = max_units if 1 <= max_units < 2**31 else 2**31 - 1
    return parts * -(-units // per), units


@pytest.mark.parametrize("name", list(FORMS))
def test_launch_count_rule_over_the_unit_table(name):
    ntaps, B, parts = FORMS[name]
    half = (ntaps - 1) // 2
    n, nch = standard_lengths(B, half)
    table = lcfir.ItemSet.unit_table(B, n, nch)
    units = sum(c * -(-m // B) for m, c in zip(n, nch))
    assert table.size == units
    # half <= B: the standard 33 units; the 96 kHz default filter's half (19 200) spans two units
    assert units == (33 if half <= B else 33 + nch[2] * (-(-half // B) - 1))
    assert launches(parts, units, 0) == (parts, units)  # no max_units tuning: one launch per partition
    for per in (1, 7, units - 1, units, units + 1, 128):
        slices = [table[u0:u0 + per] for u0 in range(0, units, per)]
        assert sum(s.size for s in slices) == units and all(0 < s.size <= per for s in slices)
        assert launches(parts, units, per) == (parts * len(slices), units)
    # every row's entries carry the row's own n <= one chunk of a partitioned plan (2^26 outputs,
    # whole units), so the standard files are eligible
    span = max(B, (1 << 26) // B * B)
    assert int(table["n"].max()) == max(n) <= span


def test_partition_item_entry_points_in_the_build_remarks():
    """The item form of the partition modes has entry points of its own, one
    instance per mode (first, add, last = 1, 2, 3) for each LDS-column kernel;
    the L = 16 384 ones use no scratch.  fir_fft_f64_kernel and
    fir_fft32_f64_kernel keep the instances they had: tests/test_items_units.py
    pins their item forms, the partition modes' plain forms are counted here."""
    lcfir.load()  # the library's own make writes the remarks next to it
    assert os.path.exists(REMARKS), "liblcfir.so without its remarks: rebuild with make -C audio-fir-filter_amd"
    k = check_resources.parse(open(REMARKS).read())
    l16 = {n: f for n, f in k.items() if "fir_fft_items_parts_kernel" in n}
    park = {n: f for n, f in k.items() if "fir_fft32_items_parts_kernel" in n}
    for got in (l16, park):
        assert len(got) == 3, sorted(got)
        assert all(any(f"kernelILi{m}EEEv" in n for n in got) for m in (1, 2, 3)), sorted(got)
    for n, f in l16.items():
        assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (n, f)
    for n, f in park.items():
        assert f["SGPRs Spill"] == 0, (n, f)
    # the plain partition forms are still there, and no item form of them under the old names
    for kernel, flags in (("fir_fft_f64_kernel", "Lb0ELb0E"), ("fir_fft32_f64_kernel", "Lb0E")):
        for m in (1, 2, 3):
            assert sum(kernel in n and f"ILi{m}E{flags}EEv" in n for n in k) == 1, (kernel, m)
            assert not any(kernel in n and f"ILi{m}E" in n and "Lb1EEEv" in n for n in k), (kernel, m)
