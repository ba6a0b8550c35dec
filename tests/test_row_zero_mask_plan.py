"""Zero mask of the trace row hash (DESIGN.md §4 "Row hash"): the host routine that marks, per
partition and folded column pair, the zero columns the prefix row kernel does not load, against a
short restatement; and the share of loads it marks at the headline plan.  No device."""
import random

import numpy as np

import zkl_hip

GEN = zkl_hip.COL_GENERAL
PAIRS_MAX = 64  # mask capacity per partition


def _periods(cols, p_max=128):
    """numpy restatement of the column scan: 0 all-zero, smallest power-of-two period, GEN."""
    out = []
    for col in cols:
        if not col.any():
            out.append(0)
            continue
        per, p = GEN, 1
        while p <= min(p_max, col.shape[0]):
            if (col.reshape(-1, p, 2) == col[:p]).all():
                per = p
                break
            p *= 2
        out.append(per)
    return out


def _bench_periods(oracle):
    """Column classes of synth_vm_segment(0x5EED0001, 16), the headline segment: the 2^10-row
    segment of the same seed has the same classes (tests/test_column_structure.py)."""
    t, _, w = oracle.synth_segment(0x5EED0001, 10, 0)
    return _periods(np.frombuffer(t, dtype=np.uint64).reshape(w, 1 << 10, 2))


def _partitions(per, np_, rate=16):
    ncols = len(per)
    psize = ncols if np_ == 1 else max(-(-ncols // np_), rate)
    return [per[c:c + psize] for c in range(0, ncols, psize)]


def _mask_ref(per, np_, rate=16):
    """The rule restated: bit j of even = column 2j of the partition has period 0; bit j of odd =
    column 2j + 1 has period 0 or does not exist; (0, 0) past 64 pairs; None past 9 partitions."""
    parts = _partitions(per, np_, rate)
    if len(parts) > 9:
        return None
    out = []
    for cols in parts:
        pairs = (len(cols) + 1) // 2
        if pairs > PAIRS_MAX:
            out.append((0, 0))
            continue
        even = sum(1 << j for j in range(pairs) if cols[2 * j] == 0)
        odd = sum(1 << j for j in range(pairs) if 2 * j + 1 >= len(cols) or cols[2 * j + 1] == 0)
        out.append((even, odd))
    return tuple(out)


def test_mask_of_the_bench_segment(oracle):
    per = _bench_periods(oracle)
    assert len(per) == 204
    for np_ in (4, 2, 1, 9):
        assert zkl_hip.plan_row_zero_mask(per, np_, 16) == _mask_ref(per, np_), np_
    # one partition of 204 columns is 102 pairs: over the capacity, nothing masked
    assert zkl_hip.plan_row_zero_mask(per, 1, 16) == ((0, 0),)


def test_mask_marks_80_of_128_loads_at_the_headline(oracle):
    """Headline plan, lead (2, 0, 2, 0): partitions 0 and 2 still absorb their last block (columns
    38..50 of the partition, 13 loads each), partitions 1 and 3 all three blocks (51 loads each):
    128 column loads per row, of which the mask marks 80."""
    per = _bench_periods(oracle)
    lead, _ = zkl_hip.plan_row_prefix(per, 1 << 20, 16, 4, 16)
    assert lead == (2, 0, 2, 0)
    masks = zkl_hip.plan_row_zero_mask(per, 4, 16)
    loads = marked = 0
    for cols, k, (even, odd) in zip(_partitions(per, 4), lead, masks):
        pairs = (len(cols) + 1) // 2
        for j in range(pairs):
            if (j + 1) // 10 < k:  # pair j is sponge element j + 1: its block comes from the table
                continue
            loads += 1
            marked += (even >> j) & 1
            if 2 * j + 1 < len(cols):
                loads += 1
                marked += (odd >> j) & 1
    assert loads == 128
    assert marked == 80


def test_mask_crafted_partitions():
    # 51 columns, one partition: 26 pairs, the last one a lone column
    per = [GEN] * 51
    assert zkl_hip.plan_row_zero_mask(per, 1, 16) == ((0, 1 << 25),)  # absent odd column of pair 25
    per[50] = 0  # the lone last column zero
    assert zkl_hip.plan_row_zero_mask(per, 1, 16) == ((1 << 25, 1 << 25),)
    per[50], per[49], per[0], per[3] = GEN, 0, 0, 0
    assert zkl_hip.plan_row_zero_mask(per, 1, 16) == ((1, (1 << 25) | (1 << 24) | 2),)
    # constant and periodic columns are not zero
    per = [1, 32, 0, 128, 0, 0, GEN]
    assert zkl_hip.plan_row_zero_mask(per, 1, 16) == ((0b0110, 0b1100),)
    # two partitions of 51: the second one's columns are counted from its own start
    per = [GEN] * 102
    per[51], per[101] = 0, 0
    assert zkl_hip.plan_row_zero_mask(per, 2, 16) == ((0, 1 << 25), (1 | 1 << 25, 1 << 25))
    # exactly 64 pairs fit; 65 do not
    assert zkl_hip.plan_row_zero_mask([0] * 128, 1, 16) == (((1 << 64) - 1, (1 << 64) - 1),)
    assert zkl_hip.plan_row_zero_mask([0] * 127, 1, 16) == (((1 << 64) - 1, (1 << 64) - 1),)
    assert zkl_hip.plan_row_zero_mask([0] * 129, 1, 16) == ((0, 0),)
    # a partition wider than the capacity beside one that fits (140 + 100 columns)
    per = [0] * 240
    assert zkl_hip.plan_row_zero_mask(per, 2, 140) == ((0, 0), ((1 << 50) - 1, (1 << 50) - 1))
    # more than 9 partitions: no plan
    assert zkl_hip.plan_row_zero_mask([0] * 160, 10, 16) is None
    assert zkl_hip.plan_row_zero_mask([0] * 256, 16, 16) is None
    assert zkl_hip.plan_row_zero_mask([0] * 144, 9, 16) == (((1 << 8) - 1,) * 2,) * 9
    assert zkl_hip.plan_row_prefix([0] * 160, 1 << 16, 16, 10, 16)[0] == (0,) * 10


def test_mask_matches_the_rule_restated():
    rng = random.Random(0x3A5C)
    for _ in range(60):
        w = rng.choice([1, 7, 33, 51, 102, 127, 128, 129, 204, 212, 280])
        per = [rng.choice([0, 0, 0, 1, 2, 32, GEN, GEN]) for _ in range(w)]
        for np_ in (1, 2, 3, 4, 9, 10, 16):
            assert zkl_hip.plan_row_zero_mask(per, np_, 16) == _mask_ref(per, np_), (per, np_)


def test_mask_switch():
    lib = zkl_hip.load_library()
    prev = lib.zkl_hip_row_zero_mask()
    with zkl_hip.row_zero_mask(False):
        assert lib.zkl_hip_row_zero_mask() == 0
        with zkl_hip.row_zero_mask(True):
            assert lib.zkl_hip_row_zero_mask() == 1
        assert lib.zkl_hip_row_zero_mask() == 0
    assert lib.zkl_hip_row_zero_mask() == prev
    assert lib.zkl_hip_set_row_zero_mask(2) != 0
