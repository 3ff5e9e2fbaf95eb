"""DELTA with 24-bit value fields (stream_tiles.h: kRecordBytes24), host builder, no GPU: the packed image is decoded in numpy
(tests/delta24_decoder.py), walked by the kernel emulation and compared with the oracle bit for bit; every case asserts that it was reached.
The matrices: tests/delta24_cases.py.  32 workgroups, forced delta24, fixed point unless a case says otherwise.
"""
import numpy as np
import pytest

import delta24_cases as dc
import delta24_decoder as dd

WORKGROUPS = 32


def test_values_below_one_pack_at_shift_zero_without_outliers():
    c = dc.below_one()
    t, plain = dc.build(c.cp, 0, "delta24", WORKGROUPS), dc.build(c.cp, 0, "delta32", WORKGROUPS)
    assert t["format"] == "delta" and t["value_bits"] == 24 and t["value_shift"] == 0
    assert plain["format"] == "delta" and plain["value_bits"] == 32 and plain["image"].size == dc.records(plain) * 768
    assert not t["blocks"]["outlier_count"].any() and dd.outlier_lists(t) == {}
    assert t["image"].size == dc.records(t) * 640 and dc.records(t) == dc.records(plain)
    unpacked, found = dd.unpack(t)
    assert found == [] and unpacked["image"].tobytes() == plain["image"].tobytes()      # the same dealing, slot for slot
    assert np.array_equal(dd.run(t, 0, c.xw, c.cp.num_rows), c.want)
    for part in range(c.cp.num_row_partitions):                                          # hs_run_partition's walk of the chains
        rows = slice(part * 128 * dc.OB_BANK, (part + 1) * 128 * dc.OB_BANK)
        got = dd.run(t, 0, c.xw, c.cp.num_rows, row_part_filter=part, rows_per_part=128 * dc.OB_BANK)
        assert np.array_equal(got[rows], c.want[rows])
    assert c.cp.num_row_partitions == 4


def test_planted_outliers_go_to_their_blocks_lists():
    p = dc.planted(WORKGROUPS)
    t = dc.build(p.cp, 0, "delta24", WORKGROUPS)
    assert t["value_bits"] == 24 and t["value_shift"] == 0
    assert dc.found_outliers(t) == p.outliers and len(p.outliers) == 8           # exactly those eight; their stream fields are 0 (unpack asserts it)
    assert int(t["blocks"]["outlier_count"].sum()) == 8 and t["image"].size == dc.records(t) * 640 + 8 * 12
    assert dd.unpack(t)[0]["image"].tobytes() == dc.build(p.cp, 0, "delta32", WORKGROUPS)["image"].tobytes()      # the picked slots are where they were
    assert p.want[p.saturated_row] == 0xFFFFFFFF
    assert np.array_equal(dd.run(t, 0, p.xw, p.cp.num_rows), p.want)


def test_integer_values_pack_at_shift_eight():
    c = dc.integers()
    t = dc.build(c.cp, 0, "delta24", WORKGROUPS)
    assert t["value_bits"] == 24 and t["value_shift"] == 8 and not t["blocks"]["outlier_count"].any()
    assert t["image"].size == dc.records(t) * 640
    assert 0 < c.want.max() < 0xFFFFFFFF
    assert np.array_equal(dd.run(t, 0, c.xw, c.cp.num_rows), c.want)


def test_too_many_outliers_keep_the_plain_record():
    c = dc.over_the_cap()
    t, plain = dc.build(c.cp, 0, "delta24", WORKGROUPS), dc.build(c.cp, 0, "delta32", WORKGROUPS)
    assert (c.m.nnz // 1000) * 4096 > t["elements"]                               # more than one outlier per 4096 element slots
    assert t["format"] == "delta" and t["value_bits"] == 32 and dc.same(t, plain)
    assert np.array_equal(dd.run(t, 0, c.xw, c.cp.num_rows), c.want)


def test_head_positions_beyond_24_bits():
    c = dc.tall(40000)
    t = dc.build(c.cp, 0, "delta24", WORKGROUPS, col_slices=2)
    assert t["value_bits"] == 24 and t["col_slices"] == 2 and t["blocks"]["nrows"].max() >= 2300
    assert max(int(r.head.max()) for r in dd.runs(t)) >= 1 << 24
    assert np.array_equal(dd.run(t, 0, c.xw, c.cp.num_rows), c.want)


@pytest.mark.parametrize("impl", [1, 2])
def test_float_modes_keep_the_plain_record(impl):
    # (the other refusal, a load with the value map asked for, needs the device builder: tests/test_gpu_delta24.py)
    c = dc.float_case(impl)
    t, plain = dc.build(c.cp, impl, "delta24", WORKGROUPS), dc.build(c.cp, impl, "delta32", WORKGROUPS)
    assert t["format"] == "delta" and t["value_bits"] == 32 and dc.same(t, plain)


def test_the_saved_bytes_rule_leaves_a_small_image_as_it_was():
    c = dc.below_one()
    plain, by_rule, forced = (dc.build(c.cp, 0, f, WORKGROUPS) for f in ("delta32", "delta", "delta24"))
    assert by_rule["value_bits"] == 32 and dc.same(by_rule, plain)
    assert 0 < plain["image"].size - forced["image"].size < 23 << 20             # what packing would save: far below kDelta24MinSavedBytes
    unforced = dc.build(c.cp, 0, None, WORKGROUPS)                                 # and whatever the planner itself picks carries no packed record
    assert unforced["value_bits"] in (0, 32) and not unforced["blocks"]["value_bits"].any()
