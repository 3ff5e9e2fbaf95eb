"""DELTA with 24-bit value fields on the device (spmv_rowblock_kernel_delta24, gpu_tiles.hip: emit_delta24_kernel): the cases of tests/test_delta24_cpu.py
through hs_load_matrix and hs_load_matrix_csr against the oracle, bit for bit; the device builder's image against the host builder's, byte for byte;
and the packed image through every entry point that runs it.  Every test asserts that its case was reached.  The matrices: tests/delta24_cases.py.
"""
import numpy as np
import pytest

from hisparse_amd import device, host

import cases
import delta24_cases as dc
import delta24_decoder as dd
import option_variants as ov

pytestmark = pytest.mark.gpu

LOADS = ["cpsr", "csr"]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ov.option_keys():
        monkeypatch.delenv("HISPARSE_" + k, raising=False)


def engine(c, impl=0, how="cpsr", fmt="delta24", **options):
    """a context with the case's matrix loaded under STREAM_FORMAT = fmt (None: unforced) and further options"""
    eng = device.SpmvEngine(impl, ob_bank=c.cp.ob_bank, vb_bank=c.cp.vb_bank)
    if fmt:
        eng.set_option("stream_format", fmt)
    for k, v in options.items():
        eng.set_option(k, v)
    if how == "cpsr":
        eng.load_matrix(c.cp)
    else:
        eng.load_matrix_csr(host.CSRMatrix.from_scipy(c.m))
        assert (eng.num_rows, eng.num_cols) == (c.cp.num_rows, c.cp.num_cols)
    return eng


def run_once(eng, xw):
    eng.load_vector(xw)
    eng.run()
    return eng.read_result()


def assert_host_image(eng, c, **options):
    """the device builder's image, Block[] and Unit[] are the host builder's, byte for byte; returns the tiles read back"""
    st, got = eng.stats(), eng.read_tiles()
    assert st["retiled_on_gpu"] == 1
    want = dc.build(c.cp, 0, "delta24", st["num_compute_units"], **options)
    assert (got["value_bits"], got["value_shift"]) == (want["value_bits"], want["value_shift"]) and st["stream_bytes"] == want["image"].size
    assert got["blocks"].tobytes() == want["blocks"].tobytes(), "Block[] differs"
    assert got["units"].tobytes() == want["units"].tobytes(), "Unit[] differs"
    bad = np.nonzero(got["image"] != want["image"])[0]
    assert not bad.size, f"image differs at {bad.size} of {want['image'].size} bytes, first at {bad[:8]}"
    return dict(want, image=got["image"], blocks=got["blocks"], units=got["units"])


@pytest.mark.parametrize("how", LOADS)
def test_values_below_one(how):
    c = dc.below_one()
    with engine(c, how=how) as eng:
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "delta" and st["value_bits"] == 24
        t = assert_host_image(eng, c)
        assert t["value_shift"] == 0 and not t["blocks"]["outlier_count"].any() and st["stream_bytes"] == dc.records(t) * 640
        assert np.array_equal(run_once(eng, c.xw), c.want)


_UNITS = []


def compute_units():
    """the device's CU count = the workgroups its plans are made for (a loaded context reports it)"""
    if not _UNITS:
        with engine(dc.integers(), fmt="delta32") as eng:
            _UNITS.append(eng.stats()["num_compute_units"])
    return _UNITS[0]


@pytest.mark.parametrize("how", LOADS)
def test_planted_outliers(how):
    p = dc.planted(compute_units())      # (the slots are picked in the plan this device's builder makes)
    with engine(p, how=how) as eng:
        st = eng.stats()
        assert st["value_bits"] == 24
        t = assert_host_image(eng, p)
        assert t["value_shift"] == 0 and dc.found_outliers(t) == p.outliers and len(p.outliers) == 8
        assert st["stream_bytes"] == dc.records(t) * 640 + 8 * 12
        got = run_once(eng, p.xw)
        assert got[p.saturated_row] == 0xFFFFFFFF and np.array_equal(got, p.want)


@pytest.mark.parametrize("how", LOADS)
def test_integer_values_shift_eight(how):
    c = dc.integers()
    with engine(c, how=how) as eng:
        assert eng.stats()["value_bits"] == 24
        t = assert_host_image(eng, c)
        assert t["value_shift"] == 8 and not t["blocks"]["outlier_count"].any()
        assert np.array_equal(run_once(eng, c.xw), c.want)


@pytest.mark.parametrize("how", LOADS)
def test_too_many_outliers_keep_the_plain_record(how):
    c = dc.over_the_cap()
    with engine(c, how=how) as eng:
        st, packed_asked = eng.stats(), eng.read_tiles()
        assert device.STREAM_FORMATS[st["stream_format"]] == "delta" and st["value_bits"] == 32
        assert (c.m.nnz // 1000) * 4096 > st["stream_elements"]
        assert np.array_equal(run_once(eng, c.xw), c.want)
    with engine(c, how=how, fmt="delta32") as eng:
        plain = eng.read_tiles()
    assert dc.same(packed_asked, plain)


@pytest.mark.parametrize("how", LOADS)
def test_head_positions_beyond_24_bits(how):
    c = dc.tall(300000)
    with engine(c, how=how, col_slices="2") as eng:
        st = eng.stats()
        assert st["value_bits"] == 24 and st["col_slices"] == 2
        t = assert_host_image(eng, c, col_slices=2)
        assert t["blocks"]["nrows"].max() >= 2300
        heads = [int(r.head.max()) for r in dd.runs(dict(t, blocks=t["blocks"][:16]))]      # (the first blocks are enough: every row range is as tall)
        assert max(heads) >= 1 << 24
        assert np.array_equal(run_once(eng, c.xw), c.want)


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("how", LOADS)
def test_float_modes_keep_the_plain_record(how, impl):
    c = dc.float_case(impl)
    with engine(c, impl=impl, how=how) as eng:
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "delta" and st["value_bits"] == 32
        assert cases.float_close(run_once(eng, c.xw), c.want)


def test_value_map_keeps_the_plain_record_and_updates_keep_working():
    c = dc.integers()
    with engine(c, how="csr", value_map="1") as eng:
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "delta" and st["value_bits"] == 32      # packed was asked for; an updated value may not fit
        assert np.array_equal(run_once(eng, c.xw), c.want)
        values = (c.m.data * np.float32(0.37)).astype(np.float32)                                     # words that would not fit a 24-bit field at shift 8
        eng.update_values(values)
        eng.run()
        got = eng.read_result()
    m2 = c.m.copy()
    m2.data = values
    _, cp2 = cases.formatted(m2, 0, dc.VB_BANK, dc.OB_BANK, True)
    assert np.array_equal(got, dc.oracle_y(cp2, 0, c.xw))


@pytest.mark.parametrize("how", LOADS)
def test_the_saved_bytes_rule_leaves_a_small_image_as_it_was(how):
    c = dc.below_one()
    with engine(c, how=how, fmt="delta") as eng:
        st, by_rule = eng.stats(), eng.read_tiles()
        assert device.STREAM_FORMATS[st["stream_format"]] == "delta" and st["value_bits"] == 32
        assert np.array_equal(run_once(eng, c.xw), c.want)
    with engine(c, how=how, fmt="delta32") as eng:
        plain = eng.read_tiles()
    assert dc.same(by_rule, plain)
    with engine(c, how=how, fmt=None) as eng:          # the planner's own plan for it carries no packed record
        assert eng.stats()["value_bits"] in (0, 32)
        assert np.array_equal(run_once(eng, c.xw), c.want)


def _case_1_or_2(which):
    return dc.below_one() if which == "below one" else dc.planted(compute_units(), col_slices=2)


@pytest.mark.parametrize("which", ["below one", "planted"])
def test_every_entry_point_runs_the_packed_image(which):
    """hs_run_partition for every partition, hs_run_batch with the carried combine on and off, hs_iterate for three steps, both stream_resident values
    -- on a plan of two column slices, so that there is a combine pass to carry"""
    c = _case_1_or_2(which)
    scale, shift = dc.word(0.5), dc.word(0.001)
    x, ys = np.array(c.xw), []
    for _ in range(3):
        ys.append(dc.oracle_y(c.cp, 0, x))
        x = dc.feedback_reference(ys[-1], x, scale, shift)
    assert np.array_equal(ys[0], c.want)
    other_x = np.array(c.xw)[::-1].copy()
    for resident in ("0", "1"):
        for carry in ("0", "1"):
            with engine(c, col_slices="2", stream_resident=resident, carry_combine=carry) as eng:
                st = eng.stats()
                assert st["value_bits"] == 24 and st["col_slices"] == 2 and st["stream_resident"] == int(resident)
                if which == "planted":
                    assert int(eng.read_tiles()["blocks"]["outlier_count"].sum()) == 8
                eng.load_vector(c.xw)
                eng.run_batch(3)
                assert np.array_equal(eng.read_result(), c.want), (resident, carry, "run_batch")
                # another x first, so that y holds something else than c.want when the partition walk begins
                assert not np.array_equal(run_once(eng, other_x), c.want)
                eng.load_vector(c.xw)
                assert c.cp.num_row_partitions == 4
                for part in reversed(range(c.cp.num_row_partitions)):
                    eng.run_partition(part, c.cp.part_len(part))
                assert np.array_equal(eng.read_result(), c.want), (resident, carry, "run_partition")
                eng.iterate(3, scale, shift)
                assert np.array_equal(eng.read_result(), ys[2]), (resident, carry, "iterate")
