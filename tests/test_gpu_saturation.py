"""Fixed point at the borders of the 32-bit accumulator: the expected words come from Python integers (q8_24_mul: the exact product + 2^23,
shifted right by 24, saturated; a row: min(sum, 2^32 - 1)) and from the oracle.  Rows that end exactly at 0xFFFFFFFE / 0xFFFFFFFF or one
product past it, per-slice partials that stay below 2^32 while their total passes it, a SWEEP row whose crossing product is the last of
its block, per column of the SpMMs, SpMSpV passes."""
import numpy as np
import pytest
import scipy.sparse as sp

from hisparse_amd import device, host
from oracle import oracle as orc

import cases
from test_gpu_float_contract import VARIANTS, _force
from test_gpu_parity import _assert_forced_plan
from test_spmm import _Hip

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF
ROWS, COLS = 700, 40000
Q = 2.0 ** -24


def q8_24_mul(a, b):
    return min((int(a) * int(b) + (1 << 23)) >> 24, TOP)


def _matrix():
    """(CSR, rows of interest): bulk rows of small values on multiples of 2^-20 (exact in Q8.24), then the border rows"""
    rng = np.random.default_rng(9)
    m = sp.random(ROWS, COLS, density=0.002, random_state=np.random.RandomState(9), format="lil", dtype=np.float32)
    special = {
        1: {0: 255.0, 9000: 0xFFFFFE * Q},                       # 0xFFFFFFFE
        2: {0: 255.0, 9000: 0xFFFFFF * Q},                       # 0xFFFFFFFF exactly
        3: {0: 255.0, 9000: 0xFFFFFF * Q, 18000: Q},             # one LSB past
        4: {100: 96.0, 9100: 96.0, 17000: 96.0, 25000: 96.0, 33000: 96.0},   # every slice below 2^32, the total past it
        5: {200: 128.0, 9200: 127.0, 18200: 0xFFFFFF * Q},       # 0xFFFFFFFF from three slices
        6: {500: 200.0},                                         # SpMSpV: past 2^32 only when column 500 comes twice
        7: {**{c: 16.0 for c in range(300, 315)}, COLS - 1: 16.0},     # 15 x 16 = 240, the last column (last of its SWEEP block) crosses
        450: {1: 255.0, 20000: 0xFFFFFF * Q, 39990: 2 * Q},      # a second row block
    }
    for r, row in special.items():
        m[r, :] = 0
        for c, v in row.items():
            m[r, c] = v
    m = m.tocsr()
    bulk = np.isin(np.repeat(np.arange(ROWS), np.diff(m.indptr)), list(special), invert=True)
    m.data[bulk] = np.round(rng.uniform(0.0, 2.0, int(bulk.sum())) * 2 ** 20) / 2 ** 20
    m.eliminate_zeros()
    m.sort_indices()
    return m, sorted(special)


def _expected(m, x_float, num_rows):
    """Python-integer Q8.24 SpMV of the stored elements"""
    aw = np.round(m.data.astype(np.float64) * 2 ** 24).astype(np.int64)
    xw = np.round(np.asarray(x_float, dtype=np.float64) * 2 ** 24).astype(np.int64)
    y = np.zeros(num_rows, dtype=np.uint32)
    for r in range(m.shape[0]):
        s = sum(q8_24_mul(aw[k], xw[m.indices[k]]) for k in range(m.indptr[r], m.indptr[r + 1]))
        y[r] = min(s, TOP)
    return y


def _setup(ob=2):
    m, special = _matrix()
    v, _ = host.default_banks(0)
    _, cp = cases.formatted(m, 0, v, ob, True)
    x = np.ones(cp.num_cols, dtype=np.float32)
    xw = host.pack_vector(0, x)
    want = _expected(m, x, cp.num_rows)
    assert want[1] == 0xFFFFFFFE and want[2] == TOP and want[3] == TOP and want[4] == TOP and want[5] == TOP and want[7] == TOP
    assert want[450] == TOP and want[6] == 200 << 24
    oracle = orc.spmv(0, [cp.channel(c) for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                      cp.ob_bank, cp.vb_bank)
    assert np.array_equal(oracle, want)
    return m, cp, x, xw, want


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("slices", [1, 3])
def test_sums_at_the_accumulator_border(variant, slices, monkeypatch):
    m, cp, x, xw, want = _setup()
    assert cp.num_row_partitions > 1
    _force(monkeypatch, variant, slices)
    hip = _Hip()
    with device.SpmvEngine(0, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
        eng.set_option("carry_combine", "1")
        eng.load_matrix(cp)
        st = eng.stats()
        _assert_forced_plan(st, cp, 0, m.nnz)
        if variant.startswith("pairs") or variant.startswith("delta"):
            assert st["col_slices"] == slices
        eng.load_vector(xw)
        outs = {}
        eng.run()
        outs["run"] = eng.read_result()
        y_dev = eng.device_result()
        poison = np.full(cp.num_rows, 0xdeadbeef, dtype=np.uint32)     # nothing left over from the run before may pass for the carried sum
        assert hip.rt.hipMemcpy(y_dev, poison.ctypes.data, poison.nbytes, 1) == 0
        eng.run()
        eng.run()                                # step 0 is combined by step 1's kernel (carried); step 1's sum is owed
        assert hip.rt.hipDeviceSynchronize() == 0
        outs["carried"] = hip.download(y_dev, (cp.num_rows,))      # read past the library, which would settle the owed sum first
        outs["stand-alone"] = eng.read_result()
        eng.load_matrix(cp)
        eng.load_vector(xw)
        for j in range(cp.num_row_partitions):
            eng.run_partition(j, cp.part_len(j))
        outs["partitions"] = eng.read_result()
    for what, y in outs.items():
        assert np.array_equal(y, want), (variant, st["col_slices"], what, np.nonzero(y != want)[0][:8], y[y != want][:8])


def test_spmm_columns_saturate_on_their_own(monkeypatch):
    # per column: x = 1 (rows 3, 4, 5, 7 saturate), x = 1/2 (row 3: 0x7FFFFFFF + ...: below the border), x = 0
    m, cp, x, xw, _ = _setup()
    X = np.stack([np.ones(cp.num_cols, np.float32), np.full(cp.num_cols, 0.5, np.float32), np.zeros(cp.num_cols, np.float32),
                  np.ones(cp.num_cols, np.float32)])
    wants = [_expected(m, X[j], cp.num_rows) for j in range(4)]
    assert wants[0][4] == TOP and wants[1][4] != TOP
    XW = np.stack([host.pack_vector(0, X[j]) for j in range(4)])
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "sweep")
    for slices in ("1", "3"):
        with device.SpmvEngine(0, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
            eng.set_option("spmm_vectors", "4")
            eng.set_option("col_slices", slices)
            eng.load_matrix(cp)
            assert device.STREAM_FORMATS[eng.stats()["stream_format"]] == "sweep"
            Y = eng.spmm(XW)
        for j in range(4):
            assert np.array_equal(Y[j], wants[j]), ("spmm_vectors=4", slices, j, np.nonzero(Y[j] != wants[j])[0][:8])
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "bitmap")
    monkeypatch.setenv("HISPARSE_COL_SLICES", "1")
    with device.SpmvEngine(0, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
        eng.load_matrix(cp)
        assert device.STREAM_FORMATS[eng.stats()["stream_format"]] == "bitmap"
        Y = eng.spmm(XW)
    for j in range(4):
        assert np.array_equal(Y[j], wants[j]), ("fused bitmap", j, np.nonzero(Y[j] != wants[j])[0][:8])


def test_spmspv_crosses_the_border_in_its_second_pass():
    m, cp, _, _, _ = _setup()
    indptr, ridx, words = host.csr_to_csc(host.CSRMatrix.from_scipy(m), 0)
    xi = np.array([0, 500, 9000, 500, 18000, 300], dtype=np.uint32)      # column 500 twice: row 6 = 200 + 200
    xv = np.ones(xi.size, dtype=np.float32)
    dense = np.zeros(COLS, dtype=np.float64)
    np.add.at(dense, xi, 1.0)
    aw = np.round(m.data.astype(np.float64) * 2 ** 24).astype(np.int64)
    want = np.zeros(ROWS, dtype=np.uint32)
    for r in range(ROWS):
        s = 0
        for k in range(m.indptr[r], m.indptr[r + 1]):
            s += q8_24_mul(aw[k], 1 << 24) * int(dense[m.indices[k]])     # each x entry its own product
        want[r] = min(s, TOP)
    assert want[6] == TOP and want[1] == 0xFFFFFFFE and want[3] == TOP
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csc(indptr, ridx, words, ROWS)
        y = eng.spmspv(xi, host.pack_vector(0, xv))
    assert np.array_equal(y, want), (np.nonzero(y != want)[0][:8], y[y != want][:8])
