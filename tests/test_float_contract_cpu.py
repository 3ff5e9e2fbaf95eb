"""The float contract helper (tests/float_contract.py) on the CPU: the numpy walk over the device image (tile_emulator.run, double sums)
keeps the D bound in every stream format, with and without column slices, and the bound rejects what the kernels must not do -- csim's
fp32 running sum, a dropped product, fp32 accumulation."""
import numpy as np
import pytest

from hisparse_amd import device, host
from oracle import oracle as orc

import cases
import float_contract as fc
import tile_emulator

FORMATS = ["pairs", "pairs24", "delta", "bitmap", "owner", "owner24", "sweep"]


def _setup(impl, rows=400, cols=20000, seed=3):
    m, x, kinds = fc.designed(rows, cols, seed)
    v, o = host.default_banks(impl)
    _, cp = cases.formatted(m, impl, v, o, True)
    xp = np.zeros(cp.num_cols, dtype=np.float32)
    xp[:cols] = x
    return m, cp, xp, host.pack_vector(impl, xp), kinds


def _tiles(cp, impl, fmt, monkeypatch, slices):
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", fmt[:5] if fmt == "pairs24" else fmt)
    monkeypatch.setenv("HISPARSE_AUX_BITS", "24" if fmt == "pairs24" else "32")
    monkeypatch.setenv("HISPARSE_COL_SLICES", str(slices))
    t = device.build_tiles(cp, impl, cp.ob_bank, cp.vb_bank, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, 256)
    assert t["format"] == fmt, t["format"]
    return t


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("slices", [1, 3])
def test_emulator_keeps_the_double_sum_bound(impl, fmt, slices, monkeypatch):
    m, cp, xp, xw, _ = _setup(impl)
    if fmt == "bitmap" and slices > 1:
        slices = 1                                           # (a forced bitmap plan is unsliced: test_tiles_cpu.test_column_slices)
    t = _tiles(cp, impl, fmt, monkeypatch, slices)
    y = tile_emulator.run(t, impl, xw, cp.num_rows)
    ref = fc.Reference(m, xp, cp.num_rows)
    ref.check(y, L=1, slices=int(t["col_slices"]), what=f"emulator {fmt}")
    assert (y[m.shape[0]:] == 0).all()                       # padded rows: exactly +0.0


@pytest.mark.parametrize("impl", [1, 2])
def test_csim_fp32_running_sum_breaks_the_bound(impl):
    # the oracle (csim's float PE: fp32 running sum in column order) on the long and the cancellation rows
    m, cp, xp, xw, kinds = _setup(impl)
    want = orc.spmv(impl, [cp.channel(c) for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                    cp.ob_bank, cp.vb_bank)
    ref = fc.Reference(m, xp, cp.num_rows)
    bad = ref.violations(want, L=1)
    assert bad[kinds["cancel"]].mean() >= 0.9 and bad[kinds["long"]].mean() >= 0.3, (bad[kinds["cancel"]].mean(), bad[kinds["long"]].mean())
    assert not ref.violations(want, L=np.maximum(ref.n, 1))[: m.shape[0]].any()     # ... and keeps the bound of its own chain length
    with pytest.raises(AssertionError):
        ref.check(want, L=1, what="csim")


def _drop_one(ys, is_float, row, val, xv):
    # one product lost per accumulate call (a chunk / unit step / bitmap row)
    if row.size > 1:
        row, val, xv = row[1:], val[1:], xv[1:]
    _real(ys, is_float, row, val, xv)


def _fp32_sums(ys, is_float, row, val, xv):
    # accumulate in fp32 instead of double
    p = (val.view(np.float32) * xv.view(np.float32)).astype(np.float32)
    for r, v in zip(row, p):
        ys[r] = np.float32(np.float32(ys[r]) + v)


_real = tile_emulator._accumulate


@pytest.mark.parametrize("mutant", [_drop_one, _fp32_sums])
@pytest.mark.parametrize("fmt", ["pairs", "delta", "owner24", "sweep"])
def test_mutated_emulator_breaks_the_bound(mutant, fmt, monkeypatch):
    impl = 1
    m, cp, xp, xw, kinds = _setup(impl)
    t = _tiles(cp, impl, fmt, monkeypatch, 1)
    ref = fc.Reference(m, xp, cp.num_rows)
    assert (ref.min_abs[kinds["long"]] > ref.bound(1)[kinds["long"]]).mean() >= 0.9     # a lost product moves y beyond the bound
    monkeypatch.setattr(tile_emulator, "_accumulate", mutant)
    y = tile_emulator.run(t, impl, xw, cp.num_rows)
    bad = ref.violations(y, L=1)
    assert bad.any()
    if mutant is _fp32_sums:
        assert bad[kinds["cancel"]].mean() >= 0.5


def test_non_finite_expectations():
    import scipy.sparse as sp
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([1.0, inf, -inf, nan, 2.0, 0.0], dtype=np.float32)
    dense = np.zeros((7, 6), dtype=np.float32)
    dense[0, [0, 1]] = 1.0                     # +inf
    dense[1, [1, 2]] = 1.0                     # inf - inf = NaN
    dense[2, [0, 3]] = 1.0                     # NaN
    dense[3, [0, 4]] = 1.0                     # finite 3
    dense[4, 2] = 2.0                          # -inf
    m = sp.csr_matrix(dense)
    m = sp.csr_matrix((np.append(m.data, 0.0).astype(np.float32), np.append(m.indices, 1), np.append(m.indptr, m.indptr[-1] + 1)), shape=(8, 6))
    ref = fc.Reference(m, x)                   # row 7: an explicit stored zero under the inf column: 0 x inf = NaN
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)
    good = f(inf, nan, nan, 3.0, -inf, 0.0, 0.0, nan)
    assert not ref.violations(good).any()
    for r, wrong in [(0, nan), (1, inf), (2, 0.0), (3, inf), (4, inf), (5, -0.0 + 1e-30), (7, 0.0)]:
        y = good.copy()
        y[r] = f(wrong)[0]
        assert ref.violations(y)[r], r
    # overflow: a fp32 running sum passes the range, the exact sum does not
    big = np.float32(2.0 ** 127 * 1.5)
    m2 = sp.csr_matrix(np.array([[big, big, -big]], dtype=np.float32))
    ref2 = fc.Reference(m2, np.ones(3, dtype=np.float32))
    assert not ref2.violations(f(big)).any() and ref2.violations(f(inf)).all()
