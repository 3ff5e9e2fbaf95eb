"""The row-major feature products (include/hisparse_wide.h) on the device: the cases of tests/wide_cases.py against the HIP library, what
hsw_info reports, the stride loop over more than two trips of the grid, a row and a column of 20 000 entries among short and empty ones,
the attention step forward and backward on one caller-owned stream with the row softmax (zero contexts, one synchronisation), and the
sampled product against hisparse_pattern.h's on the transposed operands.  The same cases on libhisparse_cpu.so: tests/test_wide_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from hisparse_amd import device, pattern, rows, wide

import rows_cases as rc
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return wc.HipMemory()


@pytest.mark.parametrize("d", wc.DS)
def test_general(mem, d):
    """300 x 517, 4000 entries, pad 0 and 8, the three calls through the host form and the device form"""
    wc.general(mem, (d,))


def device_bytes(num_rows, num_cols, nnz, transposed):
    """the header's formula"""
    held = 4 * (num_rows + 1) + 4 * max(nnz, 1) + 4 * num_rows
    return held + (4 * (num_cols + 1) + 8 * max(nnz, 1) + 4 * num_cols if transposed else 0)


def test_what_info_reports():
    indptr, indices = wc.random_pattern(wc.ROWS, wc.COLS, wc.NNZ, 1)
    for ip, ix, shape in ((indptr, indices, (wc.ROWS, wc.COLS)), (np.zeros(6, dtype=np.uint32), np.zeros(0, dtype=np.uint32), (5, 7))):
        held = {}
        for flag in (False, True):
            with wide.WideProducts((ip, ix, shape), transposed=flag) as wp:
                held[flag] = wp.info()["device_bytes"]
                assert wp.info() == {"nnz": ix.size, "device_bytes": device_bytes(shape[0], shape[1], ix.size, flag)}
        assert held[True] - held[False] >= 8 * ix.size + 4 * (shape[1] + 1)


def test_edges(mem):
    wc.edges(mem)


def test_non_finite_values(mem):
    wc.non_finite(mem)


def test_adjoint_identities(mem):
    wc.adjoint(mem)


def test_a_call_leaves_nothing_for_the_next(mem):
    wc.nothing_carried_over(mem)


def test_refusals(mem):
    wc.refusals(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def _three_calls(mem, shape, indptr, indices, d, seed, what):
    """the three _device calls over one pattern, every word inside its bound (float64 sums as the reference: the large cases)"""
    with wide.WideProducts((indptr, indices, shape)) as wp:
        for k, op in enumerate(wc.OPS):
            a, b = wc.operands(op, shape, indices.size, d, seed + k)
            wc.Reference(op, shape, indptr, indices, a, b, exact=False).check(wc.device_form(mem, wp, op, a, b, 4, what), f"{what}, {op}")


def test_stride_loop_over_the_shortest_class(mem):
    """300 000 rows of 1 ... 4 entries, 1000 columns, d = 4: the rows are all of the class of four-lane teams, more than two trips of the grid"""
    n_rows, n_cols, d = 300000, 1000, 4
    assert wide.team_lanes(1, d) == 4 and 2 * wide.rows_per_trip(_compute_units(), 1, d) < n_rows
    rng = np.random.default_rng(71)
    lengths = rng.integers(1, 5, n_rows)
    indptr = rc.indptr_of(lengths)
    indices = rng.integers(0, n_cols, int(indptr[-1])).astype(np.uint32)
    _three_calls(mem, (n_rows, n_cols), indptr, indices, d, 720, "300 000 short rows")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", [4, 64])
def test_one_row_of_20000_entries_among_short_and_empty_rows(mem, d, transposed):
    """2001 rows x 25 000 columns: one row of 20 000 entries, 199 of 1 ... 39, the others (the first and the last among them) empty; and
    the transposed pattern, whose long line is a column"""
    rng = np.random.default_rng(73)
    n_rows, n_cols = 2001, 25000
    lengths = np.zeros(n_rows, dtype=np.int64)
    live = rng.choice(np.arange(1, n_rows - 1), 200, replace=False)
    lengths[live] = rng.integers(1, 40, live.size)
    lengths[live[0]] = 20000
    assert lengths[0] == lengths[-1] == 0 and lengths.max() == 20000 and (lengths > wide.WIDE_LONG).sum() == 1
    indptr = rc.indptr_of(lengths)
    indices = rng.integers(0, n_cols, int(indptr[-1])).astype(np.uint32)
    shape = (n_rows, n_cols)
    if transposed:
        r_, c_, indptr, indices = wc.as_csr_of_the_transpose(n_rows, n_cols, indptr, indices)
        shape = (r_, c_)
    _three_calls(mem, shape, indptr, indices, d, 740 + d, f"one long {'column' if transposed else 'row'}, d {d}")


def _matrix(rows_, cols, nnz, seed):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(rows_ * cols, nnz, replace=False))
    m = sp.csr_matrix((np.ones(nnz, dtype=np.float32), (flat // cols, flat % cols)), shape=(rows_, cols))
    m.sort_indices()
    return m


def test_attention_step_on_one_stream(mem):
    """2000 x 3000, 40 000 entries, d = 20 with ld = 24, one caller-owned stream for the pattern and the rows, no host synchronisation
    until the end.  Forward: sddmm(Q, K) -> softmax (out of place) -> spmm(P, V).  Backward: spmm_t(P, gY), sddmm(gY, V),
    softmax_backward, spmm(gS, K), spmm_t(gS, Q).  After the one synchronisation every stage is checked against ITS OWN inputs as read
    back, by that stage's bound."""
    n_rows, n_cols, d, ld, scale = 2000, 3000, 20, 24, 0.5
    m = _matrix(n_rows, n_cols, 40000, 91)
    indptr, indices, shape = m.indptr.astype(np.uint32), m.indices.astype(np.uint32), (n_rows, n_cols)
    rng = np.random.default_rng(92)
    host = {"Q": rng.normal(size=(n_rows, d)), "K": rng.normal(size=(n_cols, d)), "V": rng.normal(size=(n_cols, d)), "gY": rng.normal(size=(n_rows, d))}
    host = {k: v.astype(np.float32) for k, v in host.items()}
    feat = {k: wc._features_in(mem, v, ld - wc.round_up4(d))[0] for k, v in host.items()}
    for name, n in (("Y", n_rows), ("gQ", n_rows), ("gV", n_cols), ("gK", n_cols)):
        feat[name] = mem.alloc(np.full((n, ld), wc.SENTINEL, dtype=np.uint32))
    ent = {name: mem.alloc(np.full(m.nnz, wc.SENTINEL, dtype=np.uint32)) for name in ("S", "P", "gP", "gS")}
    st = mem.stream()
    with wide.WideProducts(m) as wp, rows.RowSoftmax(m) as rs:
        assert wp.nnz == rs.nnz == m.nnz
        wp.set_stream(st.value)
        rs.set_stream(st.value)
        wp.sddmm_device(feat["Q"].ptr, ld, feat["K"].ptr, ld, d, ent["S"].ptr)
        rs.softmax_device(ent["S"].ptr, scale, ent["P"].ptr)
        wp.spmm_device(ent["P"].ptr, feat["V"].ptr, ld, d, feat["Y"].ptr, ld)
        wp.spmm_t_device(ent["P"].ptr, feat["gY"].ptr, ld, d, feat["gV"].ptr, ld)
        wp.sddmm_device(feat["gY"].ptr, ld, feat["V"].ptr, ld, d, ent["gP"].ptr)
        rs.softmax_backward_device(ent["P"].ptr, ent["gP"].ptr, scale, ent["gS"].ptr)
        wp.spmm_device(ent["gS"].ptr, feat["K"].ptr, ld, d, feat["gQ"].ptr, ld)
        wp.spmm_t_device(ent["gS"].ptr, feat["Q"].ptr, ld, d, feat["gK"].ptr, ld)
        assert mem.rt.hipStreamSynchronize(st) == 0
        got = {k: mem.fetch(b).view(np.float32) for k, b in ent.items()}
        for name, n in (("Y", n_rows), ("gQ", n_rows), ("gV", n_cols), ("gK", n_cols)):
            words = mem.fetch(feat[name]).reshape(n, ld)
            assert (words[:, d:] == wc.SENTINEL).all(), f"{name}: pad words written"
            got[name] = np.ascontiguousarray(words[:, :d]).view(np.float32)
        wp.set_stream(None)
        rs.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    assert all(np.isfinite(v).all() for v in got.values())

    def stage(op, a, b, name):
        wc.Reference(op, shape, indptr, indices, a, b).check(got[name], f"attention step, {name}")

    stage("sddmm", host["Q"], host["K"], "S")
    rc.forward_check(m.indptr, got["S"], scale, got["P"], "attention step, P")
    stage("spmm", got["P"], host["V"], "Y")
    stage("spmm_t", got["P"], host["gY"], "gV")
    stage("sddmm", host["gY"], host["V"], "gP")
    rc.backward_check(m.indptr, got["P"], got["gP"], scale, got["gS"], "attention step, gS")
    stage("spmm", got["gS"], host["K"], "gQ")
    stage("spmm_t", got["gS"], host["Q"], "gK")
    assert np.count_nonzero(got["gS"]) > 0.9 * m.nnz and (got["P"] > 0).all()


def test_sampled_product_agrees_with_the_pattern_object():
    """hsw_sddmm and hsp_sddmm (float, k = d = 16) on the transposed operands: the same products summed in double by both, so the two
    results differ by no more than the sum of their two bounds"""
    indptr, indices = wc.random_pattern(wc.ROWS, wc.COLS, wc.NNZ, 6)
    shape, d = (wc.ROWS, wc.COLS), 16
    U, V = wc.operands("sddmm", shape, wc.NNZ, d, 800)
    with wide.WideProducts((indptr, indices, shape), transposed=False) as wp, pattern.SampledProduct(1, (indptr, indices, shape), d) as sp:
        ours = wp.sddmm(U, V)
        theirs = sp.sddmm(np.ascontiguousarray(U.T), np.ascontiguousarray(V.T)).view(np.float32)
    ref = wc.Reference("sddmm", shape, indptr, indices, U, V)
    ref.check(ours, "hsw_sddmm")
    ref.check(theirs, "hsp_sddmm")
    assert (np.abs(ours.astype(np.float64) - theirs.astype(np.float64)) <= 2.0 * ref.bound.ravel()).all()
