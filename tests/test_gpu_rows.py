"""The row softmax (include/hisparse_rows.h) on the device: the cases of tests/rows_cases.py against the HIP library, what hsr_info
reports, the stride loop over more than two trips of the smallest class, a row of 300 000 entries among short and empty rows, a second
call on one object, and the attention step on one caller-owned stream: hsp_sddmm_device -> hsr_softmax_device in place ->
hs_update_values_device -> hs_run (forward and transposed context).  The same cases on libhisparse_cpu.so: tests/test_rows_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from hisparse_amd import device, host, pattern, rows

import pattern_cases as pc
import rows_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return rc.HipMemory()


def test_general_and_what_info_reports(mem):
    indptr = rc.general(mem)
    live = int((np.diff(indptr.astype(np.int64)) > 0).sum())
    with rows.RowSoftmax(indptr) as rs:
        assert rs.info() == {"nnz": int(indptr[-1]), "device_bytes": 4 * indptr.size + 4 * live + 64}      # indptr, the non-empty rows, the table
    with rows.RowSoftmax(np.zeros(6, dtype=np.uint32)) as rs:
        assert rs.info() == {"nnz": 0, "device_bytes": 4 * 6 + 4 * 1 + 64}


def test_exact_answers(mem):
    rc.exact_answers(mem)


def test_non_finite_scores(mem):
    rc.non_finite(mem)


def test_edges(mem):
    rc.edges(mem)


def test_refusals(mem):
    rc.refusals(mem)


def _matrix(rows_, cols, nnz, seed):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(rows_ * cols, nnz, replace=False))
    m = sp.csr_matrix((rng.normal(size=nnz).astype(np.float32), (flat // cols, flat % cols)), shape=(rows_, cols))
    m.sort_indices()
    return m


def _csr(m, values):
    return (m.shape[0], m.shape[1], m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ascontiguousarray(values, dtype=np.float32))


def test_stride_loop_over_the_smallest_class(mem):
    """300 000 rows of 1 ... 4 entries: all of the G = 4 class, more than two trips of the grid; every word inside its bound"""
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr(_csr(_matrix(128, 64, 200, 1), np.ones(200, dtype=np.float32)))
        cus = eng.stats()["num_compute_units"]
    n_rows = 300000
    assert 2 * rows.rows_per_trip(cus, 4) < n_rows
    lengths = np.random.default_rng(71).integers(1, 5, n_rows)
    p, _ = rc.checked_on_device(mem, rc.indptr_of(lengths), 0.7, 6.0, 72, "300 000 short rows")
    assert (p > 0).all() and (p[np.repeat(lengths, lengths) == 1] == 1.0).all()


def test_one_row_of_300000_entries_among_short_and_empty_rows(mem):
    rng = np.random.default_rng(73)
    n_rows = 20001
    lengths = np.zeros(n_rows, dtype=np.int64)
    live = rng.choice(n_rows, n_rows // 10, replace=False)
    lengths[live] = rng.integers(1, 40, live.size)
    lengths[live[0]] = 300000
    lengths[0] = lengths[-1] = 0
    assert (lengths == 0).mean() >= 0.9 and lengths.max() == 300000 and (lengths > 256).sum() == 1
    indptr = rc.indptr_of(lengths)
    p, _ = rc.checked_on_device(mem, indptr, 1.0, 4.0, 74, "one row of 300 000 entries")
    lo = int(indptr[live[0]])
    assert abs(float(p[lo: lo + 300000].astype(np.float64).sum()) - 1.0) < 1e-5


def test_a_call_leaves_nothing_for_the_next(mem):
    """other scores on the same object: the words of a fresh object"""
    indptr = rc.indptr_of(rc.general_lengths())
    with rows.RowSoftmax(indptr) as rs, rows.RowSoftmax(indptr) as fresh:
        first, second = rc.scores(rs.nnz, 30.0, 81), rc.scores(rs.nnz, 4.0, 82)
        rc.forward_check(indptr, first, 1.0, rc.device_forward(mem, rs, first, 1.0)[0], "first call")
        p = rc.device_forward(mem, rs, second, -2.5)[0]
        want = rc.device_forward(mem, fresh, second, -2.5)[0]
        assert np.array_equal(rc.words(p), rc.words(want))
        gp = rc.grads(rs.nnz, 83)
        assert np.array_equal(rc.words(rc.device_backward(mem, rs, p, gp, -2.5)), rc.words(rc.device_backward(mem, fresh, p, gp, -2.5)))


@pytest.mark.parametrize("transpose", [False, True])
def test_attention_step_on_one_stream(mem, transpose):
    """Float mode, one caller-owned stream for the three objects, no host synchronisation in between: SDDMM (k = 4) into a device buffer,
    the softmax in place, hs_update_values_device with that buffer, hs_run.  y is, bit for bit, the y of a fresh load with the
    probabilities READ BACK from the buffer, and those are inside the forward bound against the scores as they were before the softmax
    (copied aside on the same stream)."""
    impl, k, scale = 1, 4, 0.5
    m = _matrix(2000, 3000, 40000, 91)
    rt = mem.rt
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    st = mem.stream()
    U, V = pc.vectors(impl, k, 2000, 92), pc.vectors(impl, k, 3000, 93)
    du, dv, out, aside = mem.alloc(U), mem.alloc(V), mem.alloc(np.zeros(m.nnz, dtype=np.uint32)), mem.alloc(np.zeros(m.nnz, dtype=np.uint32))
    with device.SpmvEngine(impl) as eng, pattern.SampledProduct(impl, m, k) as sp, rows.RowSoftmax(m) as rs:
        assert rs.nnz == m.nnz
        eng.set_option("value_map", "1")
        eng.load_matrix_csr(_csr(m, m.data), transpose=transpose)
        x = host.pack_vector(impl, np.random.default_rng(94).normal(size=eng.num_cols).astype(np.float32))
        eng.load_vector(x)
        eng.set_stream(st.value)
        sp.set_stream(st.value)
        rs.set_stream(st.value)
        sp.sddmm_device(du.ptr, 2000, dv.ptr, 3000, k, out.ptr)
        assert rt.hipMemcpyAsync(C.c_void_p(aside.ptr), C.c_void_p(out.ptr), m.nnz * 4, 3, st) == 0      # device to device
        rs.softmax_device(out.ptr, scale, out.ptr)
        eng.update_values_device(out.ptr, m.nnz)
        eng.run()
        y = eng.read_result()
        assert rt.hipStreamSynchronize(st) == 0
        probs, scores = mem.fetch(out).view(np.float32), mem.fetch(aside).view(np.float32)
        eng.set_stream(None)
        sp.set_stream(None)
        rs.set_stream(None)
    rt.hipStreamDestroy(st)
    assert np.isfinite(scores).all() and np.count_nonzero(scores) > 0.99 * m.nnz
    rc.forward_check(m.indptr, scores, scale, probs, "the buffer")
    assert (probs > 0).all() and (probs <= 1).all()
    with device.SpmvEngine(impl) as fresh:
        fresh.load_matrix_csr(_csr(m, probs), transpose=transpose)
        fresh.load_vector(x)
        fresh.run()
        want = fresh.read_result()
    assert want.any() and np.array_equal(y, want)
