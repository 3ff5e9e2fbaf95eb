"""The bf16 calls of the multi-head attention object (include/hisparse_heads_bf16.h) on the device: the cases of tests/heads16_cases.py
against the HIP library, the stride loops of the three kernels over more than two trips of the grid at the widest group, long rows and
long columns among short and empty ones (the per-lane merge of a workgroup's four wavefronts through LDS, with dead lanes and with the
weight dealing on), and a training step on one caller-owned stream (three launches, one synchronisation).  The same cases on
libhisparse_cpu.so: tests/test_heads16_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import device, heads16, wide

import heads16_cases as c16
import rows_cases as rc
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return c16.HipMemory()


@pytest.mark.parametrize("shape", c16.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general(mem, shape):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, pad 0 and 8 elements, ldl = heads and heads + 3, lse taken and NULL, both forms,
    forward then backward with the lse just written"""
    c16.general(mem, (shape,))


def test_heads_do_not_leak(mem):
    c16.heads_do_not_leak(mem)


def test_edges(mem):
    c16.edges(mem)


def test_a_call_leaves_nothing_for_the_next_whichever_precision(mem):
    c16.nothing_carried_over(mem)


def test_forward_in_one_precision_backward_in_the_other(mem):
    c16.mixed(mem)


def test_refusals(mem):
    c16.refusals(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def _transposed(shape, indptr, indices):
    """the CSR arrays of the transposed pattern"""
    rows_, cols_ = shape
    cptr, trow, _ = wc.transposed_pattern(rows_, cols_, indptr, indices)
    return (cols_, rows_), np.asarray(cptr, dtype=np.uint32), np.asarray(trow, dtype=np.uint32)


def _short_rows(n_cols, width):
    """rows of 1 ... 4 entries over n_cols columns: more than two trips of the grid at class 1 (20 000 rows, or as many as the device's CU
    count asks for by the same formula); `width` is the row's size in 4-byte words, which sets the schedule"""
    assert wide.team_lanes(1, width) == 64
    n_rows = max(20000, 2 * wide.rows_per_trip(_compute_units(), 1, width) + 1000)
    assert 2 * wide.rows_per_trip(_compute_units(), 1, width) < n_rows
    rng = np.random.default_rng(9100)
    indptr = rc.indptr_of(rng.integers(1, 5, n_rows))
    return (n_rows, n_cols), indptr, rng.integers(0, n_cols, int(indptr[-1])).astype(np.uint32)


def test_stride_loop_of_the_row_side_at_the_widest_group(mem):
    """rows of 1 ... 4 entries over 1000 columns at 4 heads of d = 128 (1 KiB a row, 256 words): one group of 64 lanes per row, four rows per
    workgroup, and more than two trips of the grid in the forward kernel and in the backward's row kernel"""
    shape, indptr, indices = _short_rows(1000, 256)
    c16.large(mem, shape, indptr, indices, 4, 128, 9110, f"{shape[0]} short rows, 4 heads of d 128")


def test_stride_loop_of_the_column_side_at_the_widest_group(mem):
    """the mirror image: that many columns of 1 ... 4 entries over 1000 rows, more than two trips of the grid in the column kernel"""
    shape, indptr, indices = _transposed(*_short_rows(1000, 256))
    lengths = np.bincount(indices, minlength=shape[1])
    assert shape[0] == 1000 and lengths.min() >= 1 and lengths.max() <= 4
    c16.large(mem, shape, indptr, indices, 4, 128, 9120, f"{shape[1]} short columns, 4 heads of d 128")


def _long_rows():
    """2001 rows x 4096 columns: rows of 513, 1025 and 3000 entries, 199 of 1 ... 39, the others (the first and the last among them) empty
    (the pattern of tests/test_gpu_heads.py)"""
    rng = np.random.default_rng(5200)
    n_rows, n_cols = 2001, 4096
    lengths = np.zeros(n_rows, dtype=np.int64)
    live = rng.choice(np.arange(1, n_rows - 1), 202, replace=False)
    lengths[live] = rng.integers(1, 40, live.size)
    lengths[live[:3]] = (513, 1025, 3000)
    assert lengths[0] == lengths[-1] == 0 and (lengths > wide.WIDE_LONG).sum() == 3 and (lengths > 0).sum() == 202
    indptr = rc.indptr_of(lengths)
    indices = np.concatenate([rng.choice(n_cols, int(n), replace=False) for n in lengths if n]).astype(np.uint32)
    return (n_rows, n_cols), indptr, indices


@pytest.mark.parametrize("heads_,d", [(5, 8), (4, 32)])
def test_long_rows_among_short_and_empty_rows(mem, heads_, d):
    shape, indptr, indices = _long_rows()
    fwd, bwd = c16.large(mem, shape, indptr, indices, heads_, d, 9210 + d, f"long rows among short and empty ones, {heads_} heads of d {d}")
    assert fwd[0].empty.sum() == shape[0] - 202 and sorted(bwd[0].n[bwd[0].n > wide.WIDE_LONG]) == [513, 1025, 3000]


@pytest.mark.parametrize("heads_,d", [(5, 8), (4, 32)])
def test_long_columns_among_short_and_empty_columns(mem, heads_, d):
    """the transpose-shaped twin, 4096 x 2001: columns of 513, 1025 and 3000 entries among short and empty ones"""
    shape, indptr, indices = _transposed(*_long_rows())
    fwd, bwd = c16.large(mem, shape, indptr, indices, heads_, d, 9220 + d, f"long columns among short and empty ones, {heads_} heads of d {d}")
    assert shape == (4096, 2001) and bwd[0].empty_c.sum() == shape[1] - 202 and sorted(bwd[0].m[bwd[0].m > wide.WIDE_LONG]) == [513, 1025, 3000]


def _features(mem, buf, w, ld):
    elements = mem.fetch(buf).view(np.uint16).reshape(-1, ld)
    assert (elements[:, w:] == c16.SENTINEL16).all(), "an output pad was written"
    return heads16.from_bf16(elements[:, :w])


def test_training_step_on_one_stream(mem):
    """hsmh16_forward_device then hsmh16_backward_device on a caller-owned stream, one synchronisation at the end: three launches.  Y and
    lse are inside the forward's bounds, gQ, gK and gV inside the bounds computed from the lse words the device wrote, the output pads
    intact.  2000 x 3000, 40 000 entries, 3 heads of d = 16 with ld = 56 elements and ldl = 4."""
    import scipy.sparse as sp
    n_rows, n_cols, H, d, ld, ldl, scale = 2000, 3000, 3, 16, 56, 4, 0.5
    w = H * d
    rng = np.random.default_rng(9300)
    flat = np.sort(rng.choice(n_rows * n_cols, 40000, replace=False))
    m = sp.csr_matrix((np.ones(flat.size, dtype=np.float32), (flat // n_cols, flat % n_cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    indptr, indices = m.indptr.astype(np.uint32), m.indices.astype(np.uint32)
    Q, K, V, gY = c16.operands(m.shape, w, 9310)
    dq, dk, dv, dg = (c16._features_in(mem, a, ld - w)[0] for a in (Q, K, V, gY))
    dy, oq, ok, ov = (c16._out(mem, n, ld) for n in (n_rows, n_rows, n_cols, n_cols))
    dl = mem.alloc(np.full((n_rows, ldl), c16.hc.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with heads16.MultiHeadAttentionBF16(m, H) as mh:
        mh.set_stream(st.value)
        mh.forward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, H, d, scale, dy.ptr, ld, dl.ptr, ldl)
        mh.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, ldl, H, d, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld)
        assert mem.rt.hipStreamSynchronize(st) == 0
        lw = mem.fetch(dl).reshape(n_rows, ldl)
        y, gq, gk, gv = (_features(mem, b, w, ld) for b in (dy, oq, ok, ov))
        mh.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    assert (lw[:, H:] == c16.hc.SENTINEL).all()
    lse = np.ascontiguousarray(lw[:, :H]).view(np.float32)
    scores = c16.head_scores(indptr, indices, Q, K, H, exact=False)
    c16.check_forward(c16.forward_refs(scores, V, scale), y, lse, "training step, forward")
    assert np.isfinite(lse[np.diff(indptr.astype(np.int64)) > 0]).all()
    c16.check_backward(c16.backward_refs(scores, V, gY, lse, scale), gq, gk, gv, "training step, backward")
