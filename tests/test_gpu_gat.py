"""The graph attention (GAT) calls (include/hisparse_gat.h) on the device: the cases of tests/gat_cases.py against the HIP library, the
stride loops of the three kernels over more than two trips of the grid at the widest group, long rows and long columns among short and
empty ones (the per-lane merge of a workgroup's four wavefronts through LDS), a training step on one caller-owned stream (three
launches, one synchronisation) and hsmh_info unchanged by the new calls.  The same cases on libhisparse_cpu.so: tests/test_gat_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import gat, heads, wide

import gat_cases as gc
import test_gpu_heads as th
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return gc.HipMemory()


@pytest.mark.parametrize("shape", gc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general(mem, shape):
    """300 x 517, 4000 entries, slope 0.2, 0 and 1, pad 0 and 8, head-array ld = heads and heads + 3, lse taken and NULL, both forms, forward
    then backward with the lse just written"""
    gc.general(mem, (shape,))


def test_ties(mem):
    gc.ties(mem)


def test_heads_do_not_leak(mem):
    gc.heads_do_not_leak(mem)


def test_edges(mem):
    gc.edges(mem)


def test_a_call_leaves_nothing_for_the_next(mem):
    """hsgat, then hsmh_backward_device over the same D words, then hsgat again"""
    gc.nothing_carried_over(mem)


def test_refusals(mem):
    gc.refusals(mem)


def test_info_is_unchanged_by_the_new_calls(mem):
    indptr, indices = gc.random_pattern(gc.ROWS, gc.COLS, gc.NNZ, 1)
    shape = (gc.ROWS, gc.COLS)
    with gat.GraphAttention((indptr, indices, shape), 5) as ga, heads.MultiHeadAttention((indptr, indices, shape), 5) as mh:
        before = ga.info()
        assert before == mh.info() and before["nnz"] == gc.NNZ
        EL, ER, V, gY = gc.operands(shape, indptr, indices, 5, 4, 13000)
        y, lse = gc.forward_device(mem, ga, EL, ER, V, 5, 0.2)
        gc.backward_device(mem, ga, EL, ER, V, gY, lse, 5, 0.2)
        gc.backward_host(ga, EL, ER, V, gY, lse, 5, 0.2)
        assert ga.info() == before


def test_stride_loop_of_the_row_side_at_the_widest_group(mem):
    """rows of 1 ... 4 entries over 1000 columns at 4 heads of d = 64: one group of 64 lanes per row, four rows per workgroup, and more than
    two trips of the grid in the forward kernel and in the backward's row kernel"""
    shape, indptr, indices = th._short_rows(1000, 256)
    gc.large(mem, shape, indptr, indices, 4, 64, 13110, f"{shape[0]} short rows, 4 heads of d 64")


def test_stride_loop_of_the_column_side_at_the_widest_group(mem):
    """the mirror image: that many columns of 1 ... 4 entries over 1000 rows, more than two trips of the grid in the column kernel"""
    shape, indptr, indices = th._transposed(*th._short_rows(1000, 256))
    lengths = np.bincount(indices, minlength=shape[1])
    assert shape[0] == 1000 and lengths.min() >= 1 and lengths.max() <= 4
    gc.large(mem, shape, indptr, indices, 4, 64, 13120, f"{shape[1]} short columns, 4 heads of d 64")


@pytest.mark.parametrize("heads_,d", [(5, 4), (4, 16)])
def test_long_rows_among_short_and_empty_rows(mem, heads_, d):
    shape, indptr, indices = th._long_rows()
    fwd, bwd = gc.large(mem, shape, indptr, indices, heads_, d, 13210 + d, f"long rows among short and empty ones, {heads_} heads of d {d}")
    assert fwd[0].empty.sum() == shape[0] - 202 and sorted(bwd[0].n[bwd[0].n > wide.WIDE_LONG]) == [513, 1025, 3000]


@pytest.mark.parametrize("heads_,d", [(5, 4), (4, 16)])
def test_long_columns_among_short_and_empty_columns(mem, heads_, d):
    """the transpose-shaped twin, 4096 x 2001: columns of 513, 1025 and 3000 entries among short and empty ones"""
    shape, indptr, indices = th._transposed(*th._long_rows())
    fwd, bwd = gc.large(mem, shape, indptr, indices, heads_, d, 13220 + d, f"long columns among short and empty ones, {heads_} heads of d {d}")
    assert shape == (4096, 2001) and bwd[0].empty_c.sum() == shape[1] - 202 and sorted(bwd[0].m[bwd[0].m > wide.WIDE_LONG]) == [513, 1025, 3000]


def _words(mem, buf, w, ld):
    words = mem.fetch(buf).reshape(-1, ld)
    assert (words[:, w:] == gc.SENTINEL).all()
    return np.ascontiguousarray(words[:, :w]).view(np.float32)


def test_training_step_on_one_stream(mem):
    """hsgat_forward_device then hsgat_backward_device on a caller-owned stream, one synchronisation at the end: three launches.  Y and lse
    are inside the forward's bounds, gel, ger and gV inside the bounds computed from the lse words the device wrote.  2000 x 3000, 40 000
    entries, 3 heads of d = 8 with feature ld = 28 and head-array ld = 4."""
    import scipy.sparse as sp
    n_rows, n_cols, H, d, ld, ldh, slope = 2000, 3000, 3, 8, 28, 4, 0.2
    w = H * d
    rng = np.random.default_rng(13300)
    flat = np.sort(rng.choice(n_rows * n_cols, 40000, replace=False))
    m = sp.csr_matrix((np.ones(flat.size, dtype=np.float32), (flat // n_cols, flat % n_cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    indptr, indices = m.indptr.astype(np.uint32), m.indices.astype(np.uint32)
    EL, ER, V, gY = gc.operands(m.shape, indptr, indices, H, d, 13310)
    da, db = (gc._heads_in(mem, a, ldh - H)[0] for a in (EL, ER))
    dv, dg = (wc._features_in(mem, a, ld - w)[0] for a in (V, gY))
    dy, ov = (mem.alloc(np.full((n, ld), gc.SENTINEL, dtype=np.uint32)) for n in (n_rows, n_cols))
    dl, oa, ob = (mem.alloc(np.full((n, ldh), gc.SENTINEL, dtype=np.uint32)) for n in (n_rows, n_rows, n_cols))
    st = mem.stream()
    with gat.GraphAttention(m, H) as ga:
        ga.set_stream(st.value)
        ga.forward_device(da.ptr, ldh, db.ptr, ldh, dv.ptr, ld, H, d, slope, dy.ptr, ld, dl.ptr, ldh)
        ga.backward_device(da.ptr, ldh, db.ptr, ldh, dv.ptr, ld, dg.ptr, ld, dl.ptr, ldh, H, d, slope, oa.ptr, ldh, ob.ptr, ldh, ov.ptr, ld)
        assert mem.rt.hipStreamSynchronize(st) == 0
        y, gv = (_words(mem, b, w, ld) for b in (dy, ov))
        lse, gel, ger = (_words(mem, b, H, ldh) for b in (dl, oa, ob))
        ga.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    fwd = gc.forward_refs(indptr, indices, EL, ER, V, slope, exact=False)
    gc.check_forward(fwd, y, lse, "training step, forward")
    assert np.isfinite(lse[np.diff(indptr.astype(np.int64)) > 0]).all()
    gc.check_backward(gc.backward_refs(fwd, gY, lse), gel, ger, gv, "training step, backward")
