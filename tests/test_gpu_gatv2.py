"""The GATv2 calls (include/hisparse_gatv2.h) on the device: the reference of tests/gatv2_cases.py against torch's float64 autograd first,
then its cases against the HIP library, the stride loops of the kernels over more than two trips of the grid at the widest group (a
workgroup's ga sums persist across its rows), long rows and long columns among short and empty ones (the per-lane merge of a workgroup's
four wavefronts through LDS, and ga out of class-0 and short-row workgroups together), a training step on one caller-owned stream (four
launches, one synchronisation) and hsmh_info unchanged by the new calls.  The same cases on libhisparse_cpu.so: tests/test_gatv2_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import gatv2, heads, wide

import gatv2_cases as gc
import test_gpu_heads as th
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    gc.reference_against_autograd()      # before any library is tested: the reference's formulas are the gradient
    return gc.HipMemory()


@pytest.mark.parametrize("shape", gc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general(mem, shape):
    """300 x 517, 4000 entries, slope 0.2, 0 and 1, pad 0 and 8, lse taken and NULL, both forms, forward then backward with the lse just
    written, two backward calls with the same words, ga included"""
    gc.general(mem, (shape,))


def test_ties(mem):
    gc.ties(mem)


def test_heads_do_not_leak(mem):
    gc.heads_do_not_leak(mem)


def test_edges(mem):
    gc.edges(mem)


def test_a_call_leaves_nothing_for_the_next(mem):
    """hsgat2, then hsmh_backward_device over the same D words, then hsgat2 again"""
    gc.nothing_carried_over(mem)


def test_refusals(mem):
    gc.refusals(mem)


def test_info_is_unchanged_by_the_new_calls(mem):
    indptr, indices = gc.random_pattern(gc.ROWS, gc.COLS, gc.NNZ, 1)
    shape = (gc.ROWS, gc.COLS)
    with gatv2.GraphAttentionV2((indptr, indices, shape), 5) as ga, heads.MultiHeadAttention((indptr, indices, shape), 5) as mh:
        before = ga.info()
        assert before == mh.info() and before["nnz"] == gc.NNZ
        XD, XS, a, gY = gc.operands(shape, 5, 4, 15000)
        y, lse = gc.forward_device(mem, ga, XD, XS, a, 5, 0.2)
        gc.backward_device(mem, ga, XD, XS, a, gY, lse, 5, 0.2)
        gc.backward_host(ga, XD, XS, a, gY, lse, 5, 0.2)
        assert ga.work_bytes(5, 4) % (5 * 4 * 8) == 0 and ga.info() == before


def test_stride_loop_of_the_row_side_at_the_widest_group(mem):
    """rows of 1 ... 4 entries over 1000 columns at 4 heads of d = 64: one group of 64 lanes per row, four rows per workgroup, and more than
    two trips of the grid in the forward kernel and in the backward's row kernel, whose ga sums persist from one row to the next"""
    shape, indptr, indices = th._short_rows(1000, 256)
    with gatv2.GraphAttentionV2((indptr, indices, shape), 4) as ga:
        vectors = ga.work_bytes(4, 64) // (4 * 64 * 8)
    assert 2 * 4 * vectors < shape[0], (vectors, shape)      # every workgroup walks more than two workgroups' worth of rows
    gc.large(mem, shape, indptr, indices, 4, 64, 15110, f"{shape[0]} short rows, 4 heads of d 64")


def test_stride_loop_of_the_column_side_at_the_widest_group(mem):
    """the mirror image: that many columns of 1 ... 4 entries over 1000 rows, more than two trips of the grid in the column kernel"""
    shape, indptr, indices = th._transposed(*th._short_rows(1000, 256))
    lengths = np.bincount(indices, minlength=shape[1])
    assert shape[0] == 1000 and lengths.min() >= 1 and lengths.max() <= 4
    gc.large(mem, shape, indptr, indices, 4, 64, 15120, f"{shape[1]} short columns, 4 heads of d 64")


@pytest.mark.parametrize("heads_,d", [(5, 4), (4, 16)])
def test_long_rows_among_short_and_empty_rows(mem, heads_, d):
    """rows of 513, 1025 and 3000 entries: the four-wavefront merge of seventeen sums, and a ga vector out of class-0 and short-row
    workgroups together"""
    shape, indptr, indices = th._long_rows()
    fwd, bwd = gc.large(mem, shape, indptr, indices, heads_, d, 15210 + d, f"long rows among short and empty ones, {heads_} heads of d {d}")
    assert fwd[0].empty.sum() == shape[0] - 202 and sorted(bwd[0].n[bwd[0].n > wide.WIDE_LONG]) == [513, 1025, 3000]


@pytest.mark.parametrize("heads_,d", [(5, 4), (4, 16)])
def test_long_columns_among_short_and_empty_columns(mem, heads_, d):
    """the transpose-shaped twin, 4096 x 2001: columns of 513, 1025 and 3000 entries among short and empty ones"""
    shape, indptr, indices = th._transposed(*th._long_rows())
    fwd, bwd = gc.large(mem, shape, indptr, indices, heads_, d, 15220 + d, f"long columns among short and empty ones, {heads_} heads of d {d}")
    assert shape == (4096, 2001) and bwd[0].empty_c.sum() == shape[1] - 202 and sorted(bwd[0].m[bwd[0].m > wide.WIDE_LONG]) == [513, 1025, 3000]


def _words(mem, buf, w, ld):
    words = mem.fetch(buf).reshape(-1, ld)
    assert (words[:, w:] == gc.SENTINEL).all()
    return np.ascontiguousarray(words[:, :w]).view(np.float32)


def test_training_step_on_one_stream(mem):
    """hsgat2_forward_device then hsgat2_backward_device on a caller-owned stream, one synchronisation at the end: four launches.  Y and lse
    are inside the forward's bounds, gXD, gXS and ga inside the bounds computed from the lse words the device wrote.  2000 x 3000, 40 000
    entries, 3 heads of d = 8 with feature ld = 28 and lse ld = 4."""
    import scipy.sparse as sp
    n_rows, n_cols, H, d, ld, ldh, slope = 2000, 3000, 3, 8, 28, 4, 0.2
    w = H * d
    rng = np.random.default_rng(15300)
    flat = np.sort(rng.choice(n_rows * n_cols, 40000, replace=False))
    m = sp.csr_matrix((np.ones(flat.size, dtype=np.float32), (flat // n_cols, flat % n_cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    indptr, indices = m.indptr.astype(np.uint32), m.indices.astype(np.uint32)
    XD, XS, a, gY = gc.operands(m.shape, H, d, 15310)
    dd, ds, dg = (wc._features_in(mem, x, ld - w)[0] for x in (XD, XS, gY))
    da = gc._vector_in(mem, a)
    dy, od, os_ = (mem.alloc(np.full((n, ld), gc.SENTINEL, dtype=np.uint32)) for n in (n_rows, n_rows, n_cols))
    dl = mem.alloc(np.full((n_rows, ldh), gc.SENTINEL, dtype=np.uint32))
    oa = mem.alloc(np.full(w, gc.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with gatv2.GraphAttentionV2(m, H) as ga:
        nbytes = ga.work_bytes(H, d)
        work = mem.alloc(np.full(nbytes // 4, gc.NAN_WORD, dtype=np.uint32))
        ga.set_stream(st.value)
        ga.forward_device(dd.ptr, ld, ds.ptr, ld, da.ptr, H, d, slope, dy.ptr, ld, dl.ptr, ldh)
        ga.backward_device(dd.ptr, ld, ds.ptr, ld, da.ptr, dg.ptr, ld, dl.ptr, ldh, H, d, slope, od.ptr, ld, os_.ptr, ld, oa.ptr, work.ptr, nbytes)
        assert mem.rt.hipStreamSynchronize(st) == 0
        y, gxd, gxs = (_words(mem, b, w, ld) for b in (dy, od, os_))
        lse = _words(mem, dl, H, ldh)
        g_a = mem.fetch(oa).view(np.float32).reshape(H, d)
        ga.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    fwd = gc.forward_refs(indptr, indices, XD, XS, a, H, slope, exact=False)
    gc.check_forward(fwd, y, lse, "training step, forward")
    assert np.isfinite(lse[np.diff(indptr.astype(np.int64)) > 0]).all()
    gc.check_backward(gc.backward_refs(fwd, gY, lse), gxd, gxs, g_a, "training step, backward")
