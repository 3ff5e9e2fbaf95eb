"""The neighbour aggregation (include/hisparse_aggregate.h) on the device: the cases of tests/aggregate_cases.py against the HIP library,
the stride loops of the two kernels over more than two trips of the grid at the widest group, long rows and long columns among short
and empty ones (the merge of a workgroup's four wavefronts through LDS, sums and (value, index) pairs), forward and backward on one
caller-owned stream (two launches, one synchronisation) and hsw_info unchanged by the new calls.  The same cases on libhisparse_cpu.so:
tests/test_aggregate_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import wide

import aggregate_cases as ac
import test_gpu_heads as th
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return ac.HipMemory()


@pytest.mark.parametrize("d", ac.DS)
def test_general(mem, d):
    """300 x 517, 4000 entries, every legal ops word, pad 0 and 8, args taken and NULL, both forms, forward then backward with the args just
    written"""
    ac.general(mem, (d,))


@pytest.mark.parametrize("d", (256, 4))
def test_winner_positions(mem, d):
    ac.winner_positions(mem, (d,))


def test_ties(mem):
    ac.ties(mem)


def test_non_finite_values(mem):
    ac.non_finite(mem)


def test_edges(mem):
    ac.edges(mem)


def test_backward_identities(mem):
    ac.backward_identities(mem)


def test_a_call_leaves_nothing_for_the_next(mem):
    """hsagg, then hsw_spmm_device, then hsagg again on one object"""
    ac.nothing_carried_over(mem)


def test_refusals(mem):
    ac.refusals(mem)


def test_info_is_unchanged_by_the_new_calls(mem):
    indptr, indices = ac.random_pattern(ac.ROWS, ac.COLS, ac.NNZ, 1)
    shape = (ac.ROWS, ac.COLS)
    ops = ac.MEAN | ac.MAX | ac.MIN
    with ac.open_pattern(indptr, indices, shape) as na, wide.WideProducts((indptr, indices, shape)) as wp:
        before = na.info()
        assert before == wp.info() and before["nnz"] == ac.NNZ and before["device_bytes"] > 0
        X = ac.features(ac.COLS, 20, 16000)
        fwd = ac.forward_device(mem, na, X, ops, 4, True)
        g = ac.gradients(ops, ac.ROWS, 20, 16010, fwd)
        ac.backward_device(mem, na, ops, g, 4)
        ac.forward_host(na, X, ops)
        ac.backward_host(na, ops, g)
        assert na.info() == before


def test_stride_loop_of_the_row_side_at_the_widest_group(mem):
    """rows of 1 ... 4 entries over 1000 columns at d = 256: one group of 64 lanes per row, four rows per workgroup, and more than two
    trips of the grid in the forward kernel"""
    shape, indptr, indices = th._short_rows(1000, 256)
    ac.large(mem, shape, indptr, indices, 256, 16110, f"{shape[0]} short rows, d 256")


def test_stride_loop_of_the_column_side_at_the_widest_group(mem):
    """the mirror image: that many columns of 1 ... 4 entries over 1000 rows, more than two trips of the grid in the backward kernel"""
    shape, indptr, indices = th._transposed(*th._short_rows(1000, 256))
    lengths = np.bincount(indices, minlength=shape[1])
    assert shape[0] == 1000 and lengths.min() >= 1 and lengths.max() <= 4
    ac.large(mem, shape, indptr, indices, 256, 16120, f"{shape[1]} short columns, d 256")


@pytest.mark.parametrize("d", (4, 20, 256))
def test_long_rows_among_short_and_empty_rows(mem, d):
    shape, indptr, indices = th._long_rows()
    fwd, bwd = ac.large(mem, shape, indptr, indices, d, 16210 + d, f"long rows among short and empty ones, d {d}")
    assert (fwd.n == 0).sum() == shape[0] - 202 and sorted(fwd.n[fwd.n > wide.WIDE_LONG]) == [513, 1025, 3000]


@pytest.mark.parametrize("d", (4, 20, 256))
def test_long_columns_among_short_and_empty_columns(mem, d):
    """the transpose-shaped twin, 4096 x 2001: columns of 513, 1025 and 3000 entries among short and empty ones"""
    shape, indptr, indices = th._transposed(*th._long_rows())
    fwd, bwd = ac.large(mem, shape, indptr, indices, d, 16220 + d, f"long columns among short and empty ones, d {d}")
    m = np.diff(bwd.cptr)
    assert shape == (4096, 2001) and bwd.empty.sum() == shape[1] - 202 and sorted(m[m > wide.WIDE_LONG]) == [513, 1025, 3000]


def _words(mem, buf, w, ld):
    words = mem.fetch(buf).reshape(-1, ld)
    assert (words[:, w:] == ac.SENTINEL).all()
    return np.ascontiguousarray(words[:, :w])


def test_forward_then_backward_on_one_stream(mem):
    """hsagg_forward_device then hsagg_backward_device on a caller-owned stream, the backward reading the arg arrays the forward is still
    writing when it is enqueued, one synchronisation at the end: two launches.  2000 x 3000, 40 000 entries, d = 24 with ld = 28, a PNA
    layer's MEAN | MAX | MIN."""
    import scipy.sparse as sp
    n_rows, n_cols, d, ld = 2000, 3000, 24, 28
    ops = ac.MEAN | ac.MAX | ac.MIN
    rng = np.random.default_rng(16300)
    flat = np.sort(rng.choice(n_rows * n_cols, 40000, replace=False))
    m = sp.csr_matrix((np.ones(flat.size, dtype=np.float32), (flat // n_cols, flat % n_cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    indptr, indices = m.indptr.astype(np.uint32), m.indices.astype(np.uint32)
    X = ac.features(n_cols, d, 16310)
    g = {"gsum": ac.features(n_rows, d, 16311), "gmax": ac.features(n_rows, d, 16312), "gmin": ac.features(n_rows, d, 16313)}
    dx = wc._features_in(mem, X, ld - d)[0]
    dg = {k: wc._features_in(mem, a, ld - d)[0] for k, a in g.items()}
    out = {k: mem.alloc(np.full((n_rows, ld), ac.SENTINEL, dtype=np.uint32)) for k in ("sum", "max", "amax", "min", "amin")}
    ogx = mem.alloc(np.full((n_cols, ld), ac.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with ac.open_pattern(indptr, indices, m.shape) as na:
        na.set_stream(st.value)
        na.forward_device(ops, dx.ptr, ld, d, out["sum"].ptr, out["max"].ptr, out["amax"].ptr, out["min"].ptr, out["amin"].ptr, ld)
        na.backward_device(ops, dg["gsum"].ptr, dg["gmax"].ptr, out["amax"].ptr, dg["gmin"].ptr, out["amin"].ptr, ld, d, ogx.ptr, ld)
        assert mem.rt.hipStreamSynchronize(st) == 0
        fwd = {k: _words(mem, b, d, ld) if k[0] == "a" else _words(mem, b, d, ld).view(np.float32) for k, b in out.items()}
        gx = _words(mem, ogx, d, ld).view(np.float32)
        na.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    ac.ForwardRef(indptr, indices, X, exact=False).check(fwd, ops, "one stream, forward")
    grads = dict(g, amax=fwd["amax"], amin=fwd["amin"])
    ac.BackwardRef(m.shape, indptr, indices, ops, grads, exact=False).check(gx, "one stream, backward")
