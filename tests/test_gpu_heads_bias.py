"""The multi-head attention calls with a per-entry, per-head bias (include/hisparse_heads_bias.h) on the device: the cases of
tests/heads_bias_cases.py against the HIP library -- every shape of heads_cases.SHAPES in both forms, the edge patterns, a zero bias
against the plain calls bit for bit, masks, heads that do not leak, one row and one column of more than 512 entries among enough rows
and columns that the grids' stride loops run, which object takes which call, what hsmh_info reports, the refusals -- and a training step
with an edge bias on one caller-owned stream (three launches, one synchronisation).  The same cases on libhisparse_cpu.so:
tests/test_heads_bias_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import device, heads_bias, wide

import heads_bias_cases as hb
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return hb.HipMemory()


@pytest.mark.parametrize("shape", hb.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general(mem, shape):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, a bias in [-4, 4], both forms, tight and padded, lse and gbias taken and NULL"""
    hb.general(mem, (shape,))


def test_edges(mem):
    hb.edges(mem)


def test_zero_bias_gives_the_words_of_the_plain_calls(mem):
    hb.zero_bias(mem)


def test_mask(mem):
    hb.mask(mem)


def test_heads_do_not_leak(mem):
    hb.heads_do_not_leak(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def test_long_rows_and_columns_and_the_stride_loops(mem):
    """one row of 600 and one column of 700 entries (a workgroup each, the four wavefronts merged through LDS) among n rows and n
    columns, nearly all of them empty and so of class 1: n is more than one trip of the grid at both shapes, (4, 16) and (3, 8), so the
    stride loops of all three kernels run; fewer than 3000 entries in all"""
    cu = _compute_units()
    n = max(20000, max(wide.rows_per_trip(cu, 1, w) for w in (64, 24)) + 1000)
    assert all(n > wide.rows_per_trip(cu, 1, w) for w in (64, 24))
    hb.long_rows_and_columns(mem, n)


def test_objects(mem):
    hb.objects(mem)


def test_refusals(mem):
    hb.refusals(mem)


def _features(mem, buf, w, ld):
    words = mem.fetch(buf).reshape(-1, ld)
    assert (words[:, w:] == hb.SENTINEL).all()
    return np.ascontiguousarray(words[:, :w]).view(np.float32)


def test_training_step_with_an_edge_bias_on_one_stream(mem):
    """hsmhb_forward_device then hsmhb_backward_device on a caller-owned stream, one synchronisation at the end: three launches.  Y and
    lse are inside the forward's bounds; gQ, gK, gV and gbias inside the bounds computed from the lse words the device wrote.  1000 x
    1500, 20 000 entries, 3 heads of d = 8 with ld = 28 and ldl = ldb = ldgb = 4."""
    n_rows, n_cols, H, d, ld, lde, scale = 1000, 1500, 3, 8, 28, 4, 0.5
    w = H * d
    indptr, indices = hb.random_pattern(n_rows, n_cols, 20000, 12000)
    nnz = indices.size
    Q, K, V, gY = hb.operands((n_rows, n_cols), w, 12010)
    bias = hb.biases(nnz, H, 12020)
    dq, dk, dv, dg = (wc._features_in(mem, a, ld - w)[0] for a in (Q, K, V, gY))
    db = hb._entries_in(mem, bias, lde - H)[0]
    dy, oq, ok, ov = (mem.alloc(np.full((n, ld), hb.SENTINEL, dtype=np.uint32)) for n in (n_rows, n_rows, n_cols, n_cols))
    dl = mem.alloc(np.full((n_rows, lde), hb.SENTINEL, dtype=np.uint32))
    ob = mem.alloc(np.full((nnz, lde), hb.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with heads_bias.BiasedMultiHeadAttention((indptr, indices, (n_rows, n_cols)), H) as mh:
        mh.set_stream(st.value)
        mh.forward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, db.ptr, lde, H, d, scale, dy.ptr, ld, dl.ptr, lde)
        mh.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, lde, db.ptr, lde, H, d, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld, ob.ptr, lde)
        assert mem.rt.hipStreamSynchronize(st) == 0
        lw, gw = mem.fetch(dl).reshape(n_rows, lde), mem.fetch(ob).reshape(nnz, lde)
        y, gq, gk, gv = (_features(mem, b, w, ld) for b in (dy, oq, ok, ov))
        mh.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    assert (lw[:, H:] == hb.SENTINEL).all() and (gw[:, H:] == hb.SENTINEL).all()
    lse, gb = np.ascontiguousarray(lw[:, :H]).view(np.float32), np.ascontiguousarray(gw[:, :H]).view(np.float32)
    scores = hb.head_scores(indptr, indices, Q, K, H, exact=False)
    hb.check_forward(hb.forward_refs(scores, V, scale, bias), y, lse, "training step, forward")
    bwd = hb.backward_refs(scores, V, gY, lse, scale, bias)
    hb.check_backward(bwd, gq, gk, gv, "training step, backward")
    hb.check_gbias(bwd, gb, "training step, gbias")
