"""The multi-head attention calls with dropout on the attention weights (include/hisparse_heads_dropout.h) on the device: the cases of
tests/heads_dropout_cases.py against the HIP library -- every shape of heads_cases.SHAPES and (8, 16) in both forms with a bias and with
NULL, drop_p = 0 against the calls without dropout bit for bit, forward and backward in agreement on the mask over a pattern whose
column order is not its CSR order and that holds a pair twice, fully dropped rows, one row and one column of more than 512 entries among
enough rows and columns that the grids' stride loops run, the edge patterns, seeds and offsets, a masking bias with dropout, the
refusals -- and a training step with dropout on one caller-owned stream (three launches, one synchronisation).  The same cases on
libhisparse_cpu.so: tests/test_heads_dropout_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import device, heads_dropout, wide

import heads_dropout_cases as hd
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return hd.HipMemory()


@pytest.mark.parametrize("shape", hd.GENERAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general(mem, shape):
    """300 x 517, 4000 entries, drop_p 0.1 and 0.5, a bias and NULL, both forms, tight and padded, lse and gbias taken and NULL"""
    hd.general(mem, (shape,))


def test_drop_zero_gives_the_words_of_the_calls_without_dropout(mem):
    hd.zero_drop(mem)


def test_forward_and_backward_agree_on_the_mask(mem):
    hd.mask_agreement(mem)


def test_fully_dropped_rows(mem):
    hd.fully_dropped_rows(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def test_long_rows_and_columns_and_the_stride_loops(mem):
    """one row of 600 and one column of 700 entries (a workgroup each, the four wavefronts merged through LDS) among n rows and n
    columns, nearly all of them empty and so of class 1: n is more than one trip of the grid at both shapes, (4, 16) and (3, 8), so the
    stride loops of all three kernels run; fewer than 3000 entries in all; drop_p = 0.5"""
    cu = _compute_units()
    n = max(20000, max(wide.rows_per_trip(cu, 1, w) for w in (64, 24)) + 1000)
    assert all(n > wide.rows_per_trip(cu, 1, w) for w in (64, 24))
    hd.long_rows_and_columns(mem, n)


def test_edges(mem):
    hd.edges(mem)


def test_seeds_and_offsets(mem):
    hd.seeds_and_offsets(mem)


def test_a_masking_bias_with_dropout(mem):
    hd.mask_and_dropout(mem)


def test_refusals(mem):
    hd.refusals(mem)


def _features(mem, buf, w, ld):
    words = mem.fetch(buf).reshape(-1, ld)
    assert (words[:, w:] == hd.SENTINEL).all()
    return np.ascontiguousarray(words[:, :w]).view(np.float32)


def test_training_step_with_dropout_on_one_stream(mem):
    """hsmhd_forward_device then hsmhd_backward_device on a caller-owned stream, one synchronisation at the end: three launches.  Y and
    lse are inside the forward's bounds; gQ, gK, gV and gbias inside the bounds computed from the lse words the device wrote and the
    mask of hsmhd_keep_mask.  1000 x 1500, 20 000 entries, 3 heads of d = 8 with ld = 28 and ldl = ldb = ldgb = 4, drop_p = 0.2."""
    n_rows, n_cols, H, d, ld, lde, scale = 1000, 1500, 3, 8, 28, 4, 0.5
    dr = hd.Drop(0.2, 0xC0FFEE, (1 << 32) + 5)
    w = H * d
    indptr, indices = hd.random_pattern(n_rows, n_cols, 20000, 16000)
    nnz = indices.size
    Q, K, V, gY = hd.operands((n_rows, n_cols), w, 16010)
    bias = hd.biases(nnz, H, 16020)
    dq, dk, dv, dg = (wc._features_in(mem, a, ld - w)[0] for a in (Q, K, V, gY))
    db = hd.hb._entries_in(mem, bias, lde - H)[0]
    dy, oq, ok, ov = (mem.alloc(np.full((n, ld), hd.SENTINEL, dtype=np.uint32)) for n in (n_rows, n_rows, n_cols, n_cols))
    dl = mem.alloc(np.full((n_rows, lde), hd.SENTINEL, dtype=np.uint32))
    ob = mem.alloc(np.full((nnz, lde), hd.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with heads_dropout.DropoutMultiHeadAttention((indptr, indices, (n_rows, n_cols)), H) as mh:
        mh.set_stream(st.value)
        mh.forward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, db.ptr, lde, H, d, scale, *dr.args(), dy.ptr, ld, dl.ptr, lde)
        mh.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, lde, db.ptr, lde, H, d, scale, *dr.args(), oq.ptr, ld, ok.ptr, ld, ov.ptr, ld, ob.ptr, lde)
        assert mem.rt.hipStreamSynchronize(st) == 0
        lw, gw = mem.fetch(dl).reshape(n_rows, lde), mem.fetch(ob).reshape(nnz, lde)
        y, gq, gk, gv = (_features(mem, b, w, ld) for b in (dy, oq, ok, ov))
        mh.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    assert (lw[:, H:] == hd.SENTINEL).all() and (gw[:, H:] == hd.SENTINEL).all()
    lse, gb = np.ascontiguousarray(lw[:, :H]).view(np.float32), np.ascontiguousarray(gw[:, :H]).view(np.float32)
    W = dr.weights(nnz, H)
    assert 0.78 < (W != 0).mean() < 0.82
    scores = hd.head_scores(indptr, indices, Q, K, H, exact=False)
    hd.check_forward(hd.forward_refs(scores, V, scale, bias, W), y, lse, "training step, forward")
    bwd = hd.backward_refs(scores, V, gY, lse, scale, bias, W)
    hd.check_backward(bwd, gq, gk, gv, "training step, backward")
    hd.check_gbias(bwd, gb, "training step, gbias")
