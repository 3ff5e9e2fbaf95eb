"""The bf16 multi-head attention calls with a bias and dropout (include/hisparse_heads_dropout_bf16.h) on the device: the cases of
tests/heads16_dropout_cases.py against the HIP library -- every shape of heads16_cases.SHAPES and (8, 16) in both forms with a bias and
with NULL, drop_p = 0 against hsmh16_* bit for bit, forward and backward in agreement on the mask over a pattern whose column order is
not its CSR order and that holds a pair twice, fully dropped rows, the two precisions mixed, one row and one column of more than 512
entries among enough rows and columns that the grids' stride loops run, the edge patterns, seeds and offsets, a masking bias with
dropout, the refusals -- and a training step in bf16 on one caller-owned stream (three launches, one synchronisation).  The same cases on
libhisparse_cpu.so: tests/test_heads16_dropout_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import device, heads16_dropout, wide

import heads16_dropout_cases as hdx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return hdx.HipMemory()


@pytest.mark.parametrize("shape", hdx.GENERAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general(mem, shape):
    """300 x 517, 4000 entries, drop_p 0.1 and 0.5, a bias and NULL, both forms, tight and padded, lse and gbias taken and NULL"""
    hdx.general(mem, (shape,))


def test_drop_zero_gives_the_words_of_the_bf16_calls(mem):
    hdx.zero_drop(mem)


def test_forward_and_backward_agree_on_the_mask(mem):
    hdx.mask_agreement(mem)


def test_fully_dropped_rows(mem):
    hdx.fully_dropped_rows(mem)


def test_cross_precision(mem):
    hdx.cross_precision(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def test_long_rows_and_columns_and_the_stride_loops(mem):
    """one row of 600 and one column of 700 entries (a workgroup each, the four wavefronts merged through LDS) among n rows and n
    columns, nearly all of them empty and so of class 1: n is more than one trip of the grid at both shapes, (4, 32) and (3, 8), which
    the schedule takes at heads * d / 2 = 64 and 12 words, so the stride loops of all three kernels run; fewer than 3000 entries in all;
    drop_p = 0.5"""
    cu = _compute_units()
    n = max(20000, max(wide.rows_per_trip(cu, 1, w) for w in (64, 12)) + 1000)
    assert all(n > wide.rows_per_trip(cu, 1, w) for w in (64, 12))
    hdx.long_rows_and_columns(mem, n)


def test_edges(mem):
    hdx.edges(mem)


def test_seeds_and_offsets(mem):
    hdx.seeds_and_offsets(mem)


def test_a_masking_bias_with_dropout(mem):
    hdx.mask_and_dropout(mem)


def test_refusals(mem):
    hdx.refusals(mem)


def _features(mem, buf, w, ld):
    words = mem.fetch(buf).view(np.uint16).reshape(-1, ld)
    assert (words[:, w:] == hdx.h16.SENTINEL16).all()
    return heads16_dropout.from_bf16(words[:, :w])


def test_training_step_in_bf16_on_one_stream(mem):
    """hsmhd16_forward_device then hsmhd16_backward_device on a caller-owned stream, one synchronisation at the end: three launches.  Y
    and lse are inside the forward's bounds; gQ, gK, gV and gbias inside the bounds computed from the lse words the device wrote and the
    mask of hsmhd_keep_mask; hsmh_info is what it was before the calls.  1000 x 1500, 20 000 entries, 3 heads of d = 8 with ld = 32
    elements and ldl = ldb = ldgb = 4, drop_p = 0.2."""
    n_rows, n_cols, H, d, ld, lde, scale = 1000, 1500, 3, 8, 32, 4, 0.5
    dr = hdx.Drop(0.2, 0xC0FFEE, (1 << 32) + 5)
    w = H * d
    indptr, indices = hdx.random_pattern(n_rows, n_cols, 20000, 20000)
    nnz = indices.size
    Q, K, V, gY = hdx.operands((n_rows, n_cols), w, 20010)
    bias = hdx.biases(nnz, H, 20020)
    dq, dk, dv, dg = (hdx._features_in(mem, a, ld - w)[0] for a in (Q, K, V, gY))
    db = hdx.hb._entries_in(mem, bias, lde - H)[0]
    dy, oq, ok, ov = (hdx._out(mem, n, ld) for n in (n_rows, n_rows, n_cols, n_cols))
    dl = mem.alloc(np.full((n_rows, lde), hdx.SENTINEL, dtype=np.uint32))
    ob = mem.alloc(np.full((nnz, lde), hdx.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with heads16_dropout.DropoutMultiHeadAttentionBF16((indptr, indices, (n_rows, n_cols)), H) as mh:
        info = mh.info()
        mh.set_stream(st.value)
        mh.forward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, db.ptr, lde, H, d, scale, *dr.args(), dy.ptr, ld, dl.ptr, lde)
        mh.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, lde, db.ptr, lde, H, d, scale, *dr.args(), oq.ptr, ld, ok.ptr, ld, ov.ptr, ld, ob.ptr, lde)
        assert mem.rt.hipStreamSynchronize(st) == 0
        lw, gw = mem.fetch(dl).reshape(n_rows, lde), mem.fetch(ob).reshape(nnz, lde)
        y, gq, gk, gv = (_features(mem, b, w, ld) for b in (dy, oq, ok, ov))
        mh.set_stream(None)
        assert mh.info() == info, "hsmh_info changed"
    mem.rt.hipStreamDestroy(st)
    assert (lw[:, H:] == hdx.SENTINEL).all() and (gw[:, H:] == hdx.SENTINEL).all()
    lse, gb = np.ascontiguousarray(lw[:, :H]).view(np.float32), np.ascontiguousarray(gw[:, :H]).view(np.float32)
    W = dr.weights(nnz, H)
    assert 0.78 < (W != 0).mean() < 0.82
    scores = hdx.head_scores(indptr, indices, Q, K, H, exact=False)
    hdx.check_forward(hdx.forward_refs(scores, V, scale, bias, W), y, lse, "training step, forward")
    bwd = hdx.backward_refs(scores, V, gY, lse, scale, bias, W)
    hdx.check_backward(bwd, gq, gk, gv, "training step, backward")
    hdx.check_gbias(bwd, gb, "training step, gbias")
