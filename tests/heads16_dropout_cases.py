"""The cases of the bf16 calls with a bias and dropout of the multi-head attention object (include/hisparse_heads_dropout_bf16.h), shared
by tests/test_heads16_dropout_cpu.py (libhisparse_cpu.so, in a child process) and tests/test_gpu_heads16_dropout.py (the HIP library, on
the device), written against the memory interface of tests/pattern_cases.py.

Nothing is derived here.  Operands are heads16_cases.operands (rounded to bf16, handed around WIDENED), so the references are
heads_dropout_cases.forward_refs / backward_refs over exactly what the call computes on, with the weights of hsmhd_keep_mask; the header's
bound of a bf16 output word x with fp32 bound b is b + heads16_cases.bf16_term(x, b): forward_refs widens bound_y on the instance and
check_backward (heads16_cases') passes the term through check(..., extra=...).  lse and gbias are fp32 words and keep their bounds.  The
forms turn the feature arrays into bit patterns on the way in and widen the results on the way out; bias and gbias go as float32."""
import ctypes as C

import numpy as np

from hisparse_amd import heads as mha, heads16 as mh16, heads16_dropout as mhd16, heads_dropout as mhd

import heads16_cases as h16
import heads_bias_cases as hb
import heads_cases as hc
import heads_dropout_cases as hd
import pattern_cases as pc
from heads16_cases import FP32Face, _bits, _features_in, _features_out, _out, bf16_term, check_backward, operands  # noqa: F401
from heads_cases import cut, same_words, words  # noqa: F401
from heads_dropout_cases import Drop, backward_refs, biases, check_forward, check_gbias, head_scores, long_pattern, short_rows_pattern, twice_pattern, weights  # noqa: F401
from heads_dropout_cases import rounded_backward, rounded_forward, rounded_gbias  # noqa: F401
from pattern_cases import HipMemory, HostMemory, edge_patterns, random_pattern  # noqa: F401

BAD_ARG = -1
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
SENTINEL = hc.SENTINEL
# heads16_cases.SHAPES and (8, 16): one lane per head (d = 8), two (d = 16), the dealt path (d >= 32), more than four heads ((5, 8), (8, 16),
# (8, 64), (64, 8): counter word h >> 2 is not 0), 64 heads, the widest rows (8, 64) and (2, 256)
GENERAL_SHAPES = h16.SHAPES + ((8, 16),)
GENERAL = hd.GENERAL      # (drop_p, a bias or NULL, scale)
DEVICE = mhd16.DropoutMultiHeadAttentionBF16


def forward_refs(scores, V, scale, bias, W):
    refs = hd.forward_refs(scores, V, scale, bias, W)
    for r in refs:
        r.bound_y = r.bound_y + bf16_term(r.Y, r.bound_y)
    return refs


# ---- the forms: widened arrays in, widened arrays out; bias, lse and gbias float32 ---------------------------------------------------------
def forward_host(mh, Q, K, V, bias, heads, scale, dr, want_lse=True):
    """(y widened, lse or None)"""
    if want_lse:
        y, lse = DEVICE.forward(mh, _bits(Q), _bits(K), _bits(V), bias, heads, scale, *dr.args())
        return mh16.from_bf16(y), lse
    return mh16.from_bf16(DEVICE.forward(mh, _bits(Q), _bits(K), _bits(V), bias, heads, scale, *dr.args(), want_lse=False)), None


def forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, pad=0, extra=0, want_lse=True, what=""):
    """hsmhd16_forward_device over fresh buffers: the pads of the inputs NaN, y and lse pre-filled with a sentinel; the pad elements of y
    and the pad words of lse must survive.  bias None: the call is given NULL and ldb = 0."""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv) = (_features_in(mem, a, pad) for a in (Q, K, V))
    db, ldb = hb._entries_in(mem, bias, extra) if bias is not None else (None, 0)
    ldy, ldl = w + pad, heads + extra
    dy = _out(mem, mh.num_rows, ldy)
    dl = mem.alloc(np.full((mh.num_rows, ldl), SENTINEL, dtype=np.uint32)) if want_lse else None
    DEVICE.forward_device(mh, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, db.ptr if db else None, ldb, heads, w // heads, scale, *dr.args(), dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = _features_out(mem, mh, dy, mh.num_rows, w, ldy, what)
    if not want_lse:
        return y, None
    lw = mem.read(mh, dl).reshape(mh.num_rows, ldl)
    assert (lw[:, heads:] == SENTINEL).all(), f"{what}: the pad words of lse were written"
    return y, np.ascontiguousarray(lw[:, :heads]).view(np.float32)


def backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, dr, want_gbias=True):
    """(gq, gk, gv widened, gbias or None)"""
    gq, gk, gv, gb = DEVICE.backward(mh, _bits(Q), _bits(K), _bits(V), _bits(gY), lse, bias, heads, scale, *dr.args(), want_gbias=want_gbias)
    return mh16.from_bf16(gq), mh16.from_bf16(gk), mh16.from_bf16(gv), gb


def backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, pad=0, extra=0, want_gbias=True, what=""):
    """hsmhd16_backward_device over fresh buffers: the pads of the inputs NaN, the four outputs pre-filled with a sentinel; the pad elements
    of gq, gk and gv and the words h >= heads of gbias must survive"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (_features_in(mem, a, pad) for a in (Q, K, V, gY))
    dl, ldl = hc._lse_in(mem, lse, extra)
    db, ldb = hb._entries_in(mem, bias, extra) if bias is not None else (None, 0)
    ld, ldgb, nnz = w + pad, heads + extra, mh.nnz
    oq, ok, ov = (_out(mem, n, ld) for n in (mh.num_rows, mh.num_cols, mh.num_cols))
    ob = mem.alloc(np.full((nnz, ldgb), SENTINEL, dtype=np.uint32)) if want_gbias else None
    DEVICE.backward_device(mh, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, db.ptr if db else None, ldb, heads, w // heads, scale, *dr.args(), oq.ptr, ld, ok.ptr, ld,
                           ov.ptr, ld, ob.ptr if want_gbias else None, ldgb)
    out = tuple(_features_out(mem, mh, buf, n, w, ld, f"{what}, {name}") for name, buf, n in (("gq", oq, mh.num_rows), ("gk", ok, mh.num_cols), ("gv", ov, mh.num_cols)))
    if not want_gbias:
        return out + (None,)
    gw = mem.read(mh, ob).reshape(nnz, ldgb)
    assert (gw[:, heads:] == SENTINEL).all(), f"{what}: the words h >= heads of gbias were written"
    return out + (np.ascontiguousarray(gw[:, :heads]).view(np.float32),)


def all_forward_forms(mem, mh, refs, Q, K, V, bias, heads, scale, dr, what):
    """the host form with lse taken and NULL, the device form tight and padded (pad 8 elements, ldl = ldb = heads + 3), the padded one with
    lse NULL too, inside the bounds of one set of references; returns the lse of the host form"""
    y, lse = forward_host(mh, Q, K, V, bias, heads, scale, dr)
    check_forward(refs, y, lse, f"{what}, host form, lse taken")
    check_forward(refs, forward_host(mh, Q, K, V, bias, heads, scale, dr, False)[0], None, f"{what}, host form, lse NULL")
    for pad, extra, want in ((0, 0, True), (8, 3, True), (8, 3, False)):
        tag = f"{what}, device form, pad {pad}, ldl and ldb {heads + extra}, {'lse taken' if want else 'lse NULL'}"
        check_forward(refs, *forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, pad, extra, want, tag), tag)
    return lse


def all_backward_forms(mem, mh, refs, Q, K, V, gY, lse, bias, heads, scale, dr, what):
    """the host form and the device form tight and padded, each with gbias given and with NULL: the same gQ, gK and gV words either way"""
    worst = dict.fromkeys(hd.bc.OUTPUTS + ("gbias",), 0.0)
    for tag, call in ((f"{what}, host form", lambda want: backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, dr, want)),
                      (f"{what}, device form, pad 0", lambda want: backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, 0, 0, want, what)),
                      (f"{what}, device form, pad 8, ld {heads + 3}", lambda want: backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, 8, 3, want, what))):
        gq, gk, gv, gb = call(True)
        w = dict(check_backward(refs, gq, gk, gv, tag), gbias=check_gbias(refs, gb, tag))
        worst = {k: max(worst[k], w[k]) for k in worst}
        without = call(False)
        assert without[3] is None and same_words(without[:3], (gq, gk, gv)), f"{tag}: gbias NULL changes gq, gk or gv"
    return worst


def step(mem, mh, scores, Q, K, V, gY, bias, heads, scale, dr, what, pad=8, extra=1):
    """one device-form forward and the backward with the lse it wrote, both against the references; returns (y, lse, gq, gk, gv, gb)"""
    W = dr.weights(mh.nnz, heads)
    y, lse = forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, pad, extra, True, what)
    check_forward(forward_refs(scores, V, scale, bias, W), y, lse, what)
    bwd = backward_refs(scores, V, gY, lse, scale, bias, W)
    gq, gk, gv, gb = backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, pad, extra, True, what)
    check_backward(bwd, gq, gk, gv, what)
    check_gbias(bwd, gb, what)
    return y, lse, gq, gk, gv, gb


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def general(mem, shapes=GENERAL_SHAPES):
    """300 x 517, 4000 entries, every (heads, d) of heads16_cases.SHAPES and (8, 16); the four (drop_p, bias or NULL, scale) settings of
    heads_dropout_cases.GENERAL; forward in every form, then backward in every form with the lse the forward just wrote"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with DEVICE((indptr, indices, shape), heads) as mh:
            assert mh.nnz == NNZ
            Q, K, V, gY = operands(shape, heads * d, 17100 + 1000 * heads + d)
            given = biases(NNZ, heads, 17150 + 1000 * heads + d)
            scores = head_scores(indptr, indices, Q, K, heads)
            for i, (p, with_bias, scale) in enumerate(GENERAL):
                dr = Drop(p, 0x9E3779B97F4A7C15 + heads, (1 << 40) + 17 * i + d)
                bias = given if with_bias else None
                W = dr.weights(NNZ, heads)
                what = f"general, {heads} heads of d {d}, drop_p {p}, {'a bias' if with_bias else 'bias NULL'}, scale {scale}"
                lse = all_forward_forms(mem, mh, forward_refs(scores, V, scale, bias, W), Q, K, V, bias, heads, scale, dr, what)
                w = all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, scale, bias, W), Q, K, V, gY, lse, bias, heads, scale, dr, what)
                print(f"{what}: backward worst error / bound = {w['gq']:.3f} (gq), {w['gk']:.3f} (gk), {w['gv']:.3f} (gv), {w['gbias']:.3f} (gbias)")


class _Plain16:
    """the hsmh16_* calls on any object of the family, for the forms of heads16_cases.py, which call methods"""

    def __init__(self, mh):
        self._mh, self.num_rows, self.num_cols = mh, mh.num_rows, mh.num_cols

    def __getattr__(self, name):
        method = getattr(mh16.MultiHeadAttentionBF16, name)
        return lambda *a, **k: method(self._mh, *a, **k)


def zero_drop(mem, shapes=((4, 32), (5, 8), (2, 256), (8, 16))):
    """drop_p = 0: thr = 0 and c = 1.0, so with bias NULL and with a bias of all +0.0 every output word is bit for bit that of hsmh16_*,
    forward and backward, in both forms, whatever seed and offset say; gbias is inside its bound at a zero bias"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with DEVICE((indptr, indices, shape), heads) as mh:
            Q, K, V, gY = operands(shape, heads * d, 17700 + d)
            plain = _Plain16(mh)
            dr = Drop(0.0, 77 + d, 1 << 33)
            assert mhd.keep_mask(NNZ, heads, *dr.args()).all()
            zero = np.zeros((NNZ, heads), dtype=np.float32)
            assert not zero.view(np.uint32).any()      # +0.0
            scores = head_scores(indptr, indices, Q, K, heads)
            for scale in (0.5, -2.0):
                what = f"drop_p 0, {heads} heads of d {d}, scale {scale}"
                plain_f = h16.forward_device(mem, plain, Q, K, V, heads, scale, 8, 1, True, what)
                plain_fh = h16.forward_host(plain, Q, K, V, heads, scale)
                lse = plain_f[1]
                plain_b = h16.backward_device(mem, plain, Q, K, V, gY, lse, heads, scale, 8, 1, what)
                plain_bh = h16.backward_host(plain, Q, K, V, gY, lse, heads, scale)
                for bias, tag in ((None, "bias NULL"), (zero, "a +0.0 bias")):
                    assert same_words(plain_f, forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, 8, 1, True, what)), f"{what}, {tag}: the forward differs from hsmh16_forward_device"
                    assert same_words(plain_fh, forward_host(mh, Q, K, V, bias, heads, scale, dr)), f"{what}, {tag}: the host forward differs from hsmh16_forward"
                    got = backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, 8, 1, True, what)
                    assert same_words(plain_b, got[:3]), f"{what}, {tag}: the backward differs from hsmh16_backward_device"
                    assert same_words(plain_bh, backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, dr)[:3]), f"{what}, {tag}: the host backward differs from hsmh16_backward"
                    check_gbias(hb.backward_refs(scores, V, gY, lse, scale, zero), got[3], f"{what}, {tag}")


def mask_agreement(mem, shapes=((4, 32), (5, 8), (8, 16))):
    """Forward, row side and column side index the entries the same way: over heads_dropout_cases.twice_pattern(), whose column order is
    not its CSR order and which holds a pair twice, Y and all four gradients agree with the references built from hsmhd_keep_mask, in
    both forms.  The pair's two entries are two draws that differ in head 0."""
    indptr, indices, first, last = twice_pattern()
    shape = (60, 70)
    nnz = indices.size
    for heads, d in shapes:
        dr = Drop(0.5, 4243, 9)
        keep = mhd.keep_mask(nnz, heads, *dr.args())
        assert keep[first, 0] != keep[last, 0], "choose a seed for which the two entries of the pair draw differently in head 0"
        assert 0.3 < keep.mean() < 0.7
        Q, K, V, gY = operands(shape, heads * d, 18000 + d)
        bias = biases(nnz, heads, 18010 + d)
        scores = head_scores(indptr, indices, Q, K, heads)
        W = weights(keep, dr.p)
        with DEVICE((indptr, indices, shape), heads) as mh:
            assert mh.nnz == nnz
            what = f"forward and backward agree on the mask, {heads} heads of d {d}"
            lse = all_forward_forms(mem, mh, forward_refs(scores, V, 0.5, bias, W), Q, K, V, bias, heads, 0.5, dr, what)
            all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, 0.5, bias, W), Q, K, V, gY, lse, bias, heads, 0.5, dr, what)
            step(mem, mh, scores, Q, K, V, gY, None, heads, 0.5, dr, what + ", bias NULL")


def fully_dropped_rows(mem, shapes=((4, 32), (3, 8))):
    """drop_p = 0.9 on rows of 1 to 3 entries: the mask does leave (row, head) pairs with entries and no kept entry (asserted first, on the
    host); such a pair reads the word 0x0000 in its d elements of Y, not NaN; lse is, word for word, the lse of the call without
    dropout; the backward agrees with the reference and gQ of such a head is 0x0000 too"""
    indptr, indices = short_rows_pattern()
    shape = (200, 90)
    nnz = indices.size
    of = pc.entry_rows(indptr)
    for heads, d in shapes:
        dr = Drop(0.9, 5, 3)
        keep = mhd.keep_mask(nnz, heads, *dr.args())
        kept = np.stack([np.bincount(of[keep[:, h] != 0], minlength=200) for h in range(heads)], axis=1)      # (rows, heads)
        nonempty = np.diff(indptr.astype(np.int64)) > 0
        gone = nonempty[:, None] & (kept == 0)
        assert gone.any() and (nonempty[:, None] & (kept > 0)).any(), "the case needs both kinds of (row, head)"
        Q, K, V, gY = operands(shape, heads * d, 18100 + d)
        bias = biases(nnz, heads, 18110 + d)
        scores = head_scores(indptr, indices, Q, K, heads)
        with DEVICE((indptr, indices, shape), heads) as mh:
            for b in (bias, None):
                what = f"fully dropped rows, {heads} heads of d {d}, {'a bias' if b is not None else 'bias NULL'}"
                for form in ("host", "device"):
                    y, lse = forward_host(mh, Q, K, V, b, heads, 0.5, dr) if form == "host" else forward_device(mem, mh, Q, K, V, b, heads, 0.5, dr, 8, 1, True, what)
                    y0, lse0 = forward_host(mh, Q, K, V, b, heads, 0.5, Drop(0.0, 0, 0))
                    assert same_words((lse,), (lse0,)), f"{what}, {form} form: lse is not the lse without dropout"
                    assert not words(y).reshape(200, heads, d)[gone].any(), f"{what}, {form} form: a fully dropped (row, head) is not 0x0000"
                    assert np.isfinite(y).all() and np.isfinite(lse[nonempty]).all()
                    assert (words(y0).reshape(200, heads, d)[gone] != 0).any()
                y, lse, gq, gk, gv, gb = step(mem, mh, scores, Q, K, V, gY, b, heads, 0.5, dr, what)
                assert not words(gq).reshape(200, heads, d)[gone].any(), f"{what}: gq of a fully dropped (row, head) is not 0x0000"
                assert (gb[~(keep != 0) & nonempty[of][:, None] & ~gone[of]] != 0).any(), "a dropped entry's gbias word is -P D, not zero"


def cross_precision(mem, heads=4, d=32):
    """a forward in one precision, the backward in the other, on one object with the same (drop_p, seed, offset): the bf16 forward's lse fed
    to hsmhd_backward_device on the widened operands, and hsmhd_forward_device's lse fed to the bf16 backward; every word inside the bounds
    of the references built from the lse words given and ONE mask"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 6)
    shape = (ROWS, COLS)
    scale, dr = 0.25, Drop(0.3, 0xABCDEF0123, (3 << 32) + 11)
    with DEVICE((indptr, indices, shape), heads) as mh:
        Q, K, V, gY = operands(shape, heads * d, 18200)
        bias = biases(NNZ, heads, 18210)
        scores = head_scores(indptr, indices, Q, K, heads)
        W = dr.weights(NNZ, heads)
        for b in (bias, None):
            tag = "a bias" if b is not None else "bias NULL"
            y16, lse16 = forward_device(mem, mh, Q, K, V, b, heads, scale, dr, 8, 1, True, "cross")
            check_forward(forward_refs(scores, V, scale, b, W), y16, lse16, f"cross precision, bf16 forward, {tag}")
            g32 = hd.backward_device(mem, mh, Q, K, V, gY, lse16, b, heads, scale, dr, 4, 1, True, "cross")
            r32 = hd.backward_refs(scores, V, gY, lse16, scale, b, W)
            hd.check_backward(r32, *g32[:3], f"cross precision, fp32 backward from the bf16 lse, {tag}")
            check_gbias(r32, g32[3], f"cross precision, fp32 backward from the bf16 lse, {tag}")
            y32, lse32 = hd.forward_device(mem, mh, Q, K, V, b, heads, scale, dr, 4, 1, True, "cross")
            hd.check_forward(hd.forward_refs(scores, V, scale, b, W), y32, lse32, f"cross precision, fp32 forward, {tag}")
            g16 = backward_device(mem, mh, Q, K, V, gY, lse32, b, heads, scale, dr, 8, 1, True, "cross")
            r16 = backward_refs(scores, V, gY, lse32, scale, b, W)
            check_backward(r16, *g16[:3], f"cross precision, bf16 backward from the fp32 lse, {tag}")
            check_gbias(r16, g16[3], f"cross precision, bf16 backward from the fp32 lse, {tag}")


def long_rows_and_columns(mem, n, shapes=((4, 32), (3, 8))):
    """the device forms over heads_bias_cases.long_pattern(n) (one row of 600 and one column of 700 entries), drop_p 0.5, forward then
    backward with the lse just written, float64 sums in the references; n is chosen by the caller so that the grid's stride loop runs"""
    indptr, indices = long_pattern(n)
    shape = (n, n)
    for heads, d in shapes:
        what = f"long row and column among {n}, {heads} heads of d {d}, drop_p 0.5"
        Q, K, V, gY = operands(shape, heads * d, 18300 + d)
        bias = biases(indices.size, heads, 18310 + d)
        scores = head_scores(indptr, indices, Q, K, heads, exact=False)
        dr = Drop(0.5, 99, (1 << 32) + 1)
        with DEVICE((indptr, indices, shape), heads) as mh:
            got = step(mem, mh, scores, Q, K, V, gY, bias, heads, 0.5, dr, what)
            assert same_words(got[2:], backward_device(mem, mh, Q, K, V, gY, got[1], bias, heads, 0.5, dr, 8, 1, True, what)), f"{what}: two calls give other words"
            step(mem, mh, scores, Q, K, V, gY, None, heads, 0.5, dr, what + ", bias NULL")


def edges(mem, heads=3, d=8):
    """every pattern of pattern_cases.edge_patterns() at (3, 8) with drop_p 0.5, a bias and NULL: empty rows and columns (0x0000, and -inf
    in lse), nnz = 0 with NULL indices (no per-entry pointer is dereferenced), one entry, unsorted columns, a pair held twice"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with DEVICE((indptr, indices, shape), heads) as mh:
            assert mh.nnz == indices.size
            Q, K, V, gY = operands(shape, heads * d, 18400)
            given = biases(indices.size, heads, 18410)
            scores = head_scores(indptr, indices, Q, K, heads)
            dr = Drop(0.5, 8, 2)
            W = dr.weights(indices.size, heads)
            assert W.shape == (indices.size, heads)
            for bias in (given, None):
                what = f"{name}, {'a bias' if bias is not None else 'bias NULL'}"
                fwd = forward_refs(scores, V, 1.5, bias, W)
                lse = all_forward_forms(mem, mh, fwd, Q, K, V, bias, heads, 1.5, dr, what)
                assert (lse[fwd[0].empty] == -np.inf).all()
                all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, 1.5, bias, W), Q, K, V, gY, lse, bias, heads, 1.5, dr, what)


def seeds_and_offsets(mem, heads=5, d=8):
    """different seeds give different masks and different words; offset k and offset 2^32 + k too (the high word of the offset is used),
    and so do the two halves of the seed; the same inputs twice give the same words"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    Q, K, V, gY = operands(shape, heads * d, 18500)
    bias = biases(NNZ, heads, 18510)
    scores = head_scores(indptr, indices, Q, K, heads)
    base = Drop(0.5, 1234, 7)
    others = (Drop(0.5, 1235, 7), Drop(0.5, 1234 + (1 << 32), 7), Drop(0.5, 1234, 8), Drop(0.5, 1234, (1 << 32) + 7))
    with DEVICE((indptr, indices, shape), heads) as mh:
        k0 = mhd.keep_mask(NNZ, heads, *base.args())
        first = step(mem, mh, scores, Q, K, V, gY, bias, heads, 0.5, base, "seeds and offsets, base")
        again = step(mem, mh, scores, Q, K, V, gY, bias, heads, 0.5, base, "seeds and offsets, base again")
        assert same_words(first, again), "the same inputs twice give other words"
        for dr in others:
            k1 = mhd.keep_mask(NNZ, heads, *dr.args())
            differ = (k0 != k1).mean()
            assert 0.4 < differ < 0.6, f"seed {dr.seed:#x}, offset {dr.offset:#x}: {differ:.3f} of the decisions differ from the base's"
            got = step(mem, mh, scores, Q, K, V, gY, bias, heads, 0.5, dr, f"seeds and offsets, seed {dr.seed:#x}, offset {dr.offset:#x}")
            assert not np.array_equal(words(got[0]), words(first[0])) and same_words((got[1],), (first[1],)), "another mask, the same lse"


def mask_and_dropout(mem, heads=4, d=32):
    """A -inf bias on a random third of the entries (the first entry of every row stays) together with drop_p 0.5 computes what the pattern
    WITHOUT those entries computes under the same draws for the remaining entries' CSR indices of the ORIGINAL pattern.  The masked
    entries' gbias words are zero."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 6)
    shape = (ROWS, COLS)
    rng = np.random.default_rng(18600)
    of = pc.entry_rows(indptr)
    masked = rng.random(NNZ) < 1.0 / 3.0
    masked[indptr[:-1][np.diff(indptr.astype(np.int64)) > 0]] = False
    stay = ~masked
    assert NNZ // 4 < masked.sum() < NNZ // 2
    kptr = np.zeros(ROWS + 1, dtype=np.uint32)
    kptr[1:] = np.cumsum(np.bincount(of[stay], minlength=ROWS))
    kidx = indices[stay]
    Q, K, V, gY = operands(shape, heads * d, 18610)
    bias = biases(NNZ, heads, 18620)
    scale, dr = 0.5, Drop(0.5, 31337, 12)
    W = dr.weights(NNZ, heads)[stay]      # the draws of the ORIGINAL indices
    assert not np.array_equal(W, dr.weights(int(stay.sum()), heads)), "the reduced pattern's own draws would be others"
    scores = head_scores(kptr, kidx, Q, K, heads)
    fwd = forward_refs(scores, V, scale, bias[stay], W)
    with_mask = bias.copy()
    with_mask[masked] = -np.inf
    with DEVICE((indptr, indices, shape), heads) as mh:
        for form in ("host", "device"):
            what = f"a -inf bias with dropout, {form} form"
            y, lse = forward_host(mh, Q, K, V, with_mask, heads, scale, dr) if form == "host" else forward_device(mem, mh, Q, K, V, with_mask, heads, scale, dr, 8, 1, True, what)
            check_forward(fwd, y, lse, what)
            bwd = backward_refs(scores, V, gY, lse, scale, bias[stay], W)
            got = backward_host(mh, Q, K, V, gY, lse, with_mask, heads, scale, dr) if form == "host" else backward_device(mem, mh, Q, K, V, gY, lse, with_mask, heads, scale, dr, 8, 1, True, what)
            check_backward(bwd, *got[:3], what)
            check_gbias(bwd, got[3][stay], what)
            assert not (got[3][masked] != 0).any(), f"{what}: a masked entry's gbias word is not zero"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
FEATURES = hc.FEATURES
BAD_DROPS = hd.BAD_DROPS


def refusals(mem):
    """every rule of the header: d = 4, heads * d = 520 and 1024, ld not a multiple of 8 or below heads * d, a misaligned pointer, overlap
    (bias and gbias among them), every bad drop_p, and a backward on an object without the entry map (the message names hsmhb_create), with
    a bias and without; each is HS_ERR_BAD_ARG with a message, the forward runs on any object, hsmh_info reports what it reported, and
    after every refusal the object gives the words it gave"""
    l = mhd16.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    heads, d = 2, 8
    w = heads * d
    one = np.zeros(8, dtype=np.uint32).ctypes.data
    assert l.hsmhd16_forward_device(None, vp(one), 8, vp(one), 8, vp(one), 8, vp(one), 1, 1, 8, 1.0, 0.5, 1, 1, vp(one), 8, None, 1) == BAD_ARG
    assert l.hsmhd16_forward(None, vp(one), vp(one), vp(one), vp(one), 1, 8, 1.0, 0.5, 1, 1, vp(one), None) == BAD_ARG
    assert l.hsmhd16_backward_device(None, vp(one), 8, vp(one), 8, vp(one), 8, vp(one), 8, vp(one), 1, vp(one), 1, 1, 8, 1.0, 0.5, 1, 1, vp(one), 8, vp(one), 8, vp(one), 8, None, 1) == BAD_ARG
    assert l.hsmhd16_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), vp(one), 1, 8, 1.0, 0.5, 1, 1, vp(one), vp(one), vp(one), None) == BAD_ARG
    dr = Drop(0.25, 3, 4)
    with DEVICE((indptr, indices, shape), 4) as mh, mha.MultiHeadAttention((indptr, indices, shape), 4) as plain, DEVICE((indptr, indices, shape), 4, backward=False) as no_flag:
        Q, K, V, gY = operands(shape, w, 18700)
        bias = biases(7, heads, 18710)
        scores = head_scores(indptr, indices, Q, K, heads)
        W = dr.weights(7, heads)
        want_f = forward_host(mh, Q, K, V, bias, heads, 0.5, dr)
        check_forward(forward_refs(scores, V, 0.5, bias, W), *want_f, "refusals")
        want_b = backward_host(mh, Q, K, V, gY, want_f[1], bias, heads, 0.5, dr)
        brefs = backward_refs(scores, V, gY, want_f[1], 0.5, bias, W)
        check_backward(brefs, *want_b[:3], "refusals")
        check_gbias(brefs, want_b[3], "refusals")
        info = {obj: obj.info() for obj in (mh, plain, no_flag)}

        # which object: the forward on any, the backward only with the map
        for obj in (plain, no_flag):
            assert same_words(want_f, forward_host(obj, Q, K, V, bias, heads, 0.5, dr)), "the forward on an object without the map"
            assert same_words(want_f, forward_device(mem, obj, Q, K, V, bias, heads, 0.5, dr, 8, 1, True, "no map"))
            for b in (bias, None):
                for call in (lambda: backward_host(obj, Q, K, V, gY, want_f[1], b, heads, 0.5, dr), lambda: backward_device(mem, obj, Q, K, V, gY, want_f[1], b, heads, 0.5, dr)):
                    try:
                        call()
                    except mha.DeviceError as e:
                        assert e.code == BAD_ARG and "hsmhb_create" in str(e), str(e)
                    else:
                        raise AssertionError("the bf16 backward with dropout ran on an object without the entry map")
            assert same_words(want_f, forward_host(obj, Q, K, V, bias, heads, 0.5, dr)), "unusable after the refused backward"
        assert {obj: obj.info() for obj in (mh, plain, no_flag)} == info, "hsmh_info changed"

        def still_usable(rc, what):
            assert rc == BAD_ARG and l.hsmh_last_error(mh._h), (what, rc)
            assert same_words(forward_host(mh, Q, K, V, bias, heads, 0.5, dr), want_f), f"unusable after {what}"
            assert same_words(backward_host(mh, Q, K, V, gY, want_f[1], bias, heads, 0.5, dr), want_b), f"unusable after {what}"

        def forward_call(a):
            return l.hsmhd16_forward_device(mh._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["bias"]), a["ldb"], a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6,
                                            vp(a["y"]), a["ldy"], vp(a["lse"]), a["ldl"])

        def backward_call(a):
            return l.hsmhd16_backward_device(mh._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["ldl"], vp(a["bias"]), a["ldb"],
                                             a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6, vp(a["gq"]), a["ldgq"], vp(a["gk"]), a["ldgk"], vp(a["gv"]), a["ldgv"], vp(a["gbias"]), a["ldgb"])

        # buffers of 9 rows x 32 elements (ld = 16 elements: 32 bytes a row), 16-byte aligned; lse: 6 rows, bias and gbias: 7 rows of 2 words
        names = FEATURES + ("y", "lse", "bias", "gbias")
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 16 for name in FEATURES + ("y",)}, heads=heads, d=d, scale=1.0, drop_p=0.5, ldl=2, ldb=2, ldgb=2)
        no_bias = dict(ok, bias=None, ldb=0)
        wide_ld = {"ld" + n: 1024 for n in FEATURES + ("y",)}
        assert forward_call(ok) == 0 and backward_call(ok) == 0 and backward_call(dict(ok, gbias=None, ldgb=0)) == 0
        assert forward_call(no_bias) == 0 and backward_call(no_bias) == 0 and backward_call(dict(no_bias, gbias=None, ldgb=0)) == 0
        for bad in BAD_DROPS:
            for base in (ok, no_bias):
                still_usable(forward_call(dict(base, drop_p=bad)), f"forward_device: drop_p {bad}")
                assert b"drop_p" in l.hsmh_last_error(mh._h)
                still_usable(backward_call(dict(base, drop_p=bad)), f"backward_device: drop_p {bad}")
                assert b"drop_p" in l.hsmh_last_error(mh._h)
        shared = [("d = 4", dict(d=4)), ("d = 12", dict(heads=1, d=12)), ("heads * d = 520", dict(wide_ld, heads=65, d=8)), ("heads * d = 1024", dict(wide_ld, heads=4, d=256)),
                  ("heads * d = 768", dict(wide_ld, heads=3, d=256)), ("heads > max_heads", dict(heads=5)), ("scale NaN", dict(scale=float("nan"))), ("ldl < heads", dict(ldl=1)),
                  ("misaligned lse", dict(lse=ok["lse"] + 2)), ("misaligned bias", dict(bias=ok["bias"] + 2)), ("ldb < heads", dict(ldb=1))]
        for name in ("q", "k", "v"):
            shared += [(f"null {name}", {name: None}), (f"misaligned {name} by 2", {name: ok[name] + 2}), (f"misaligned {name} by 8", {name: ok[name] + 8}),
                       (f"ld{name} % 8", {"ld" + name: 20}), (f"ld{name} < heads * d", {"ld" + name: 8})]
        for what, change in shared:
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        for what, change in (("y is bias", dict(y=ok["bias"])), ("lse is bias", dict(lse=ok["bias"])), ("y is q", dict(y=ok["q"])), ("y inside k", dict(y=ok["k"] + 64)),
                             ("lse inside y", dict(lse=ok["y"] + 16)), ("misaligned y", dict(y=ok["y"] + 4)), ("ldy % 8", dict(ldy=20)), ("null y", dict(y=None))):
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("misaligned gbias", dict(gbias=ok["gbias"] + 2)), ("ldgb < heads", dict(ldgb=1)), ("gq is bias", dict(gq=ok["bias"])), ("gv inside bias", dict(gv=ok["bias"] + 16)),
                  ("gq is q", dict(gq=ok["q"])), ("gk is gq", dict(gk=ok["gq"])), ("misaligned gy", dict(gy=ok["gy"] + 4)), ("null lse", dict(lse=None)), ("ldgq % 8", dict(ldgq=20)),
                  ("ldgv < heads * d", dict(ldgv=8)), ("misaligned gk", dict(gk=ok["gk"] + 8))]
        bcases += [(f"gbias is {name}", dict(gbias=ok[name])) for name in ("q", "k", "v", "gy", "lse", "bias", "gq", "gk", "gv")]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        for what, change in [("misaligned gbias", dict(gbias=ok["gbias"] + 2)), ("ldgb < heads", dict(ldgb=1))] + [(f"gbias is {name}", dict(gbias=ok[name])) for name in ("q", "lse", "gk")]:
            still_usable(backward_call(dict(no_bias, **change)), "backward_device, bias NULL: " + what)
        # a refused shape names the rule
        assert forward_call(dict(ok, d=4)) == BAD_ARG and "8, 16, 32, 64, 128, 256" in l.hsmh_last_error(mh._h).decode()
        assert forward_call(dict(ok, **wide_ld, heads=4, d=256)) == BAD_ARG and "at most 512" in l.hsmh_last_error(mh._h).decode()
        # the host forms
        host = {name: np.zeros(9 * 16, np.uint32) for name in names}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, heads=heads, d=d, scale=1.0, drop_p=0.5)

        def forward_host_call(a):
            return l.hsmhd16_forward(mh._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["bias"]), a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6, vp(a["y"]), vp(a["lse"]))

        def backward_host_call(a):
            return l.hsmhd16_backward(mh._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), vp(a["bias"]), a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6, vp(a["gq"]),
                                      vp(a["gk"]), vp(a["gv"]), vp(a["gbias"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0 and backward_host_call(dict(okh, gbias=None)) == 0
        assert forward_host_call(dict(okh, bias=None)) == 0 and backward_host_call(dict(okh, bias=None)) == 0
        for bad in BAD_DROPS:
            still_usable(forward_host_call(dict(okh, drop_p=bad)), f"forward: drop_p {bad}")
            still_usable(backward_host_call(dict(okh, drop_p=bad, bias=None)), f"backward: drop_p {bad}")
        for what, change in (("y is bias", dict(y=okh["bias"])), ("d = 4", dict(d=4)), ("heads * d = 1024", dict(heads=4, d=256)), ("null q", dict(q=None)), ("y is k", dict(y=okh["k"]))):
            still_usable(forward_host_call(dict(okh, **change)), "forward: " + what)
        for what, change in (("gbias is bias", dict(gbias=okh["bias"])), ("gbias is gk", dict(gbias=okh["gk"], bias=None)), ("gq is bias", dict(gq=okh["bias"])), ("null lse", dict(lse=None)),
                             ("d = 4", dict(d=4)), ("gq is gk", dict(gq=okh["gk"]))):
            still_usable(backward_host_call(dict(okh, **change)), "backward: " + what)
        for obj, call in ((plain, "hsmh_create"), (no_flag, "no flag")):
            rc = l.hsmhd16_backward_device(obj._h, vp(ok["q"]), 16, vp(ok["k"]), 16, vp(ok["v"]), 16, vp(ok["gy"]), 16, vp(ok["lse"]), 2, None, 0, heads, d, 1.0, 0.5, 5, 6, vp(ok["gq"]), 16,
                                           vp(ok["gk"]), 16, vp(ok["gv"]), 16, None, 0)
            assert rc == BAD_ARG and b"hsmhb_create" in l.hsmh_last_error(obj._h), call
        mh.set_stream(None)
        mh.sync()
