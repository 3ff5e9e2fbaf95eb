"""The cases of the bf16 calls of the multi-head attention object (include/hisparse_heads_bf16.h), shared by tests/test_heads16_cpu.py
(libhisparse_cpu.so, in a child process) and tests/test_gpu_heads16.py (the HIP library, on the device), written against the memory
interface of tests/pattern_cases.py.

Operands are heads_cases.operands(...) rounded to bf16 and handed around WIDENED (float32 arrays whose every word is a bf16 value), so
that the references are heads_cases.forward_refs / backward_refs over exactly what the call computes on; the forms below turn them into
bit patterns on the way in and widen the results on the way out.  attention_cases.Reference and attention_backward_cases.Reference are
used unchanged.  The header's bound of an output word x with fp32 bound b is b + 2^-8 (|x| + b) + 2^-134 (half a bf16 ulp, half the
bf16 subnormal spacing): forward_refs widens bound_y on the instance, check_backward passes the term through check(..., extra=...).
lse has no extra term.  No other tolerance is introduced.  Both references assert their input condition (rho <= 2^-12) themselves, on
the rounded operands."""
import ctypes as C

import numpy as np

from hisparse_amd import heads as mha, heads16 as mh16

import attention_backward_cases as bc
import heads_cases as hc
import pattern_cases as pc
from heads_cases import check_forward, cut, head_scores, rounded_backward, rounded_forward, same_words  # noqa: F401
from pattern_cases import HipMemory, HostMemory, edge_patterns, random_pattern  # noqa: F401

BAD_ARG = -1
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
SENTINEL16, NAN16 = 0xDEAD, 0x7FC0
HALF_ULP, HALF_SUBNORMAL = 2.0 ** -8, 2.0 ** -134
# head widths of 1, 2, 4, 8, ... lanes, both sides of the weight-dealing switch (d = 16 and 32), dead lanes ((5, 8), (3, 16), (3, 32)), the 64-lane group
SHAPES = ((1, 8), (2, 8), (5, 8), (3, 16), (4, 32), (3, 32), (2, 64), (4, 64), (4, 128), (2, 256), (8, 64), (64, 8))


def bf16_term(x, b):
    """what the second rounding adds to the bound b of a word whose reference is x"""
    return HALF_ULP * (np.abs(x) + b) + HALF_SUBNORMAL


def twice(a):
    """float64 or float32 words rounded to fp32 and then to bf16, widened again"""
    return mh16.from_bf16(mh16.to_bf16(np.asarray(a).astype(np.float32)))


# ---- references ----------------------------------------------------------------------------------------------------------------------
def operands(shape, width, seed):
    """Q, K, V, gY of heads_cases.operands rounded to bf16, widened"""
    return tuple(twice(a) for a in hc.operands(shape, width, seed))


def forward_refs(scores, V, scale):
    refs = hc.forward_refs(scores, V, scale)
    for r in refs:
        r.bound_y = r.bound_y + bf16_term(r.Y, r.bound_y)
    return refs


backward_refs = hc.backward_refs


def check_backward(refs, gq, gk, gv, what):
    d = refs[0].d
    worst = dict.fromkeys(bc.OUTPUTS, 0.0)
    for got, n in ((gq, refs[0].GQ.shape[0]), (gk, refs[0].GK.shape[0]), (gv, refs[0].GV.shape[0])):
        assert np.asarray(got).shape == (n, len(refs) * d), (what, np.asarray(got).shape)
    for h, r in enumerate(refs):
        extra = {name: bf16_term(r.want[name], r.bound[name]) for name in bc.OUTPUTS}
        w = r.check(cut(gq, h, d), cut(gk, h, d), cut(gv, h, d), f"{what}, head {h}", extra=extra)
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


# ---- the forms: widened arrays in, widened arrays out -----------------------------------------------------------------------------------
class FP32Face:
    """the fp32 calls of the same object (the base class's methods on the same handle), for heads_cases' forms"""
    def __init__(self, obj):
        self._o, self.num_rows, self.num_cols = obj, obj.num_rows, obj.num_cols

    def __getattr__(self, name):
        if name in ("forward", "backward", "forward_device", "backward_device"):
            return getattr(mha.MultiHeadAttention, name).__get__(self._o)
        return getattr(self._o, name)


def _bits(a):
    b = mh16.to_bf16(a)
    assert np.array_equal(mh16.from_bf16(b).view(np.uint32), np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)), "an operand that is not a bf16 value"
    return b


def _features_in(mem, a, pad):
    """a (n, w) on the device as bf16 with ld = w + pad elements, the pad elements NaN"""
    ld = a.shape[1] + pad
    buf = np.full((a.shape[0], ld), NAN16, dtype=np.uint16)
    buf[:, : a.shape[1]] = _bits(a)
    return mem.alloc(buf.view(np.uint32)), ld


def _out(mem, n, ld):
    return mem.alloc(np.full((n, ld), SENTINEL16, dtype=np.uint16).view(np.uint32))


def _features_out(mem, mh, buf, n, w, ld, what):
    words = mem.read(mh, buf).view(np.uint16).reshape(n, ld)
    assert (words[:, w:] == SENTINEL16).all(), f"{what}: the pad elements of the result were written"
    return mh16.from_bf16(words[:, :w])


def forward_host(mh, Q, K, V, heads, scale, want_lse=True):
    """(y widened, lse or None)"""
    if want_lse:
        y, lse = mh.forward(_bits(Q), _bits(K), _bits(V), heads, scale)
        return mh16.from_bf16(y), lse
    return mh16.from_bf16(mh.forward(_bits(Q), _bits(K), _bits(V), heads, scale, want_lse=False)), None


def forward_device(mem, mh, Q, K, V, heads, scale, pad=0, ldl_extra=0, want_lse=True, what=""):
    """hsmh16_forward_device over fresh buffers: input pads NaN, y and lse pre-filled with a sentinel; the pads of both must survive"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv) = (_features_in(mem, a, pad) for a in (Q, K, V))
    ldy, ldl = w + pad, heads + ldl_extra
    dy = _out(mem, mh.num_rows, ldy)
    dl = mem.alloc(np.full((mh.num_rows, ldl), hc.SENTINEL, dtype=np.uint32)) if want_lse else None
    mh.forward_device(dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, heads, w // heads, scale, dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = _features_out(mem, mh, dy, mh.num_rows, w, ldy, what)
    if not want_lse:
        return y, None
    lw = mem.read(mh, dl).reshape(mh.num_rows, ldl)
    assert (lw[:, heads:] == hc.SENTINEL).all(), f"{what}: the pad words of lse were written"
    return y, np.ascontiguousarray(lw[:, :heads]).view(np.float32)


def backward_host(mh, Q, K, V, gY, lse, heads, scale):
    return tuple(mh16.from_bf16(g) for g in mh.backward(_bits(Q), _bits(K), _bits(V), _bits(gY), lse, heads, scale))


def backward_device(mem, mh, Q, K, V, gY, lse, heads, scale, pad=0, ldl_extra=0, what=""):
    """hsmh16_backward_device over fresh buffers: the pads of the inputs (lse among them) NaN, the three outputs pre-filled with a sentinel"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (_features_in(mem, a, pad) for a in (Q, K, V, gY))
    dl, ldl = hc._lse_in(mem, lse, ldl_extra)
    ld = w + pad
    oq, ok, ov = (_out(mem, n, ld) for n in (mh.num_rows, mh.num_cols, mh.num_cols))
    mh.backward_device(dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, heads, w // heads, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld)
    return tuple(_features_out(mem, mh, buf, n, w, ld, f"{what}, {name}") for name, buf, n in (("gq", oq, mh.num_rows), ("gk", ok, mh.num_cols), ("gv", ov, mh.num_cols)))


def all_forward_forms(mem, mh, refs, Q, K, V, heads, scale, pads, extras, what):
    """the host form and the device form at every pad and ldl, each with lse taken and with NULL; returns the lse of the host form"""
    y, lse = forward_host(mh, Q, K, V, heads, scale)
    check_forward(refs, y, lse, f"{what}, host form, lse taken")
    check_forward(refs, forward_host(mh, Q, K, V, heads, scale, False)[0], None, f"{what}, host form, lse NULL")
    for pad in pads:
        for extra in extras:
            for want in (True, False):
                tag = f"{what}, device form, pad {pad}, ldl {heads + extra}, {'lse taken' if want else 'lse NULL'}"
                check_forward(refs, *forward_device(mem, mh, Q, K, V, heads, scale, pad, extra, want, tag), tag)
    return lse


def all_backward_forms(mem, mh, refs, Q, K, V, gY, lse, heads, scale, pads, extras, what):
    worst = check_backward(refs, *backward_host(mh, Q, K, V, gY, lse, heads, scale), f"{what}, host form")
    for pad in pads:
        for extra in extras:
            tag = f"{what}, device form, pad {pad}, ldl {heads + extra}"
            w = check_backward(refs, *backward_device(mem, mh, Q, K, V, gY, lse, heads, scale, pad, extra, tag), tag)
            worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def general(mem, shapes=SHAPES):
    """300 x 517, 4000 entries, every (heads, d) of SHAPES, scale 0.125, 1 and -2, pad 0 and 8 elements, ldl = heads and heads + 3, lse
    taken and NULL, both forms; forward, then backward with the lse the forward just wrote"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with mh16.MultiHeadAttentionBF16((indptr, indices, shape), heads) as mh:
            assert mh.nnz == NNZ and mh.info()["nnz"] == NNZ
            Q, K, V, gY = operands(shape, heads * d, 9100 + 1000 * heads + d)
            scores = head_scores(indptr, indices, Q, K, heads)
            for scale in (0.125, 1.0, -2.0):
                what = f"general, {heads} heads of d {d}, scale {scale}"
                fwd = forward_refs(scores, V, scale)
                print(f"{what}: input condition, largest expm1(eta_r) = {max(float(r.rho[r.finite].max()) for r in fwd):.3g}")
                lse = all_forward_forms(mem, mh, fwd, Q, K, V, heads, scale, (0, 8), (0, 3), what)
                w = all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, scale), Q, K, V, gY, lse, heads, scale, (0, 8), (0, 3), what)
                print(f"{what}: backward worst error / bound = {w['gq']:.3f} (gq), {w['gk']:.3f} (gk), {w['gv']:.3f} (gv)")


def heads_do_not_leak(mem, shapes=((4, 16), (5, 8))):
    """heads_cases.heads_do_not_leak with bf16 operands.  Forward: head 1's elements of some K rows are NaN, of others +inf, and head 1's
    elements of some V rows are NaN; the other heads stay inside the bounds of the CLEAN reference, head 1 follows the special-row table
    through its own reference.  Backward, from clean operands: head 1's lse word of some rows is NaN, of others -inf; the other heads stay
    inside their bounds, head 1 is NaN in gQ of those rows and in gK and gV of the columns they touch."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    n = np.diff(indptr.astype(np.int64))
    of = pc.entry_rows(indptr)
    k_nan, k_inf, v_nan = np.array([3, 77, 200]), np.array([11, 150, 401]), np.array([5, 90, 333, 500])
    r_nan, r_inf = (np.nonzero(n >= 3)[0][[2, 40]], np.nonzero(n >= 3)[0][[7, 90]])
    scale = 0.5
    for heads, d in shapes:
        h1 = slice(d, 2 * d)
        with mh16.MultiHeadAttentionBF16((indptr, indices, shape), heads) as mh:
            Q, K, V, gY = operands(shape, heads * d, 9300 + 1000 * heads + d)
            clean = forward_refs(head_scores(indptr, indices, Q, K, heads), V, scale)
            Kp, Vp = K.copy(), V.copy()
            Kp[k_nan, h1], Kp[k_inf, h1], Vp[v_nan, h1] = np.nan, np.inf, np.nan
            planted = forward_refs(head_scores(indptr, indices, Q, Kp, heads), V, scale)      # head 1: the planted K over the clean V
            assert planted[1].bad.sum() >= 3 and planted[1].finite.sum() > ROWS // 2
            refs = [planted[h] if h == 1 else clean[h] for h in range(heads)]
            touched = np.zeros(ROWS, dtype=bool)
            touched[of[np.isin(indices, v_nan)]] = True
            assert 3 <= touched.sum() < ROWS // 4
            what = f"heads do not leak, forward, {heads} heads of d {d}"
            for y, lse in (forward_host(mh, Q, Kp, Vp, heads, scale), forward_device(mem, mh, Q, Kp, Vp, heads, scale, 8, 1, True, what)):
                assert np.isnan(y[touched, h1]).all(), f"{what}: a row that holds a NaN row of V is not NaN in head 1"
                y = y.copy()
                y[touched, h1] = rounded_forward(refs)[0][touched, h1]      # checked above; the rest of head 1 against its reference
                check_forward(refs, y, lse, what)
                assert np.isfinite(np.delete(y, np.s_[d: 2 * d], axis=1)[n > 0]).all() and np.isfinite(np.delete(lse, 1, axis=1)[n > 0]).all()
            # backward
            scores = head_scores(indptr, indices, Q, K, heads)
            lse = rounded_forward(clean)[1]
            lse[r_nan, 1], lse[r_inf, 1] = np.nan, -np.inf
            brefs = backward_refs(scores, V, gY, lse, scale)
            assert brefs[1].bad_r.sum() == 4 and 4 <= brefs[1].bad_c.sum() < COLS // 4 and not any(r.bad_r.any() for h, r in enumerate(brefs) if h != 1)
            what = f"heads do not leak, backward, {heads} heads of d {d}"
            for g in (backward_host(mh, Q, K, V, gY, lse, heads, scale), backward_device(mem, mh, Q, K, V, gY, lse, heads, scale, 8, 1, what)):
                check_backward(brefs, *g, what)
                for a in g:
                    assert np.isfinite(np.delete(a, np.s_[d: 2 * d], axis=1)).all(), f"{what}: head 1's lse words reached another head"


def edges(mem, heads=3, d=16):
    """every pattern of pattern_cases.edge_patterns() at (3, 16): nnz = 0 ... 7, runs of empty rows, empty columns, one row that holds all
    301 entries, unsorted columns, a pair held twice; rows and columns without entries read 0x0000 (and -inf in lse) bit for bit: the
    references' checks look at the widened words, and 0x0000 is the only element that widens to the word 0"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with mh16.MultiHeadAttentionBF16((indptr, indices, shape), heads) as mh:
            assert mh.nnz == indices.size
            Q, K, V, gY = operands(shape, heads * d, 9500)
            scores = head_scores(indptr, indices, Q, K, heads)
            fwd = forward_refs(scores, V, 1.5)
            assert all(r.empty.sum() == (np.diff(indptr.astype(np.int64)) == 0).sum() for r in fwd)
            lse = all_forward_forms(mem, mh, fwd, Q, K, V, heads, 1.5, (8,), (1,), name)
            assert (lse[fwd[0].empty] == -np.inf).all()
            all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, 1.5), Q, K, V, gY, lse, heads, 1.5, (8,), (1,), name)


def nothing_carried_over(mem):
    """heads, d and the PRECISION changing between calls on one object: (4, 128) bf16, then (5, 4) fp32, then (5, 8) bf16 with another
    scale, then (4, 128) bf16 again gives the bits of the first time, and the calls in between the words of fresh objects (no m, l or D
    word of one call reaches another, whichever precision wrote it)"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with mh16.MultiHeadAttentionBF16((indptr, indices, shape), 8) as mh, mh16.MultiHeadAttentionBF16((indptr, indices, shape), 5) as fresh, \
            mha.MultiHeadAttention((indptr, indices, shape), 5) as fresh32:
        Q, K, V, gY = operands(shape, 512, 9800)
        f1 = forward_device(mem, mh, Q, K, V, 4, 1.0)
        b1 = backward_device(mem, mh, Q, K, V, gY, f1[1], 4, 1.0)
        # fp32, (5, 4), on the same object
        Q2, K2, V2, gY2 = hc.operands(shape, 20, 9810)
        f2 = hc.forward_device(mem, FP32Face(mh), Q2, K2, V2, 5, -0.75, 4, 2)
        b2 = hc.backward_device(mem, FP32Face(mh), Q2, K2, V2, gY2, f2[1], 5, -0.75, 4, 2)
        assert same_words(f2, hc.forward_device(mem, fresh32, Q2, K2, V2, 5, -0.75, 4, 2))
        assert same_words(b2, hc.backward_device(mem, fresh32, Q2, K2, V2, gY2, f2[1], 5, -0.75, 4, 2))
        scores = head_scores(indptr, indices, Q2, K2, 5)
        hc.check_forward(hc.forward_refs(scores, V2, -0.75), *f2, "the fp32 call in between")
        hc.check_backward(hc.backward_refs(scores, V2, gY2, f2[1], -0.75), *b2, "the fp32 call in between")
        # bf16, (5, 8), another scale
        Q3, K3, V3, gY3 = operands(shape, 40, 9820)
        f3 = forward_device(mem, mh, Q3, K3, V3, 5, 0.3, 8, 2)
        b3 = backward_device(mem, mh, Q3, K3, V3, gY3, f3[1], 5, 0.3, 8, 2)
        assert same_words(f3, forward_device(mem, fresh, Q3, K3, V3, 5, 0.3, 8, 2))
        assert same_words(b3, backward_device(mem, fresh, Q3, K3, V3, gY3, f3[1], 5, 0.3, 8, 2))
        scores = head_scores(indptr, indices, Q3, K3, 5)
        check_forward(forward_refs(scores, V3, 0.3), *f3, "third call")
        check_backward(backward_refs(scores, V3, gY3, f3[1], 0.3), *b3, "third call")
        assert same_words(f1, forward_device(mem, mh, Q, K, V, 4, 1.0)) and same_words(f1, forward_host(mh, Q, K, V, 4, 1.0))
        assert same_words(b1, backward_device(mem, mh, Q, K, V, gY, f1[1], 4, 1.0)) and same_words(b1, backward_host(mh, Q, K, V, gY, f1[1], 4, 1.0))


def mixed(mem, heads=4, d=32):
    """a forward in one precision, the backward in the other, on one object: the fp32 forward's lse (over the widened operands) fed to the
    bf16 backward, and the bf16 forward's lse fed to the fp32 backward; every gradient inside the bounds computed from the lse words given"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 6)
    shape = (ROWS, COLS)
    with mh16.MultiHeadAttentionBF16((indptr, indices, shape), heads) as mh:
        Q, K, V, gY = operands(shape, heads * d, 9900)
        scores = head_scores(indptr, indices, Q, K, heads)
        y32, lse32 = hc.forward_device(mem, FP32Face(mh), Q, K, V, heads, 0.25, 4, 1)
        hc.check_forward(hc.forward_refs(scores, V, 0.25), y32, lse32, "mixed, fp32 forward")
        check_backward(backward_refs(scores, V, gY, lse32, 0.25), *backward_device(mem, mh, Q, K, V, gY, lse32, heads, 0.25, 8, 1, "mixed"), "mixed, bf16 backward from the fp32 lse")
        y16, lse16 = forward_device(mem, mh, Q, K, V, heads, 0.25, 8, 1)
        check_forward(forward_refs(scores, V, 0.25), y16, lse16, "mixed, bf16 forward")
        hc.check_backward(hc.backward_refs(scores, V, gY, lse16, 0.25), *hc.backward_device(mem, FP32Face(mh), Q, K, V, gY, lse16, heads, 0.25, 4, 1, "mixed"),
                          "mixed, fp32 backward from the bf16 lse")


def large(mem, shape, indptr, indices, heads, d, seed, what):
    """the device forms over one large pattern, forward then backward with the lse just written, every word of every head inside its bound
    (float64 sums as the references); returns the two lists of references"""
    Q, K, V, gY = operands(shape, heads * d, seed)
    scores = head_scores(indptr, indices, Q, K, heads, exact=False)
    fwd = forward_refs(scores, V, 0.5)
    with mh16.MultiHeadAttentionBF16((indptr, indices, shape), heads) as mh:
        y, lse = forward_device(mem, mh, Q, K, V, heads, 0.5, 8, 1, True, what)
        check_forward(fwd, y, lse, what)
        bwd = backward_refs(scores, V, gY, lse, 0.5)
        check_backward(bwd, *backward_device(mem, mh, Q, K, V, gY, lse, heads, 0.5, 8, 1, what), what)
    return fwd, bwd


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
FEATURES = hc.FEATURES
FORWARD = hc.FORWARD


def refusals(mem):
    """every rule of the header's SHAPES ACCEPTED and LAYOUT paragraphs through the four calls: HS_ERR_BAD_ARG with a message, and after
    each refusal the bf16 calls AND the fp32 calls of the object still give their bits"""
    l = mh16.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    one = np.zeros(8, dtype=np.uint16).ctypes.data
    assert l.hsmh16_forward_device(None, vp(one), 8, vp(one), 8, vp(one), 8, 1, 8, 1.0, vp(one), 8, None, 1) == BAD_ARG
    assert l.hsmh16_forward(None, vp(one), vp(one), vp(one), 1, 8, 1.0, vp(one), None) == BAD_ARG
    assert l.hsmh16_backward_device(None, vp(one), 8, vp(one), 8, vp(one), 8, vp(one), 8, vp(one), 1, 1, 8, 1.0, vp(one), 8, vp(one), 8, vp(one), 8) == BAD_ARG
    assert l.hsmh16_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), 1, 8, 1.0, vp(one), vp(one), vp(one)) == BAD_ARG

    heads, d = 2, 8
    w = heads * d
    with mh16.MultiHeadAttentionBF16((indptr, indices, shape), 4) as mh, mh16.MultiHeadAttentionBF16((indptr, indices, shape), 4, backward=False) as fwd_only:
        Q, K, V, gY = operands(shape, w, 9950)
        want_y, want_l = forward_host(mh, Q, K, V, heads, 0.5)
        scores = head_scores(indptr, indices, Q, K, heads)
        check_forward(forward_refs(scores, V, 0.5), want_y, want_l, "refusals")
        want_g = backward_host(mh, Q, K, V, gY, want_l, heads, 0.5)
        check_backward(backward_refs(scores, V, gY, want_l, 0.5), *want_g, "refusals")
        # the fp32 calls of the same objects, (2, 4)
        Q32, K32, V32, gY32 = hc.operands(shape, 8, 9960)
        want32 = {}
        for obj in (mh, fwd_only):
            want32[obj] = hc.forward_host(FP32Face(obj), Q32, K32, V32, 2, 0.5)
        want_g32 = hc.backward_host(FP32Face(mh), Q32, K32, V32, gY32, want32[mh][1], 2, 0.5)

        def still_usable(rc, what, obj=mh):
            assert rc == BAD_ARG and l.hsmh_last_error(obj._h), (what, rc)
            assert same_words(forward_host(obj, Q, K, V, heads, 0.5), (want_y, want_l)), f"unusable after {what}"
            assert same_words(hc.forward_host(FP32Face(obj), Q32, K32, V32, 2, 0.5), want32[obj]), f"the fp32 forward differs after {what}"
            if obj is mh:
                assert same_words(backward_host(mh, Q, K, V, gY, want_l, heads, 0.5), want_g), f"unusable after {what}"
                assert same_words(hc.backward_host(FP32Face(mh), Q32, K32, V32, gY32, want32[mh][1], 2, 0.5), want_g32), f"the fp32 backward differs after {what}"

        def forward_call(a, obj=mh):
            return l.hsmh16_forward_device(obj._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], a["heads"], a["d"], a["scale"], vp(a["y"]), a["ldy"], vp(a["lse"]),
                                           a["ldl"])

        def backward_call(a, obj=mh):
            return l.hsmh16_backward_device(obj._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["ldl"], a["heads"], a["d"],
                                            a["scale"], vp(a["gq"]), a["ldgq"], vp(a["gk"]), a["ldgk"], vp(a["gv"]), a["ldgv"])

        # buffers of 9 rows x 32 elements (64 bytes a row, ld up to 32), 16-byte aligned; lse: 6 rows of up to 4 words.  With ld = 16 elements
        # a row is 32 bytes, as a row of heads_cases.refusals is (8 words), so the overlap pairs below are that file's, byte for byte
        names = FEATURES + ("y", "lse")
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 16 for name in FEATURES + ("y",)}, heads=heads, d=d, scale=1.0, ldl=2)
        assert forward_call(ok) == 0 and backward_call(ok) == 0
        q, k, v, gy, y, ls, gq, gk = (ok[n] for n in ("q", "k", "v", "gy", "y", "lse", "gq", "gk"))
        nan, inf = float("nan"), float("inf")
        wide_ld = lambda names_, ld: {"ld" + n: ld for n in names_}      # noqa: E731
        # SHAPES ACCEPTED (the object's max_heads is 4), scale, lse: the rules both calls share
        shared = [("d = 0", dict(d=0)), ("d = 4", dict(d=4)), ("d = 12", dict(heads=1, d=12)), ("d = 24", dict(heads=1, d=24)), ("d = 512", dict(heads=1, d=512)),
                  ("d = 2^31", dict(heads=1, d=2 ** 31)), ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5, d=8)), ("heads * d = 1024", dict(heads=4, d=256)),
                  ("heads * d = 768", dict(heads=3, d=256)), ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf)), ("scale -inf", dict(scale=-inf)),
                  ("misaligned lse", dict(lse=ls + 2)), ("ldl < heads", dict(ldl=1)), ("ldl = 0", dict(ldl=0))]
        for what, change in shared:
            if "heads * d" in what or "d = 512" in what or "2^31" in what:
                change = dict(wide_ld(FEATURES + ("y",), 1024), **change)
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        fcases = [("y is q", dict(y=q)), ("y inside k", dict(y=k + 16 * 4)), ("y is v", dict(y=v)), ("y's last row in v", dict(v=q + 16, y=q + 16 + 8 * 8 * 4)),
                  ("lse inside y", dict(lse=y + 4 * 4)), ("y over the last lse word", dict(y=ls + 32)), ("lse inside q", dict(lse=q + 8))]
        for name in FORWARD:
            ptr, ld = ok[name], "ld" + name
            fcases += [(f"null {name}", {name: None}), (f"misaligned {name} by 2", {name: ptr + 2}), (f"misaligned {name} by 4", {name: ptr + 4}),
                       (f"misaligned {name} by 8", {name: ptr + 8}), (f"{ld} % 8", {ld: 20}), (f"{ld} < heads * d", {ld: 8})]
        for what, change in fcases:
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("null lse", dict(lse=None)), ("gq is q", dict(gq=q)), ("gk inside k", dict(gk=k + 16 * 4)), ("gv is v", dict(gv=v)), ("gq is gy", dict(gq=gy)), ("gk is q", dict(gk=q)),
                  ("gv is gk", dict(gv=gk)), ("gk is gq", dict(gk=gq)), ("gv's first row in gq's last", dict(gv=gq + 5 * 8 * 4)), ("gq is lse", dict(gq=ls)),
                  ("gv over the last lse word", dict(gv=ls + 32)), ("gq's last row in v", dict(v=q + 16, gq=q + 16 + 8 * 8 * 4))]
        for name in FEATURES:
            ptr, ld = ok[name], "ld" + name
            bcases += [(f"null {name}", {name: None}), (f"misaligned {name} by 2", {name: ptr + 2}), (f"misaligned {name} by 4", {name: ptr + 4}),
                       (f"misaligned {name} by 8", {name: ptr + 8}), (f"{ld} % 8", {ld: 20}), (f"{ld} < heads * d", {ld: 8})]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        # the host forms
        host = {name: np.zeros(9 * 16, np.uint16) for name in names}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, heads=heads, d=d, scale=1.0)

        def forward_host_call(a, obj=mh):
            return l.hsmh16_forward(obj._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), a["heads"], a["d"], a["scale"], vp(a["y"]), vp(a["lse"]))

        def backward_host_call(a, obj=mh):
            return l.hsmh16_backward(obj._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), a["heads"], a["d"], a["scale"], vp(a["gq"]), vp(a["gk"]), vp(a["gv"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0
        both = [("d = 0", dict(d=0)), ("d = 4", dict(d=4)), ("d = 12", dict(d=12)), ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5)),
                ("heads * d = 1024", dict(heads=4, d=256)), ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf))]
        for what, change in both + [(f"null {n}", {n: None}) for n in FORWARD] + [("y is k", dict(y=okh["k"])), ("lse inside y", dict(lse=okh["y"] + 8))]:
            still_usable(forward_host_call(dict(okh, **change)), "forward: " + what)
        for what, change in both + [(f"null {n}", {n: None}) for n in FEATURES + ("lse",)] + [("gk is k", dict(gk=okh["k"])), ("gq is gk", dict(gq=okh["gk"])),
                                                                                             ("gv inside lse", dict(gv=okh["lse"] + 8)), ("gq inside gy", dict(gq=okh["gy"] + 8))]:
            still_usable(backward_host_call(dict(okh, **change)), "backward: " + what)
        # backward on an object created without HSMH_BACKWARD: refused in both forms, and the forward of that object still runs
        still_usable(backward_call(ok, fwd_only), "backward_device without HSMH_BACKWARD", fwd_only)
        still_usable(backward_host_call(okh, fwd_only), "backward without HSMH_BACKWARD", fwd_only)
        assert b"HSMH_BACKWARD" in l.hsmh_last_error(fwd_only._h)
        assert forward_call(ok, fwd_only) == 0
        # a refused shape names the rule and points to the fp32 calls
        assert forward_call(dict(ok, d=4)) == BAD_ARG
        msg = l.hsmh_last_error(mh._h).decode()
        assert "8, 16, 32, 64, 128, 256" in msg and "hsmh_forward_device" in msg and "hsmh_backward_device" in msg, msg
        assert forward_call(dict(ok, heads=4, d=256, **wide_ld(FEATURES + ("y",), 1024))) == BAD_ARG
        msg = l.hsmh_last_error(mh._h).decode()
        assert "at most 512" in msg and "hsmh_forward_device" in msg, msg
        # ranges that touch without sharing a byte are fine: lse right behind y's 6 rows, gv right behind the 9 rows of gk, gq right behind lse's 6 rows; a NULL lse
        assert forward_call(dict(ok, lse=y + (5 * 16 + 16) * 2)) == 0
        assert forward_call(dict(ok, lse=None, ldl=0)) == 0
        assert backward_call(dict(ok, gv=gk + (8 * 16 + 16) * 2)) == 0
        assert backward_call(dict(ok, gq=ls + 48)) == 0
        for obj in (mh, fwd_only):
            obj.set_stream(None)
            obj.sync()
