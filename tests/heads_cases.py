"""The cases of the multi-head attention object (include/hisparse_heads.h), shared by tests/test_heads_cpu.py (libhisparse_cpu.so, in a
child process) and tests/test_gpu_heads.py (the HIP library, on the device), written against the memory interface of
tests/pattern_cases.py.

The reference is the project's own, per head: head h of a call is columns h d ... h d + d - 1 of every feature operand and column h of
lse, and it is held to attention_cases.Reference (forward: every word of Y and of lse) and to attention_backward_cases.Reference
(backward: every word of gQ, gK and gV, from the lse words AS GIVEN to the call) with their bounds unchanged.  No tolerance is
introduced here.  Both references assert their input condition (rho <= 2^-12) themselves.  exact=False (float64 sums, the 2^-52 terms
doubled) is used by the large cases of the GPU tests only, as in the two single-head case files."""
import ctypes as C

import numpy as np

from hisparse_amd import attention, attention_backward, heads as mha

import attention_backward_cases as bc
import attention_cases as ac
import pattern_cases as pc
import wide_cases as wc
from pattern_cases import HipMemory, HostMemory, edge_patterns, random_pattern  # noqa: F401

BAD_ARG, BAD_MATRIX = -1, -4
SENTINEL, NAN_WORD = wc.SENTINEL, wc.NAN_WORD
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
# head widths of 1, 2, 4, 8, ... lanes, both sides of the weight-dealing switch (d = 16), dead lanes ((5, 4), (3, 8), (3, 16)), the widest group
SHAPES = ((1, 4), (2, 4), (5, 4), (3, 8), (4, 16), (3, 16), (2, 32), (4, 64), (2, 128), (1, 256), (8, 32), (64, 4))


# ---- the per-head references ---------------------------------------------------------------------------------------------------------
def cut(a, h, d):
    """head h's d columns of a feature array, contiguous"""
    return np.ascontiguousarray(a[:, h * d: (h + 1) * d])


def head_scores(indptr, indices, Q, K, heads, exact=True):
    """what depends on the pattern, Q and K alone, per head"""
    d = Q.shape[1] // heads
    assert Q.shape[1] == K.shape[1] == heads * d
    return [bc.scores_of(indptr, indices, cut(Q, h, d), cut(K, h, d), exact) for h in range(heads)]


def forward_refs(scores, V, scale):
    d = V.shape[1] // len(scores)
    return [ac.Reference(s, cut(V, h, d), scale) for h, s in enumerate(scores)]


def backward_refs(scores, V, gY, lse, scale):
    """lse: (rows, heads) float32, the words the backward call is given"""
    d = V.shape[1] // len(scores)
    lse = np.asarray(lse, dtype=np.float32)
    assert lse.shape == (scores[0].indptr.size - 1, len(scores))
    return [bc.Reference(s, cut(V, h, d), cut(gY, h, d), np.ascontiguousarray(lse[:, h]), scale) for h, s in enumerate(scores)]


def check_forward(refs, y, lse, what):
    """every word of every head of y (rows x heads d) and, unless None, of lse (rows x heads); the largest error / bound seen"""
    y = np.asarray(y, dtype=np.float32)
    d = refs[0].d
    assert y.shape == (refs[0].Y.shape[0], len(refs) * d), (what, y.shape)
    if lse is not None:
        lse = np.asarray(lse, dtype=np.float32)
        assert lse.shape == (y.shape[0], len(refs)), (what, lse.shape)
    return max(r.check(cut(y, h, d), None if lse is None else np.ascontiguousarray(lse[:, h]), f"{what}, head {h}") for h, r in enumerate(refs))


def check_backward(refs, gq, gk, gv, what):
    d = refs[0].d
    worst = dict.fromkeys(bc.OUTPUTS, 0.0)
    for got, n in ((gq, refs[0].GQ.shape[0]), (gk, refs[0].GK.shape[0]), (gv, refs[0].GV.shape[0])):
        assert np.asarray(got).shape == (n, len(refs) * d), (what, np.asarray(got).shape)
    for h, r in enumerate(refs):
        w = r.check(cut(gq, h, d), cut(gk, h, d), cut(gv, h, d), f"{what}, head {h}")
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


def rounded_forward(refs):
    """a correct forward result: the references' own words rounded once, (y (rows, heads d), lse (rows, heads))"""
    parts = [r.rounded() for r in refs]
    return np.concatenate([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)


def rounded_backward(refs, grads=None):
    parts = [r.rounded(None if grads is None else grads[h]) for h, r in enumerate(refs)]
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(3))


# ---- inputs and the forms ------------------------------------------------------------------------------------------------------------
def operands(shape, width, seed):
    """Q, K, V, gY of `width` = heads * d words per row"""
    return bc.operands(shape, width, seed)


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_words(a, b):
    return all(np.array_equal(words(x), words(y)) for x, y in zip(a, b))


def forward_host(mh, Q, K, V, heads, scale, want_lse=True):
    """(y, lse or None)"""
    if want_lse:
        return mh.forward(Q, K, V, heads, scale)
    return mh.forward(Q, K, V, heads, scale, want_lse=False), None


def forward_device(mem, mh, Q, K, V, heads, scale, pad=0, ldl_extra=0, want_lse=True, what=""):
    """hsmh_forward_device over fresh buffers: input pads NaN, y and lse pre-filled with a sentinel; the pad words of both must survive"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv) = (wc._features_in(mem, a, pad) for a in (Q, K, V))
    ldy, ldl = w + pad, heads + ldl_extra
    dy = mem.alloc(np.full((mh.num_rows, ldy), SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full((mh.num_rows, ldl), SENTINEL, dtype=np.uint32)) if want_lse else None
    mh.forward_device(dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, heads, w // heads, scale, dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = wc._features_out(mem, mh, dy, mh.num_rows, w, ldy, what)
    if not want_lse:
        return y, None
    lw = mem.read(mh, dl).reshape(mh.num_rows, ldl)
    assert (lw[:, heads:] == SENTINEL).all(), f"{what}: the pad words of lse were written"
    return y, np.ascontiguousarray(lw[:, :heads]).view(np.float32)


def _lse_in(mem, lse, ldl_extra):
    """lse (rows, heads) on the device in rows of heads + ldl_extra words, the pad words NaN"""
    lse = np.ascontiguousarray(lse, dtype=np.float32)
    buf = np.full((lse.shape[0], lse.shape[1] + ldl_extra), NAN_WORD, dtype=np.uint32)
    buf[:, : lse.shape[1]] = lse.view(np.uint32)
    return mem.alloc(buf), lse.shape[1] + ldl_extra


def backward_host(mh, Q, K, V, gY, lse, heads, scale):
    return mh.backward(Q, K, V, gY, lse, heads, scale)


def backward_device(mem, mh, Q, K, V, gY, lse, heads, scale, pad=0, ldl_extra=0, what=""):
    """hsmh_backward_device over fresh buffers: the pads of the inputs (lse among them) NaN, the three outputs pre-filled with a sentinel"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (wc._features_in(mem, a, pad) for a in (Q, K, V, gY))
    dl, ldl = _lse_in(mem, lse, ldl_extra)
    ld = w + pad
    oq = mem.alloc(np.full((mh.num_rows, ld), SENTINEL, dtype=np.uint32))
    ok, ov = (mem.alloc(np.full((mh.num_cols, ld), SENTINEL, dtype=np.uint32)) for _ in range(2))
    mh.backward_device(dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, heads, w // heads, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld)
    return tuple(wc._features_out(mem, mh, buf, n, w, ld, f"{what}, {name}") for name, buf, n in (("gq", oq, mh.num_rows), ("gk", ok, mh.num_cols), ("gv", ov, mh.num_cols)))


def all_forward_forms(mem, mh, refs, Q, K, V, heads, scale, pads, extras, what):
    """the host form and the device form at every pad and ldl, each with lse taken and with NULL, inside the bounds of one set of
    references; returns the lse of the host form"""
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
    """300 x 517, 4000 entries, every (heads, d) of SHAPES, scale 0.125, 1 and -2, pad 0 and 8, ldl = heads and heads + 3, lse taken and
    NULL, both forms; forward, then backward with the lse the forward just wrote"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with mha.MultiHeadAttention((indptr, indices, shape), heads) as mh:
            assert mh.nnz == NNZ and mh.info()["nnz"] == NNZ
            Q, K, V, gY = operands(shape, heads * d, 6100 + 1000 * heads + d)
            scores = head_scores(indptr, indices, Q, K, heads)
            for scale in (0.125, 1.0, -2.0):
                what = f"general, {heads} heads of d {d}, scale {scale}"
                lse = all_forward_forms(mem, mh, forward_refs(scores, V, scale), Q, K, V, heads, scale, (0, 8), (0, 3), what)
                w = all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, scale), Q, K, V, gY, lse, heads, scale, (0, 8), (0, 3), what)
                print(f"{what}: backward worst error / bound = {w['gq']:.3f} (gq), {w['gk']:.3f} (gk), {w['gv']:.3f} (gv)")


def heads_do_not_leak(mem, shapes=((4, 16), (5, 4))):
    """Forward: head 1's words of some K rows are NaN, of others +inf, and head 1's words of some V rows are NaN.  Heads 0, 2, ... stay
    inside their bounds of the CLEAN reference (the same operands without the planted words); head 1 follows the special-row table of
    hisparse_attention.h through its own reference (built from the planted K), and every row that holds a column whose V row is NaN is
    NaN in all of head 1's words of Y (a weight, zero or not, times NaN) while its lse word stays inside its bound.
    Backward, from clean operands: head 1's lse word of some rows is NaN, of others -inf.  Heads 0, 2, ... stay inside the bounds of their
    references; head 1 is NaN in gQ of those rows and in gK and gV of the columns they touch (attention_backward_cases.Reference.check)."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    n = np.diff(indptr.astype(np.int64))
    of = pc.entry_rows(indptr)
    k_nan, k_inf, v_nan = np.array([3, 77, 200]), np.array([11, 150, 401]), np.array([5, 90, 333, 500])
    r_nan, r_inf = (np.nonzero(n >= 3)[0][[2, 40]], np.nonzero(n >= 3)[0][[7, 90]])
    scale = 0.5
    for heads, d in shapes:
        h1 = slice(d, 2 * d)
        with mha.MultiHeadAttention((indptr, indices, shape), heads) as mh:
            Q, K, V, gY = operands(shape, heads * d, 6300 + 1000 * heads + d)
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
            for y, lse in (forward_host(mh, Q, Kp, Vp, heads, scale), forward_device(mem, mh, Q, Kp, Vp, heads, scale, 4, 1, True, what)):
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
            for g in (backward_host(mh, Q, K, V, gY, lse, heads, scale), backward_device(mem, mh, Q, K, V, gY, lse, heads, scale, 4, 1, what)):
                check_backward(brefs, *g, what)
                for a in g:
                    assert np.isfinite(np.delete(a, np.s_[d: 2 * d], axis=1)).all(), f"{what}: head 1's lse words reached another head"


def edges(mem, heads=3, d=8):
    """every pattern of pattern_cases.edge_patterns() at (3, 8): nnz = 0 ... 7, runs of empty rows, empty columns, one row that holds all
    301 entries, unsorted columns, a pair held twice; rows and columns without entries read +0.0 (and -inf in lse) bit for bit"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with mha.MultiHeadAttention((indptr, indices, shape), heads) as mh:
            assert mh.nnz == indices.size
            Q, K, V, gY = operands(shape, heads * d, 6500)
            scores = head_scores(indptr, indices, Q, K, heads)
            fwd = forward_refs(scores, V, 1.5)
            assert all(r.empty.sum() == (np.diff(indptr.astype(np.int64)) == 0).sum() for r in fwd)
            lse = all_forward_forms(mem, mh, fwd, Q, K, V, heads, 1.5, (8,), (1,), name)
            assert (lse[fwd[0].empty] == -np.inf).all()
            all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, 1.5), Q, K, V, gY, lse, heads, 1.5, (8,), (1,), name)


def agreement(mem, heads=4, d=16):
    """(4, 16) on the general pattern: `heads` calls of hsat_forward and hsab_backward over the heads' slices (lse column h made
    contiguous) and the one call of this object lie inside the same per-head bounds"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    Q, K, V, gY = operands(shape, heads * d, 6600)
    scores = head_scores(indptr, indices, Q, K, heads)
    fwd = forward_refs(scores, V, 0.25)
    with mha.MultiHeadAttention((indptr, indices, shape), heads) as mh, attention.PatternAttention((indptr, indices, shape)) as pa, \
            attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        y, lse = forward_host(mh, Q, K, V, heads, 0.25)
        check_forward(fwd, y, lse, "agreement, one call")
        per = [pa.forward(cut(Q, h, d), cut(K, h, d), cut(V, h, d), 0.25) for h in range(heads)]
        check_forward(fwd, np.concatenate([p[0] for p in per], axis=1), np.stack([p[1] for p in per], axis=1), "agreement, per-head calls")
        bwd = backward_refs(scores, V, gY, lse, 0.25)
        check_backward(bwd, *backward_host(mh, Q, K, V, gY, lse, heads, 0.25), "agreement, one call")
        per = [pb.backward(cut(Q, h, d), cut(K, h, d), cut(V, h, d), cut(gY, h, d), np.ascontiguousarray(lse[:, h]), 0.25) for h in range(heads)]
        check_backward(bwd, *(np.concatenate([p[i] for p in per], axis=1) for i in range(3)), "agreement, per-head calls")


def nothing_carried_over(mem):
    """heads and d changing between calls on one object: (4, 64), then (5, 4) with another scale, then (4, 64) again gives the bits of the
    first time, and the second call the words of a fresh object (no m, l or D word of one call reaches another)"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with mha.MultiHeadAttention((indptr, indices, shape), 8) as mh, mha.MultiHeadAttention((indptr, indices, shape), 5) as fresh:
        Q, K, V, gY = operands(shape, 256, 6800)
        f1 = forward_device(mem, mh, Q, K, V, 4, 1.0)
        b1 = backward_device(mem, mh, Q, K, V, gY, f1[1], 4, 1.0)
        Q2, K2, V2, gY2 = operands(shape, 20, 6810)
        f2 = forward_device(mem, mh, Q2, K2, V2, 5, -0.75, 4, 2)
        b2 = backward_device(mem, mh, Q2, K2, V2, gY2, f2[1], 5, -0.75, 4, 2)
        assert same_words(f2, forward_device(mem, fresh, Q2, K2, V2, 5, -0.75, 4, 2))
        assert same_words(b2, backward_device(mem, fresh, Q2, K2, V2, gY2, f2[1], 5, -0.75, 4, 2))
        scores = head_scores(indptr, indices, Q2, K2, 5)
        check_forward(forward_refs(scores, V2, -0.75), *f2, "second call")
        check_backward(backward_refs(scores, V2, gY2, f2[1], -0.75), *b2, "second call")
        assert same_words(f1, forward_device(mem, mh, Q, K, V, 4, 1.0)) and same_words(f1, forward_host(mh, Q, K, V, 4, 1.0))
        assert same_words(b1, backward_device(mem, mh, Q, K, V, gY, f1[1], 4, 1.0)) and same_words(b1, backward_host(mh, Q, K, V, gY, f1[1], 4, 1.0))


def large(mem, shape, indptr, indices, heads, d, seed, what):
    """the device forms over one large pattern, forward then backward with the lse just written, every word of every head inside its bound
    (float64 sums as the references); returns the two lists of references"""
    Q, K, V, gY = operands(shape, heads * d, seed)
    scores = head_scores(indptr, indices, Q, K, heads, exact=False)
    fwd = forward_refs(scores, V, 0.5)
    with mha.MultiHeadAttention((indptr, indices, shape), heads) as mh:
        y, lse = forward_device(mem, mh, Q, K, V, heads, 0.5, 4, 1, True, what)
        check_forward(fwd, y, lse, what)
        bwd = backward_refs(scores, V, gY, lse, 0.5)
        check_backward(bwd, *backward_device(mem, mh, Q, K, V, gY, lse, heads, 0.5, 4, 1, what), what)
    return fwd, bwd


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _create(rows, cols, indptr, indices, max_heads=4, flags=1):
    l = mha.lib()
    h = C.c_void_p(0xBAD)
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint32)
    indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    rc = l.hsmh_create(C.byref(h), 0, rows, cols, None if indptr is None else indptr.ctypes.data, None if indices is None else indices.ctypes.data, max_heads, flags)
    return rc, h


FEATURES = ("q", "k", "v", "gy", "gq", "gk", "gv")
FORWARD = ("q", "k", "v", "y")


def refusals(mem):
    l = mha.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    bad_index = indices.copy()
    bad_index[3] = 9
    down = np.array([0, 3, 2, 4, 5, 6, 7], dtype=np.uint32)
    shifted = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
    for what, args, code in (("null indptr", (6, 9, None, indices), BAD_ARG), ("null indices", (6, 9, indptr, None), BAD_ARG), ("no rows", (0, 9, indptr, indices), BAD_ARG),
                             ("no columns", (6, 0, indptr, indices), BAD_ARG), ("index = num_cols", (6, 9, indptr, bad_index), BAD_MATRIX),
                             ("indptr decreases", (6, 9, down, indices), BAD_MATRIX), ("indptr[0] = 1", (6, 9, shifted, indices), BAD_MATRIX),
                             ("max_heads = 0", (6, 9, indptr, indices, 0), BAD_ARG), ("max_heads = 65", (6, 9, indptr, indices, 65), BAD_ARG),
                             ("flags = 2", (6, 9, indptr, indices, 4, 2), BAD_ARG), ("flags = 3", (6, 9, indptr, indices, 4, 3), BAD_ARG),
                             ("flags = 2^31", (6, 9, indptr, indices, 4, 2 ** 31), BAD_ARG)):
        rc, h = _create(*args)
        assert rc == code and not h.value and l.hsmh_last_error(None), (what, rc, h.value)
    assert l.hsmh_create(None, 0, 6, 9, indptr.ctypes.data, indices.ctypes.data, 4, 1) == BAD_ARG and l.hsmh_last_error(None)
    for max_heads in (1, 64):      # the ends of the range are fine
        rc, h = _create(6, 9, indptr, indices, max_heads, 0)
        assert rc == 0 and h.value and l.hsmh_destroy(h) == 0
    # null-object calls
    one = np.zeros(4, dtype=np.float32).ctypes.data
    assert l.hsmh_info(None, None, None) == BAD_ARG and l.hsmh_sync(None) == BAD_ARG and l.hsmh_set_stream(None, None) == BAD_ARG
    assert l.hsmh_forward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, 1, 4, 1.0, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsmh_forward(None, vp(one), vp(one), vp(one), 1, 4, 1.0, vp(one), None) == BAD_ARG
    assert l.hsmh_backward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 1, 1, 4, 1.0, vp(one), 4, vp(one), 4, vp(one), 4) == BAD_ARG
    assert l.hsmh_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), 1, 4, 1.0, vp(one), vp(one), vp(one)) == BAD_ARG
    assert l.hsmh_destroy(None) == 0

    heads, d = 2, 4
    w = heads * d
    with mha.MultiHeadAttention((indptr, indices, shape), 4) as mh, mha.MultiHeadAttention((indptr, indices, shape), 4, backward=False) as fwd_only:
        Q, K, V, gY = operands(shape, w, 6900)
        want_y, want_l = forward_host(mh, Q, K, V, heads, 0.5)
        scores = head_scores(indptr, indices, Q, K, heads)
        check_forward(forward_refs(scores, V, 0.5), want_y, want_l, "refusals")
        want_g = backward_host(mh, Q, K, V, gY, want_l, heads, 0.5)
        check_backward(backward_refs(scores, V, gY, want_l, 0.5), *want_g, "refusals")

        def still_usable(rc, what, obj=mh):
            assert rc == BAD_ARG and l.hsmh_last_error(obj._h), (what, rc)
            assert same_words(forward_host(obj, Q, K, V, heads, 0.5), (want_y, want_l)), f"unusable after {what}"
            if obj is mh:
                assert same_words(backward_host(mh, Q, K, V, gY, want_l, heads, 0.5), want_g), f"unusable after {what}"

        def forward_call(a, obj=mh):
            return l.hsmh_forward_device(obj._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], a["heads"], a["d"], a["scale"], vp(a["y"]), a["ldy"], vp(a["lse"]),
                                         a["ldl"])

        def backward_call(a, obj=mh):
            return l.hsmh_backward_device(obj._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["ldl"], a["heads"], a["d"],
                                          a["scale"], vp(a["gq"]), a["ldgq"], vp(a["gk"]), a["ldgk"], vp(a["gv"]), a["ldgv"])

        # buffers of 9 rows x 16 words (the larger dimension, ld up to 16), 16-byte aligned; lse: 6 rows of up to 4 words
        names = FEATURES + ("y", "lse")
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 8 for name in FEATURES + ("y",)}, heads=heads, d=d, scale=1.0, ldl=2)
        assert forward_call(ok) == 0 and backward_call(ok) == 0
        q, k, v, gy, y, ls, gq, gk = (ok[n] for n in ("q", "k", "v", "gy", "y", "lse", "gq", "gk"))
        nan, inf = float("nan"), float("inf")
        wide_ld = lambda names_, ld: {"ld" + n: ld for n in names_}      # noqa: E731
        # SHAPES ACCEPTED (the object's max_heads is 4), scale, lse: the rules both calls share
        shared = [("d = 0", dict(d=0)), ("d = 1", dict(d=1)), ("d = 2", dict(d=2)), ("d = 3", dict(d=3)), ("d = 5", dict(heads=1, d=5)), ("d = 12", dict(heads=1, d=12)),
                  ("d = 24", dict(heads=1, d=24)), ("d = 512", dict(heads=1, d=512)), ("d = 2^31", dict(heads=1, d=2 ** 31)), ("heads = 0", dict(heads=0)),
                  ("heads > max_heads", dict(heads=5, d=4)), ("heads * d = 512", dict(heads=4, d=128)), ("heads * d = 512 at d = 256", dict(heads=2, d=256)),
                  ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf)), ("scale -inf", dict(scale=-inf)), ("misaligned lse", dict(lse=ls + 2)), ("ldl < heads", dict(ldl=1)),
                  ("ldl = 0", dict(ldl=0))]
        for what, change in shared:
            if "heads * d" in what or "d = 512" in what or "2^31" in what:
                change = dict(wide_ld(FEATURES + ("y",), 512), **change)
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        fcases = [("y is q", dict(y=q)), ("y inside k", dict(y=k + 16 * 4)), ("y is v", dict(y=v)), ("y's last row in v", dict(v=q + 16, y=q + 16 + 8 * 8 * 4)),
                  ("lse inside y", dict(lse=y + 4 * 4)), ("y over the last lse word", dict(y=ls + 32)), ("lse inside q", dict(lse=q + 8))]
        for name in FORWARD:
            ptr, ld = ok[name], "ld" + name
            fcases += [(f"null {name}", {name: None}), (f"misaligned {name}", {name: ptr + 4}), (f"misaligned {name} by 8", {name: ptr + 8}), (f"{ld} % 4", {ld: 10}),
                       (f"{ld} < heads * d", {ld: 4})]
        for what, change in fcases:
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("null lse", dict(lse=None)), ("gq is q", dict(gq=q)), ("gk inside k", dict(gk=k + 16 * 4)), ("gv is v", dict(gv=v)), ("gq is gy", dict(gq=gy)), ("gk is q", dict(gk=q)),
                  ("gv is gk", dict(gv=gk)), ("gk is gq", dict(gk=gq)), ("gv's first row in gq's last", dict(gv=gq + 5 * 8 * 4)), ("gq is lse", dict(gq=ls)),
                  ("gv over the last lse word", dict(gv=ls + 32)), ("gq's last row in v", dict(v=q + 16, gq=q + 16 + 8 * 8 * 4))]
        for name in FEATURES:
            ptr, ld = ok[name], "ld" + name
            bcases += [(f"null {name}", {name: None}), (f"misaligned {name}", {name: ptr + 4}), (f"misaligned {name} by 8", {name: ptr + 8}), (f"{ld} % 4", {ld: 10}),
                       (f"{ld} < heads * d", {ld: 4})]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        # the host forms
        host = {name: np.zeros(9 * 8, np.float32) for name in names}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, heads=heads, d=d, scale=1.0)

        def forward_host_call(a, obj=mh):
            return l.hsmh_forward(obj._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), a["heads"], a["d"], a["scale"], vp(a["y"]), vp(a["lse"]))

        def backward_host_call(a, obj=mh):
            return l.hsmh_backward(obj._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), a["heads"], a["d"], a["scale"], vp(a["gq"]), vp(a["gk"]), vp(a["gv"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0
        both = [("d = 0", dict(d=0)), ("d = 6", dict(d=6)), ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5)), ("heads * d = 512", dict(heads=4, d=128)),
                ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf))]
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
        # a refused shape names the rule and points to the per-head calls
        assert forward_call(dict(ok, d=5)) == BAD_ARG
        msg = l.hsmh_last_error(mh._h).decode()
        assert "4, 8, 16, 32, 64, 128, 256" in msg and "hsat_forward_device" in msg and "hsab_backward_device" in msg, msg
        # ranges that touch without sharing a byte are fine: lse right behind y's 6 rows, gv right behind the 9 rows of gk, gq right behind lse's 6 rows; a NULL lse
        assert forward_call(dict(ok, lse=y + (5 * 8 + 8) * 4)) == 0
        assert forward_call(dict(ok, lse=None, ldl=0)) == 0
        assert backward_call(dict(ok, gv=gk + (8 * 8 + 8) * 4)) == 0
        assert backward_call(dict(ok, gq=ls + 48)) == 0
        for obj in (mh, fwd_only):
            obj.set_stream(None)
            obj.sync()
