"""The cases of the multi-head attention calls with dropout on the attention weights (include/hisparse_heads_dropout.h), shared by
tests/test_heads_dropout_cpu.py (libhisparse_cpu.so, in a child process) and tests/test_gpu_heads_dropout.py (the HIP library, on the
device), written against the memory interface of tests/pattern_cases.py, as tests/heads_bias_cases.py is.

The references are heads_bias_cases.ForwardReference and BackwardReference restated with a weight w_e in {0, c} per entry and head,
c = 1 / (1 - drop_p) in float64, taken from hsmhd_keep_mask (a call without a bias is held to the references at a zero bias: the same
T_e, and an eta_e that is an upper bound of the plain calls').  The bounds are derived, not fitted:

Forward.  The computed weights are P_e (1 + dl_e) / (1 + dl_bar) with |dl_e| <= rho_r and dl_bar a mean of the dl_e under the weights
of ALL the row's entries, so every one of them is off by at most 2 rho / (1 - rho) P_e, because |(1 + dl_e) / (1 + dl_bar) - 1| <=
2 rho / (1 - rho).  Without dropout the weights sum to one and the error can be centred on Y, which gives the term rho / (1 - rho)
sum P |V - Y|; the KEPT weights do not sum to one, so the term is
    2 rho / (1 - rho) sum_e w_e P_e |V_e|
and the summation term takes B = sum_e w_e P_e |V_e| (the multiplication by c, one more rounding of 2^-53, is inside its 16 spare
units).  l is summed over all entries, so LSE and bound_lse are the references' without dropout, unchanged.

Backward.  GP_e -> w_e GP_e, and its error gam_e -> w_e gam_e + 2^-52 |w_e GP_e| (the product by c is one more rounding in double).
P_e is the weight WITHOUT dropout, so rho_e and everything that is built from P_e, GP_e and gam_e keeps its form: D, epsD, GS, GB, eps,
mag, the bounds of gQ, gK and gbias.  gV_c = sum w_e P_e gY_e: w_e P_e takes the place of P_e in the value and in both bound terms.

With drop_p = 0 every w_e is 1.0 and every value above is the bias references' exactly in float64 (x * 1.0 = x, and the sums are formed
the same way); tests/test_heads_dropout_cpu.py asserts it without any library."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import heads as mha, heads_dropout as mhd

import attention_backward_cases as bc
import attention_cases as ac
import float_contract as fc
import heads_bias_cases as hb
import heads_cases as hc
import pattern_cases as pc
import wide_cases as wc
from heads_cases import SHAPES, cut, operands, same_words, words  # noqa: F401
from heads_bias_cases import biases, head_scores, check_forward, check_backward, check_gbias, rounded_forward, rounded_backward, rounded_gbias, long_pattern  # noqa: F401
from pattern_cases import HipMemory, HostMemory, edge_patterns, random_pattern  # noqa: F401

BAD_ARG = -1
SENTINEL, NAN_WORD = wc.SENTINEL, wc.NAN_WORD
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
TINY = 2.0 ** -149
GENERAL_SHAPES = SHAPES + ((8, 16),)      # (5, 4), (8, 16), (8, 32) and (64, 4) hold more than four heads: counter word h >> 2 is not 0
DEVICE = mhd.DropoutMultiHeadAttention


def scale_c(drop_p):
    """c = 1 / (1 - drop_p), formed in double from the float the call is given"""
    return 1.0 / (1.0 - float(np.float32(drop_p)))


def threshold(drop_p):
    return int(np.floor(float(np.float32(drop_p)) * 4294967296.0))


def weights(keep, drop_p):
    """(nnz, heads) float64: c where kept, 0 where dropped"""
    return np.asarray(keep, dtype=np.float64) * scale_c(drop_p)


def mask_weights(nnz, heads, drop_p, seed, offset):
    """the weights of a call, from hsmhd_keep_mask of the library under test"""
    return weights(mhd.keep_mask(nnz, heads, drop_p, seed, offset), drop_p)


# ---- the two references, restated with w_e ---------------------------------------------------------------------------------------------
class ForwardReference(ac.Reference):
    """heads_bias_cases.ForwardReference with the weights `w` (one float64 per entry, 0 or c) of one head; check() and rounded() are
    inherited.  A row with entries and a finite lse whose kept set is empty has Y = 0 and a bound of 2^-149: +-0.0 alone passes, and the
    cases assert the sign themselves."""

    def __init__(self, scores, V, scale, b, w):
        sc, s = float(np.float32(scale)), scores
        b = np.asarray(b, dtype=np.float32)
        w = np.asarray(w, dtype=np.float64)
        assert b.shape == s.S.shape == w.shape
        self.scores, ip, of = s, s.indptr, s.of
        self.n = np.diff(ip)
        self.d = V.shape[1]
        kk = 1.0 if s.exact else 2.0
        with np.errstate(all="ignore"):
            fin = s.fin & np.isfinite(b)
            t_bad = np.where(s.fin, b, np.float32(scale) * s.ieee + b)
            neg = ~fin & np.isneginf(t_bad)
            bad = ~fin & ~neg
            b64 = np.where(fin, b, 0.0).astype(np.float64)
            assert not (fin & ~np.isfinite(sc * s.S + b64)).any()
            T = np.where(fin, sc * s.S + b64, -np.inf)
            eta = (1.0 + fc.U) * abs(sc) * s.delta + fc.U * np.abs(sc * s.S) + TINY
            eta = np.where(fin, (1.0 + fc.U) * eta + fc.U * np.abs(T), 0.0)
            self.empty = self.n == 0
            self.bad = ac._seg_sum(bad[:, None].astype(np.float64), ip)[:, 0] > 0
            self.dead = ~self.empty & ~self.bad & (ac._seg_sum(fin[:, None].astype(np.float64), ip)[:, 0] == 0)
            self.finite = ~self.empty & ~self.bad & ~self.dead
            self.M = ac._seg_max(T, ip, -np.inf)
            live = self.finite[of]
            E = np.where(live, np.exp(T - np.where(live, self.M[of], 0.0)), 0.0)
            V64 = V.astype(np.float64)[s.indices]
            seg = ac._seg_fsum if s.exact else ac._seg_sum
            self.L = seg(E[:, None], ip)[:, 0]                      # over ALL entries
            Lsafe = np.where(self.finite, self.L, 1.0)
            self.P = E / Lsafe[of]                                   # the weights without dropout
            self.W = w
            self.Y = seg((w * E)[:, None] * V64, ip) / Lsafe[:, None]
            self.B = ac._seg_sum((w * self.P)[:, None] * np.abs(V64), ip)
            self.LSE = np.where(self.finite, self.M, 0.0) + np.log(Lsafe)
            self.eta = ac._seg_max(eta, ip, 0.0)
        self.rho = np.expm1(self.eta)
        assert (self.rho[self.finite] <= ac.RHO_MAX).all(), f"input condition: expm1(eta_r) reaches {self.rho[self.finite].max():.3g}"
        rho, n = self.rho[:, None], self.n[:, None]
        self.bound_y = fc.U * np.abs(self.Y) + 2.0 * rho / (1.0 - rho) * self.B + kk * (n + 16) * 2.0 ** -52 * self.B + TINY
        self.bound_lse = fc.U * np.abs(self.LSE) + self.eta + kk * (self.n + 16) * 2.0 ** -52 * (1.0 + np.abs(self.LSE)) + TINY
        self.kept = ac._seg_sum((w != 0)[:, None].astype(np.float64), ip)[:, 0]      # kept entries per row


class BackwardReference(hb.BackwardReference):
    """heads_bias_cases.BackwardReference with the weights `w` of one head; gradients(), check(), check_gbias(), rounded() and
    rounded_gbias() are inherited"""

    def __init__(self, scores, V, gY, lse, scale, b, w):
        s, sc = scores, float(np.float32(scale))
        b = np.asarray(b, dtype=np.float32)
        w = np.asarray(w, dtype=np.float64)
        assert b.shape == s.S.shape == w.shape and np.isfinite(b).all()
        self.scores, self.sc, self.d = s, sc, V.shape[1]
        ip, ix, of = s.indptr, s.indices, s.of
        assert s.fin.all() and gY.dtype == np.float32 and V.dtype == np.float32 and gY.shape[1] == V.shape[1] == s.d
        lse = np.asarray(lse, dtype=np.float32)
        assert lse.shape == (ip.size - 1,)
        self.kk = kk = 1.0 if s.exact else 2.0
        self.seg = ac._seg_fsum if s.exact else ac._seg_sum
        self.n = np.diff(ip)
        self.perm = np.argsort(ix, kind="stable")
        self.m = np.bincount(ix, minlength=V.shape[0]).astype(np.int64)
        self.cptr = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.empty_r, self.empty_c = self.n == 0, self.m == 0
        self.bad_r = ~self.empty_r & ~np.isfinite(lse)
        self.bad_c = np.zeros(V.shape[0], dtype=bool)
        self.bad_c[ix[self.bad_r[of]]] = True
        self.live = live = ~self.bad_r[of]
        g64 = (gY[of] * V[ix]).astype(np.float64)
        gp0 = np.array([math.fsum(row) for row in g64.tolist()], dtype=np.float64) if s.exact else g64.sum(axis=1)
        gam0 = fc.U * np.abs(gp0) + kk * self.d * 2.0 ** -52 * np.abs(g64).sum(axis=1) + TINY
        self.W = w
        self.GP = w * gp0                                                        # GP -> w GP
        gam = w * gam0 + 2.0 ** -52 * np.abs(self.GP)                            # gam -> w gam + 2^-52 |w GP|
        T = sc * s.S + b.astype(np.float64)
        assert np.isfinite(T).all()
        eta = (1.0 + fc.U) * abs(sc) * s.delta + fc.U * np.abs(sc * s.S) + TINY
        eta = (1.0 + fc.U) * eta + fc.U * np.abs(T)
        self.rho = rho = np.expm1(eta + 32.0 * 2.0 ** -52)
        assert (rho[live] <= bc.RHO_MAX).all(), f"input condition: rho_e reaches {rho[live].max():.3g}"
        with np.errstate(all="ignore"):
            self.P = P = np.where(live, np.exp(T - np.where(live, lse.astype(np.float64)[of], 0.0)), 0.0)
        assert np.isfinite(P).all()
        self.K64, self.Q64, self.G64 = K64, Q64, G64 = s.K64[ix], s.Q64[of], gY.astype(np.float64)[of]
        self.D = self.seg((P * self.GP)[:, None], ip)[:, 0]
        Dof = self.D[of]
        eps_d = ac._seg_sum((P * (rho * np.abs(self.GP) + (1.0 + rho) * gam))[:, None], ip)[:, 0] + kk * (self.n + 16) * 2.0 ** -52 * ac._seg_sum((P * np.abs(self.GP))[:, None], ip)[:, 0]
        self.GB = P * (self.GP - Dof)
        self.GS = sc * P * (self.GP - Dof)
        eps1 = rho * P * np.abs(self.GP - Dof) + (1.0 + rho) * P * (gam + eps_d[of])
        eps = abs(sc) * eps1
        self.bound_gb = eps1 + fc.U * np.abs(self.GB) + TINY
        self.mag = mag = abs(sc) * P * (np.abs(self.GP) + np.abs(Dof))
        self.PW = PW = w * P                                                     # P -> w P in gV
        self.GQ, self.GK, self.GV = self.gradients(self.GS, PW)
        n, m, pm = self.n[:, None], self.m[:, None], self.perm
        self.bound = {"gq": fc.U * np.abs(self.GQ) + ac._seg_sum(eps[:, None] * np.abs(K64), ip) + kk * (n + 16) * 2.0 ** -52 * ac._seg_sum(mag[:, None] * np.abs(K64), ip) + TINY,
                      "gk": fc.U * np.abs(self.GK) + ac._seg_sum((eps[:, None] * np.abs(Q64))[pm], self.cptr)
                      + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((mag[:, None] * np.abs(Q64))[pm], self.cptr) + TINY,
                      "gv": fc.U * np.abs(self.GV) + ac._seg_sum(((rho * PW)[:, None] * np.abs(G64))[pm], self.cptr)
                      + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((PW[:, None] * np.abs(G64))[pm], self.cptr) + TINY}
        self.want = {"gq": self.GQ, "gk": self.GK, "gv": self.GV}
        self.empty = {"gq": self.empty_r, "gk": self.empty_c, "gv": self.empty_c}
        self.bad = {"gq": self.bad_r, "gk": self.bad_c, "gv": self.bad_c}


def _bias_or_zero(bias, nnz, heads):
    return np.zeros((nnz, heads), dtype=np.float32) if bias is None else bias


def forward_refs(scores, V, scale, bias, W):
    """bias: (nnz, heads) float32 or None; W: (nnz, heads) float64"""
    d = V.shape[1] // len(scores)
    bias = _bias_or_zero(bias, W.shape[0], len(scores))
    return [ForwardReference(s, cut(V, h, d), scale, np.ascontiguousarray(bias[:, h]), np.ascontiguousarray(W[:, h])) for h, s in enumerate(scores)]


def backward_refs(scores, V, gY, lse, scale, bias, W):
    d = V.shape[1] // len(scores)
    lse = np.asarray(lse, dtype=np.float32)
    assert lse.shape == (scores[0].indptr.size - 1, len(scores))
    bias = _bias_or_zero(bias, W.shape[0], len(scores))
    return [BackwardReference(s, cut(V, h, d), cut(gY, h, d), np.ascontiguousarray(lse[:, h]), scale, np.ascontiguousarray(bias[:, h]), np.ascontiguousarray(W[:, h]))
            for h, s in enumerate(scores)]


class Drop:
    """drop_p, seed and offset of a call"""

    def __init__(self, drop_p, seed, offset):
        self.p, self.seed, self.offset = drop_p, seed, offset

    def args(self):
        return self.p, self.seed, self.offset

    def weights(self, nnz, heads):
        return mask_weights(nnz, heads, self.p, self.seed, self.offset)


# ---- the forms ---------------------------------------------------------------------------------------------------------------------------
def forward_host(mh, Q, K, V, bias, heads, scale, dr, want_lse=True):
    """(y, lse or None)"""
    if want_lse:
        return DEVICE.forward(mh, Q, K, V, bias, heads, scale, *dr.args())
    return DEVICE.forward(mh, Q, K, V, bias, heads, scale, *dr.args(), want_lse=False), None


def forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, pad=0, extra=0, want_lse=True, what=""):
    """hsmhd_forward_device over fresh buffers: the pads of the inputs NaN, y and lse pre-filled with a sentinel; the pad words of both must
    survive.  bias None: the call is given NULL and ldb = 0."""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv) = (wc._features_in(mem, a, pad) for a in (Q, K, V))
    db, ldb = hb._entries_in(mem, bias, extra) if bias is not None else (None, 0)
    ldy, ldl = w + pad, heads + extra
    dy = mem.alloc(np.full((mh.num_rows, ldy), SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full((mh.num_rows, ldl), SENTINEL, dtype=np.uint32)) if want_lse else None
    DEVICE.forward_device(mh, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, db.ptr if db else None, ldb, heads, w // heads, scale, *dr.args(), dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = wc._features_out(mem, mh, dy, mh.num_rows, w, ldy, what)
    if not want_lse:
        return y, None
    lw = mem.read(mh, dl).reshape(mh.num_rows, ldl)
    assert (lw[:, heads:] == SENTINEL).all(), f"{what}: the pad words of lse were written"
    return y, np.ascontiguousarray(lw[:, :heads]).view(np.float32)


def backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, dr, want_gbias=True):
    """(gq, gk, gv, gbias or None)"""
    return DEVICE.backward(mh, Q, K, V, gY, lse, bias, heads, scale, *dr.args(), want_gbias=want_gbias)


def backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, pad=0, extra=0, want_gbias=True, what=""):
    """hsmhd_backward_device over fresh buffers: the pads of the inputs NaN, the four outputs pre-filled with a sentinel; the words h >= heads
    of gbias must survive"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (wc._features_in(mem, a, pad) for a in (Q, K, V, gY))
    dl, ldl = hc._lse_in(mem, lse, extra)
    db, ldb = hb._entries_in(mem, bias, extra) if bias is not None else (None, 0)
    ld, ldgb, nnz = w + pad, heads + extra, mh.nnz
    oq = mem.alloc(np.full((mh.num_rows, ld), SENTINEL, dtype=np.uint32))
    ok, ov = (mem.alloc(np.full((mh.num_cols, ld), SENTINEL, dtype=np.uint32)) for _ in range(2))
    ob = mem.alloc(np.full((nnz, ldgb), SENTINEL, dtype=np.uint32)) if want_gbias else None
    DEVICE.backward_device(mh, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, db.ptr if db else None, ldb, heads, w // heads, scale, *dr.args(), oq.ptr, ld, ok.ptr, ld,
                           ov.ptr, ld, ob.ptr if want_gbias else None, ldgb)
    out = tuple(wc._features_out(mem, mh, buf, n, w, ld, f"{what}, {name}") for name, buf, n in (("gq", oq, mh.num_rows), ("gk", ok, mh.num_cols), ("gv", ov, mh.num_cols)))
    if not want_gbias:
        return out + (None,)
    gw = mem.read(mh, ob).reshape(nnz, ldgb)
    assert (gw[:, heads:] == SENTINEL).all(), f"{what}: the words h >= heads of gbias were written"
    return out + (np.ascontiguousarray(gw[:, :heads]).view(np.float32),)


def all_forward_forms(mem, mh, refs, Q, K, V, bias, heads, scale, dr, what):
    """the host form with lse taken and NULL, the device form tight and padded (pad 8, ldl = ldb = heads + 3), the padded one with lse
    NULL too, inside the bounds of one set of references; returns the lse of the host form"""
    y, lse = forward_host(mh, Q, K, V, bias, heads, scale, dr)
    check_forward(refs, y, lse, f"{what}, host form, lse taken")
    check_forward(refs, forward_host(mh, Q, K, V, bias, heads, scale, dr, False)[0], None, f"{what}, host form, lse NULL")
    for pad, extra, want in ((0, 0, True), (8, 3, True), (8, 3, False)):
        tag = f"{what}, device form, pad {pad}, ldl and ldb {heads + extra}, {'lse taken' if want else 'lse NULL'}"
        check_forward(refs, *forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, pad, extra, want, tag), tag)
    return lse


def all_backward_forms(mem, mh, refs, Q, K, V, gY, lse, bias, heads, scale, dr, what):
    """the host form and the device form tight and padded, each with gbias given and with NULL: the same gQ, gK and gV words either way"""
    worst = dict.fromkeys(bc.OUTPUTS + ("gbias",), 0.0)
    for tag, call in ((f"{what}, host form", lambda want: backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, dr, want)),
                      (f"{what}, device form, pad 0", lambda want: backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, 0, 0, want, what)),
                      (f"{what}, device form, pad 8, ld {heads + 3}", lambda want: backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, 8, 3, want, what))):
        gq, gk, gv, gb = call(True)
        w = dict(check_backward(refs, gq, gk, gv, tag), gbias=check_gbias(refs, gb, tag))
        worst = {k: max(worst[k], w[k]) for k in worst}
        without = call(False)
        assert without[3] is None and same_words(without[:3], (gq, gk, gv)), f"{tag}: gbias NULL changes gq, gk or gv"
    return worst


def step(mem, mh, scores, Q, K, V, gY, bias, heads, scale, dr, what, pad=4, extra=1):
    """one device-form forward and the backward with the lse it wrote, both against the references; returns (y, lse, gq, gk, gv, gb)"""
    W = dr.weights(mh.nnz, heads)
    y, lse = forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, pad, extra, True, what)
    fwd = forward_refs(scores, V, scale, bias, W)
    check_forward(fwd, y, lse, what)
    bwd = backward_refs(scores, V, gY, lse, scale, bias, W)
    gq, gk, gv, gb = backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, pad, extra, True, what)
    check_backward(bwd, gq, gk, gv, what)
    check_gbias(bwd, gb, what)
    return y, lse, gq, gk, gv, gb


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
GENERAL = ((0.1, True, 0.125), (0.5, False, -2.0), (0.5, True, 1.0), (0.1, False, 0.5))      # (drop_p, a bias or NULL, scale)


def general(mem, shapes=GENERAL_SHAPES):
    """300 x 517, 4000 entries, every (heads, d) of heads_cases.SHAPES and (8, 16); drop_p 0.1 and 0.5, each with a bias in [-4, 4] and with
    NULL; forward in every form, then backward in every form with the lse the forward just wrote"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with DEVICE((indptr, indices, shape), heads) as mh:
            assert mh.nnz == NNZ
            Q, K, V, gY = operands(shape, heads * d, 13100 + 1000 * heads + d)
            given = biases(NNZ, heads, 13150 + 1000 * heads + d)
            scores = head_scores(indptr, indices, Q, K, heads)
            for i, (p, with_bias, scale) in enumerate(GENERAL):
                dr = Drop(p, 0x9E3779B97F4A7C15 + heads, (1 << 40) + 17 * i + d)
                bias = given if with_bias else None
                W = dr.weights(NNZ, heads)
                what = f"general, {heads} heads of d {d}, drop_p {p}, {'a bias' if with_bias else 'bias NULL'}, scale {scale}"
                lse = all_forward_forms(mem, mh, forward_refs(scores, V, scale, bias, W), Q, K, V, bias, heads, scale, dr, what)
                w = all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, scale, bias, W), Q, K, V, gY, lse, bias, heads, scale, dr, what)
                print(f"{what}: backward worst error / bound = {w['gq']:.3f} (gq), {w['gk']:.3f} (gk), {w['gv']:.3f} (gv), {w['gbias']:.3f} (gbias)")


def zero_drop(mem, shapes=((4, 16), (5, 4), (2, 128), (8, 16))):
    """drop_p = 0: thr = 0 and c = 1.0, so every output word is bit for bit that of hsmhb_* with the same bias, and with bias NULL that of
    hsmh_*, forward and backward, in both forms, whatever seed and offset say"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with DEVICE((indptr, indices, shape), heads) as mh:
            Q, K, V, gY = operands(shape, heads * d, 13700 + d)
            bias = biases(NNZ, heads, 13710 + d)
            plain = hb.Plain(mh)
            dr = Drop(0.0, 77 + d, 1 << 33)
            assert mhd.keep_mask(NNZ, heads, *dr.args()).all()
            for scale in (0.5, -2.0):
                what = f"drop_p 0, {heads} heads of d {d}, scale {scale}"
                # with a bias: hsmhb_*
                want_f = hb.forward_device(mem, mh, Q, K, V, bias, heads, scale, 4, 1, True, what)
                assert same_words(want_f, forward_device(mem, mh, Q, K, V, bias, heads, scale, dr, 4, 1, True, what)), f"{what}: the forward differs from hsmhb_forward_device"
                assert same_words(hb.forward_host(mh, Q, K, V, bias, heads, scale), forward_host(mh, Q, K, V, bias, heads, scale, dr)), f"{what}: the host forward differs from hsmhb_forward"
                lse = want_f[1]
                want_b = hb.backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, 4, 1, True, what)
                assert same_words(want_b, backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, dr, 4, 1, True, what)), f"{what}: the backward differs from hsmhb_backward_device"
                assert same_words(hb.backward_host(mh, Q, K, V, gY, lse, bias, heads, scale), backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, dr)), f"{what}: the host backward differs"
                # bias NULL: hsmh_*
                plain_f = hc.forward_device(mem, plain, Q, K, V, heads, scale, 4, 1, True, what)
                assert same_words(plain_f, forward_device(mem, mh, Q, K, V, None, heads, scale, dr, 4, 1, True, what)), f"{what}: the forward with bias NULL differs from hsmh_forward_device"
                assert same_words(hc.forward_host(plain, Q, K, V, heads, scale), forward_host(mh, Q, K, V, None, heads, scale, dr)), f"{what}: the host forward with bias NULL differs"
                lse = plain_f[1]
                plain_b = hc.backward_device(mem, plain, Q, K, V, gY, lse, heads, scale, 4, 1, what)
                got = backward_device(mem, mh, Q, K, V, gY, lse, None, heads, scale, dr, 4, 1, True, what)
                assert same_words(plain_b, got[:3]), f"{what}: the backward with bias NULL differs from hsmh_backward_device"
                assert same_words(hc.backward_host(plain, Q, K, V, gY, lse, heads, scale), backward_host(mh, Q, K, V, gY, lse, None, heads, scale, dr)[:3]), f"{what}: the host backward differs"
                zero = np.zeros((NNZ, heads), dtype=np.float32)
                check_gbias(hb.backward_refs(head_scores(indptr, indices, Q, K, heads), V, gY, lse, scale, zero), got[3], what)


def twice_pattern():
    """60 x 70, 500 entries and one pair held twice (row 11 holds its first column again, as its last entry); the columns of a row are
    not sorted where the pair was added, and the order of the entries by column is not their CSR order"""
    indptr, indices = random_pattern(60, 70, 500, 21)
    ip = indptr.astype(np.int64)
    r = 11
    assert ip[r + 1] - ip[r] >= 2
    indices = np.concatenate([indices[: ip[r + 1]], indices[ip[r]: ip[r] + 1], indices[ip[r + 1]:]]).astype(np.uint32)
    indptr = indptr.copy()
    indptr[r + 1:] += 1
    first, last = int(ip[r]), int(ip[r + 1])      # the two entries of the pair
    assert indices[first] == indices[last] and indices.size == 501
    assert not np.array_equal(np.argsort(indices, kind="stable"), np.arange(indices.size)), "the column order is the row order"
    return indptr, indices, first, last


def mask_agreement(mem, shapes=((4, 16), (5, 4), (8, 16))):
    """Forward, row side and column side index the entries the same way: over a pattern whose column order is not its CSR order and which
    holds a pair twice, Y and all four gradients agree with the references built from hsmhd_keep_mask, in both forms.  The pair's two
    entries are two draws: the seed is chosen so that they differ in head 0."""
    indptr, indices, first, last = twice_pattern()
    shape = (60, 70)
    nnz = indices.size
    for heads, d in shapes:
        dr = Drop(0.5, 4243, 9)
        keep = mhd.keep_mask(nnz, heads, *dr.args())
        assert keep[first, 0] != keep[last, 0], "choose a seed for which the two entries of the pair draw differently in head 0"
        assert 0.3 < keep.mean() < 0.7
        Q, K, V, gY = operands(shape, heads * d, 14000 + d)
        bias = biases(nnz, heads, 14010 + d)
        scores = head_scores(indptr, indices, Q, K, heads)
        W = weights(keep, dr.p)
        with DEVICE((indptr, indices, shape), heads) as mh:
            assert mh.nnz == nnz
            what = f"forward and backward agree on the mask, {heads} heads of d {d}"
            lse = all_forward_forms(mem, mh, forward_refs(scores, V, 0.5, bias, W), Q, K, V, bias, heads, 0.5, dr, what)
            all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, 0.5, bias, W), Q, K, V, gY, lse, bias, heads, 0.5, dr, what)
            step(mem, mh, scores, Q, K, V, gY, None, heads, 0.5, dr, what + ", bias NULL")


def short_rows_pattern(rows=200, cols=90, seed=31):
    """rows of 1 to 3 entries, every tenth row empty"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 4, rows)
    n[::10] = 0
    indptr = np.zeros(rows + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(n)
    indices = np.concatenate([np.sort(rng.choice(cols, int(k), replace=False)) for k in n]).astype(np.uint32)
    return indptr, indices


def fully_dropped_rows(mem, shapes=((4, 16), (3, 8))):
    """drop_p = 0.9 on rows of 1 to 3 entries: a (row, head) with entries and no kept entry reads +0.0 in its d words of Y, bit for bit,
    not NaN; lse is, word for word, the lse of the call without dropout; the backward agrees with the reference (gQ of such a head is
    exactly zero too: every GP is 0 and so is D)."""
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
        Q, K, V, gY = operands(shape, heads * d, 14100 + d)
        bias = biases(nnz, heads, 14110 + d)
        scores = head_scores(indptr, indices, Q, K, heads)
        with DEVICE((indptr, indices, shape), heads) as mh:
            for b in (bias, None):
                what = f"fully dropped rows, {heads} heads of d {d}, {'a bias' if b is not None else 'bias NULL'}"
                for form in ("host", "device"):
                    y, lse = forward_host(mh, Q, K, V, b, heads, 0.5, dr) if form == "host" else forward_device(mem, mh, Q, K, V, b, heads, 0.5, dr, 4, 1, True, what)
                    y0, lse0 = forward_host(mh, Q, K, V, b, heads, 0.5, Drop(0.0, 0, 0))
                    assert same_words((lse,), (lse0,)), f"{what}, {form} form: lse is not the lse without dropout"
                    yw = words(y).reshape(200, heads, d)
                    assert not yw[gone].any(), f"{what}, {form} form: a fully dropped (row, head) is not +0.0"
                    assert np.isfinite(y).all() and np.isfinite(lse[nonempty]).all()
                    assert (words(y0).reshape(200, heads, d)[gone] != 0).any()
                y, lse, gq, gk, gv, gb = step(mem, mh, scores, Q, K, V, gY, b, heads, 0.5, dr, what)
                assert not words(gq).reshape(200, heads, d)[gone].any(), f"{what}: gq of a fully dropped (row, head) is not +0.0"
                assert (gb[~(keep != 0) & nonempty[of][:, None] & ~gone[of]] != 0).any(), "a dropped entry's gbias word is -P D, not zero"


def long_rows_and_columns(mem, n, shapes=((4, 16), (3, 8))):
    """the device forms over heads_bias_cases.long_pattern(n) (one row of 600 and one column of 700 entries), drop_p 0.5, forward then
    backward with the lse just written, float64 sums in the references; n is chosen by the caller so that the grid's stride loop runs"""
    indptr, indices = long_pattern(n)
    shape = (n, n)
    for heads, d in shapes:
        what = f"long row and column among {n}, {heads} heads of d {d}, drop_p 0.5"
        Q, K, V, gY = operands(shape, heads * d, 14200 + d)
        bias = biases(indices.size, heads, 14210 + d)
        scores = head_scores(indptr, indices, Q, K, heads, exact=False)
        dr = Drop(0.5, 99, (1 << 32) + 1)
        with DEVICE((indptr, indices, shape), heads) as mh:
            got = step(mem, mh, scores, Q, K, V, gY, bias, heads, 0.5, dr, what)
            assert same_words(got[2:], backward_device(mem, mh, Q, K, V, gY, got[1], bias, heads, 0.5, dr, 4, 1, True, what)), f"{what}: two calls give other words"
            step(mem, mh, scores, Q, K, V, gY, None, heads, 0.5, dr, what + ", bias NULL")


def edges(mem, heads=3, d=8):
    """every pattern of pattern_cases.edge_patterns() at (3, 8) with drop_p 0.5, a bias and NULL: empty rows and columns, nnz = 0 with
    NULL indices (no per-entry pointer is dereferenced), unsorted columns, a pair held twice"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with DEVICE((indptr, indices, shape), heads) as mh:
            assert mh.nnz == indices.size
            Q, K, V, gY = operands(shape, heads * d, 14300)
            given = biases(indices.size, heads, 14310)
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


def seeds_and_offsets(mem, heads=5, d=4):
    """different seeds give different masks and different words; offset k and offset 2^32 + k too (the high word of the offset is used),
    and so do the two halves of the seed; the same inputs twice give the same words"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    Q, K, V, gY = operands(shape, heads * d, 14400)
    bias = biases(NNZ, heads, 14410)
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


def mask_and_dropout(mem, heads=4, d=16):
    """A -inf bias on a random third of the entries (the first entry of every row stays) together with drop_p 0.5 computes what the pattern
    WITHOUT those entries computes under the same draws for the remaining entries' CSR indices of the ORIGINAL pattern: the reference is
    built over the reduced pattern with the rows of hsmhd_keep_mask(original nnz) of the kept entries.  The masked entries' gbias words
    are zero."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 6)
    shape = (ROWS, COLS)
    rng = np.random.default_rng(14500)
    of = pc.entry_rows(indptr)
    masked = rng.random(NNZ) < 1.0 / 3.0
    masked[indptr[:-1][np.diff(indptr.astype(np.int64)) > 0]] = False
    stay = ~masked
    assert NNZ // 4 < masked.sum() < NNZ // 2
    kptr = np.zeros(ROWS + 1, dtype=np.uint32)
    kptr[1:] = np.cumsum(np.bincount(of[stay], minlength=ROWS))
    kidx = indices[stay]
    Q, K, V, gY = operands(shape, heads * d, 14510)
    bias = biases(NNZ, heads, 14520)
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
            y, lse = forward_host(mh, Q, K, V, with_mask, heads, scale, dr) if form == "host" else forward_device(mem, mh, Q, K, V, with_mask, heads, scale, dr, 4, 1, True, what)
            check_forward(fwd, y, lse, what)
            bwd = backward_refs(scores, V, gY, lse, scale, bias[stay], W)
            got = backward_host(mh, Q, K, V, gY, lse, with_mask, heads, scale, dr) if form == "host" else backward_device(mem, mh, Q, K, V, gY, lse, with_mask, heads, scale, dr, 4, 1, True, what)
            check_backward(bwd, *got[:3], what)
            check_gbias(bwd, got[3][stay], what)
            assert not (got[3][masked] != 0).any(), f"{what}: a masked entry's gbias word is not zero"


# ---- refusals and objects ----------------------------------------------------------------------------------------------------------------
FEATURES = hc.FEATURES
BAD_DROPS = (1.0, -0.1, float("nan"), float("inf"), -float("inf"), 1.5)


def refusals(mem):
    """drop_p of 1.0, -0.1, NaN and inf is HS_ERR_BAD_ARG with a message in all four calls and in hsmhd_keep_mask; a backward on an object
    without the entry map is HS_ERR_BAD_ARG and the message names hsmhb_create, with a bias and without; the forward runs on any object
    and hsmh_info reports what it reported; the overlap and alignment rules of hisparse_heads_bias.h hold, also for gbias without a bias;
    after every refusal the object is usable"""
    l = mhd.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    heads, d = 2, 4
    w = heads * d
    one = np.zeros(4, dtype=np.float32).ctypes.data
    assert l.hsmhd_forward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 1, 1, 4, 1.0, 0.5, 1, 1, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsmhd_forward(None, vp(one), vp(one), vp(one), vp(one), 1, 4, 1.0, 0.5, 1, 1, vp(one), None) == BAD_ARG
    assert l.hsmhd_backward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 1, vp(one), 1, 1, 4, 1.0, 0.5, 1, 1, vp(one), 4, vp(one), 4, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsmhd_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), vp(one), 1, 4, 1.0, 0.5, 1, 1, vp(one), vp(one), vp(one), None) == BAD_ARG
    # hsmhd_keep_mask needs no object
    k = np.zeros((7, heads), dtype=np.uint8)
    assert l.hsmhd_keep_mask(7, heads, 0.5, 1, 2, k.ctypes.data) == 0 and l.hsmhd_keep_mask(0, heads, 0.5, 1, 2, None) == 0
    for bad in BAD_DROPS:
        assert l.hsmhd_keep_mask(7, heads, bad, 1, 2, k.ctypes.data) == BAD_ARG, bad
    assert l.hsmhd_keep_mask(7, 0, 0.5, 1, 2, k.ctypes.data) == BAD_ARG and l.hsmhd_keep_mask(7, 65, 0.5, 1, 2, k.ctypes.data) == BAD_ARG
    assert l.hsmhd_keep_mask(7, heads, 0.5, 1, 2, None) == BAD_ARG
    dr = Drop(0.25, 3, 4)
    with DEVICE((indptr, indices, shape), 4) as mh, mha.MultiHeadAttention((indptr, indices, shape), 4) as plain, DEVICE((indptr, indices, shape), 4, backward=False) as no_flag:
        Q, K, V, gY = operands(shape, w, 14600)
        bias = biases(7, heads, 14610)
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
            assert same_words(want_f, forward_device(mem, obj, Q, K, V, bias, heads, 0.5, dr, 4, 1, True, "no map"))
            for b in (bias, None):
                for call in (lambda: backward_host(obj, Q, K, V, gY, want_f[1], b, heads, 0.5, dr), lambda: backward_device(mem, obj, Q, K, V, gY, want_f[1], b, heads, 0.5, dr)):
                    try:
                        call()
                    except mha.DeviceError as e:
                        assert e.code == BAD_ARG and "hsmhb_create" in str(e), str(e)
                    else:
                        raise AssertionError("the backward with dropout ran on an object without the entry map")
            assert same_words(want_f, forward_host(obj, Q, K, V, bias, heads, 0.5, dr)), "unusable after the refused backward"
        assert {obj: obj.info() for obj in (mh, plain, no_flag)} == info, "hsmh_info changed"

        def still_usable(rc, what):
            assert rc == BAD_ARG and l.hsmh_last_error(mh._h), (what, rc)
            assert same_words(forward_host(mh, Q, K, V, bias, heads, 0.5, dr), want_f), f"unusable after {what}"
            assert same_words(backward_host(mh, Q, K, V, gY, want_f[1], bias, heads, 0.5, dr), want_b), f"unusable after {what}"

        def forward_call(a):
            return l.hsmhd_forward_device(mh._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["bias"]), a["ldb"], a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6,
                                          vp(a["y"]), a["ldy"], vp(a["lse"]), a["ldl"])

        def backward_call(a):
            return l.hsmhd_backward_device(mh._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["ldl"], vp(a["bias"]), a["ldb"],
                                           a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6, vp(a["gq"]), a["ldgq"], vp(a["gk"]), a["ldgk"], vp(a["gv"]), a["ldgv"], vp(a["gbias"]), a["ldgb"])

        names = FEATURES + ("y", "lse", "bias", "gbias")
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 8 for name in FEATURES + ("y",)}, heads=heads, d=d, scale=1.0, drop_p=0.5, ldl=2, ldb=2, ldgb=2)
        no_bias = dict(ok, bias=None, ldb=0)
        assert forward_call(ok) == 0 and backward_call(ok) == 0 and backward_call(dict(ok, gbias=None, ldgb=0)) == 0
        assert forward_call(no_bias) == 0 and backward_call(no_bias) == 0 and backward_call(dict(no_bias, gbias=None, ldgb=0)) == 0
        for bad in BAD_DROPS:
            for base in (ok, no_bias):
                still_usable(forward_call(dict(base, drop_p=bad)), f"forward_device: drop_p {bad}")
                assert b"drop_p" in l.hsmh_last_error(mh._h)
                still_usable(backward_call(dict(base, drop_p=bad)), f"backward_device: drop_p {bad}")
                assert b"drop_p" in l.hsmh_last_error(mh._h)
        for what, change in (("misaligned bias", dict(bias=ok["bias"] + 2)), ("ldb < heads", dict(ldb=1)), ("y is bias", dict(y=ok["bias"])), ("lse is bias", dict(lse=ok["bias"])),
                             ("misaligned q", dict(q=ok["q"] + 4)), ("y is q", dict(y=ok["q"])), ("d = 5", dict(heads=1, d=5)), ("scale NaN", dict(scale=float("nan"))),
                             ("heads > max_heads", dict(heads=5)), ("ldl < heads", dict(ldl=1))):
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("misaligned bias", dict(bias=ok["bias"] + 2)), ("ldb < heads", dict(ldb=1)), ("misaligned gbias", dict(gbias=ok["gbias"] + 2)), ("ldgb < heads", dict(ldgb=1)),
                  ("gq is bias", dict(gq=ok["bias"])), ("gv inside bias", dict(gv=ok["bias"] + 16)), ("gq is q", dict(gq=ok["q"])), ("misaligned gy", dict(gy=ok["gy"] + 4)),
                  ("null lse", dict(lse=None))]
        bcases += [(f"gbias is {name}", dict(gbias=ok[name])) for name in ("q", "k", "v", "gy", "lse", "bias", "gq", "gk", "gv")]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        for what, change in [("misaligned gbias", dict(gbias=ok["gbias"] + 2)), ("ldgb < heads", dict(ldgb=1))] + [(f"gbias is {name}", dict(gbias=ok[name])) for name in ("q", "lse", "gk")]:
            still_usable(backward_call(dict(no_bias, **change)), "backward_device, bias NULL: " + what)
        # the host forms
        host = {name: np.zeros(9 * 8, np.float32) for name in names}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, heads=heads, d=d, scale=1.0, drop_p=0.5)

        def forward_host_call(a):
            return l.hsmhd_forward(mh._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["bias"]), a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6, vp(a["y"]), vp(a["lse"]))

        def backward_host_call(a):
            return l.hsmhd_backward(mh._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), vp(a["bias"]), a["heads"], a["d"], a["scale"], a["drop_p"], 5, 6, vp(a["gq"]),
                                    vp(a["gk"]), vp(a["gv"]), vp(a["gbias"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0 and backward_host_call(dict(okh, gbias=None)) == 0
        assert forward_host_call(dict(okh, bias=None)) == 0 and backward_host_call(dict(okh, bias=None)) == 0
        for bad in BAD_DROPS:
            still_usable(forward_host_call(dict(okh, drop_p=bad)), f"forward: drop_p {bad}")
            still_usable(backward_host_call(dict(okh, drop_p=bad, bias=None)), f"backward: drop_p {bad}")
        for what, change in (("y is bias", dict(y=okh["bias"])), ("d = 6", dict(d=6)), ("null q", dict(q=None))):
            still_usable(forward_host_call(dict(okh, **change)), "forward: " + what)
        for what, change in (("gbias is bias", dict(gbias=okh["bias"])), ("gbias is gk", dict(gbias=okh["gk"], bias=None)), ("gq is bias", dict(gq=okh["bias"])), ("null lse", dict(lse=None))):
            still_usable(backward_host_call(dict(okh, **change)), "backward: " + what)
        mh.set_stream(None)
        mh.sync()
