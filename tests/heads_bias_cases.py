"""The cases of the multi-head attention calls with a per-entry, per-head bias (include/hisparse_heads_bias.h), shared by
tests/test_heads_bias_cpu.py (libhisparse_cpu.so, in a child process) and tests/test_gpu_heads_bias.py (the HIP library, on the device),
written against the memory interface of tests/pattern_cases.py, as tests/heads_cases.py is.

The reference is the project's own two references (attention_cases.Reference, attention_backward_cases.Reference) restated per head with
    T_e = scale S_e + b_e
where b_e is the bias word of the entry and head.  The per-entry score error becomes
    eta'_e = (1 + u) eta_e + u |T_e|,      u = 2^-24,
eta_e being the existing expression taken at scale S_e and the new term the rounding of the one extra add.  Everything downstream of
eta_e is unchanged: rho, the bounds of Y, lse, gQ, gK and gV, and the input condition rho <= 2^-12, asserted by both references.  The
gradient of the bias, GB_e = P_e (GP_e - D_r), is held to
    eps_e / |scale| + u |GB_e| + 2^-149
with eps_e the backward reference's bound on GS_e (formed here without its factor |scale|, so that scale = 0 is covered) and the rest the
final rounding.  No other tolerance is introduced.  Bias values are drawn in [-4, 4], so that the input condition holds with room.
A bias word that is not finite makes its score -inf, +inf or NaN, and the row follows the forward reference's table; the backward
reference takes finite scores only (a masked pattern is compared with the reference over the pattern without the masked entries)."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import heads as mha, heads16, heads_bias as mhb

import attention_backward_cases as bc
import attention_cases as ac
import float_contract as fc
import heads_cases as hc
import pattern_cases as pc
import rows_cases as rc
import wide_cases as wc
from heads_cases import SHAPES, cut, operands, same_words, words  # noqa: F401
from pattern_cases import HipMemory, HostMemory, edge_patterns, random_pattern  # noqa: F401

BAD_ARG = -1
SENTINEL, NAN_WORD = wc.SENTINEL, wc.NAN_WORD
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
TINY = 2.0 ** -149


# ---- the two references, restated with T_e = scale S_e + b_e ----------------------------------------------------------------------------
class ForwardReference(ac.Reference):
    """attention_cases.Reference with the bias words `b` (one float32 per entry) of one head; check() and rounded() are inherited"""

    def __init__(self, scores, V, scale, b):
        sc, s = float(np.float32(scale)), scores
        b = np.asarray(b, dtype=np.float32)
        assert b.shape == s.S.shape
        self.scores, ip, of = s, s.indptr, s.of
        self.n = np.diff(ip)
        self.d = V.shape[1]
        kk = 1.0 if s.exact else 2.0
        with np.errstate(all="ignore"):
            fin = s.fin & np.isfinite(b)
            t_bad = np.where(s.fin, b, np.float32(scale) * s.ieee + b)       # the non-finite scores' t, in fp32 (a finite score plus such a bias is the bias)
            neg = ~fin & np.isneginf(t_bad)
            bad = ~fin & ~neg                                                 # NaN or +inf
            b64 = np.where(fin, b, 0.0).astype(np.float64)
            assert not (fin & ~np.isfinite(sc * s.S + b64)).any()
            T = np.where(fin, sc * s.S + b64, -np.inf)
            eta = (1.0 + fc.U) * abs(sc) * s.delta + fc.U * np.abs(sc * s.S) + TINY      # the existing expression at scale S_e
            eta = np.where(fin, (1.0 + fc.U) * eta + fc.U * np.abs(T), 0.0)              # and the rounding of the add
            self.empty = self.n == 0
            self.bad = ac._seg_sum(bad[:, None].astype(np.float64), ip)[:, 0] > 0
            self.dead = ~self.empty & ~self.bad & (ac._seg_sum(fin[:, None].astype(np.float64), ip)[:, 0] == 0)
            self.finite = ~self.empty & ~self.bad & ~self.dead
            self.M = ac._seg_max(T, ip, -np.inf)
            live = self.finite[of]
            E = np.where(live, np.exp(T - np.where(live, self.M[of], 0.0)), 0.0)
            V64 = V.astype(np.float64)[s.indices]
            seg = ac._seg_fsum if s.exact else ac._seg_sum
            self.L = seg(E[:, None], ip)[:, 0]
            Lsafe = np.where(self.finite, self.L, 1.0)
            self.P = E / Lsafe[of]
            self.Y = seg(E[:, None] * V64, ip) / Lsafe[:, None]
            self.D = ac._seg_sum(self.P[:, None] * np.abs(V64 - self.Y[of]), ip)
            self.B = ac._seg_sum(self.P[:, None] * np.abs(V64), ip)
            self.LSE = np.where(self.finite, self.M, 0.0) + np.log(Lsafe)
            self.eta = ac._seg_max(eta, ip, 0.0)
        self.rho = np.expm1(self.eta)
        assert (self.rho[self.finite] <= ac.RHO_MAX).all(), f"input condition: expm1(eta_r) reaches {self.rho[self.finite].max():.3g}"
        rho, n = self.rho[:, None], self.n[:, None]
        self.bound_y = fc.U * np.abs(self.Y) + rho / (1.0 - rho) * self.D + kk * (n + 16) * 2.0 ** -52 * self.B + TINY
        self.bound_lse = fc.U * np.abs(self.LSE) + self.eta + kk * (self.n + 16) * 2.0 ** -52 * (1.0 + np.abs(self.LSE)) + TINY


class BackwardReference(bc.Reference):
    """attention_backward_cases.Reference with the (finite) bias words `b` of one head, and GB with its bound; gradients(), check() and
    rounded() are inherited"""

    def __init__(self, scores, V, gY, lse, scale, b):
        s, sc = scores, float(np.float32(scale))
        b = np.asarray(b, dtype=np.float32)
        assert b.shape == s.S.shape and np.isfinite(b).all()
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
        self.GP = np.array([math.fsum(row) for row in g64.tolist()], dtype=np.float64) if s.exact else g64.sum(axis=1)
        gam = fc.U * np.abs(self.GP) + kk * self.d * 2.0 ** -52 * np.abs(g64).sum(axis=1) + TINY
        T = sc * s.S + b.astype(np.float64)
        assert np.isfinite(T).all()
        eta = (1.0 + fc.U) * abs(sc) * s.delta + fc.U * np.abs(sc * s.S) + TINY      # the existing expression at scale S_e
        eta = (1.0 + fc.U) * eta + fc.U * np.abs(T)                                   # and the rounding of the add
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
        eps1 = rho * P * np.abs(self.GP - Dof) + (1.0 + rho) * P * (gam + eps_d[of])       # eps_e / |scale|
        eps = abs(sc) * eps1
        self.bound_gb = eps1 + fc.U * np.abs(self.GB) + TINY
        self.mag = mag = abs(sc) * P * (np.abs(self.GP) + np.abs(Dof))
        self.GQ, self.GK, self.GV = self.gradients(self.GS, P)
        n, m, pm = self.n[:, None], self.m[:, None], self.perm
        self.bound = {"gq": fc.U * np.abs(self.GQ) + ac._seg_sum(eps[:, None] * np.abs(K64), ip) + kk * (n + 16) * 2.0 ** -52 * ac._seg_sum(mag[:, None] * np.abs(K64), ip) + TINY,
                      "gk": fc.U * np.abs(self.GK) + ac._seg_sum((eps[:, None] * np.abs(Q64))[pm], self.cptr)
                      + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((mag[:, None] * np.abs(Q64))[pm], self.cptr) + TINY,
                      "gv": fc.U * np.abs(self.GV) + ac._seg_sum(((rho * P)[:, None] * np.abs(G64))[pm], self.cptr)
                      + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((P[:, None] * np.abs(G64))[pm], self.cptr) + TINY}
        self.want = {"gq": self.GQ, "gk": self.GK, "gv": self.GV}
        self.empty = {"gq": self.empty_r, "gk": self.empty_c, "gv": self.empty_c}
        self.bad = {"gq": self.bad_r, "gk": self.bad_c, "gv": self.bad_c}

    def check_gbias(self, gb, what, extra=None, want=None):
        """every word of this head's gbias (one per entry); the largest error / bound seen"""
        gb = np.asarray(gb, dtype=np.float32)
        assert gb.shape == self.GB.shape, (what, gb.shape, self.GB.shape)
        assert np.isnan(gb[~self.live]).all(), f"{what}: gbias of an entry of a row with a non-finite lse is not NaN"
        g = gb.astype(np.float64)[self.live]
        assert np.isfinite(g).all(), f"{what}: non-finite words of gbias in rows with a finite lse"
        bound = self.bound_gb if extra is None else self.bound_gb + extra
        ratio = np.abs(g - (self.GB if want is None else want)[self.live]) / bound[self.live]
        worst = float(ratio.max()) if ratio.size else 0.0
        if worst > 1.0:
            i = int(np.nonzero(ratio > 1.0)[0][0])
            e = int(np.nonzero(self.live)[0][i])
            raise AssertionError(f"{what}: {int((ratio > 1.0).sum())} of {ratio.size} words of gbias break the contract, worst error / bound {worst:.3f}, first [{e}]: "
                                 f"got={g[i]!r} want={self.GB[e]!r} bound={bound[e]:.3g}")
        return worst

    def rounded_gbias(self):
        return np.where(self.live, self.GB, np.nan).astype(np.float32)


def forward_refs(scores, V, scale, bias):
    """bias: (nnz, heads) float32"""
    d = V.shape[1] // len(scores)
    return [ForwardReference(s, cut(V, h, d), scale, np.ascontiguousarray(bias[:, h])) for h, s in enumerate(scores)]


def backward_refs(scores, V, gY, lse, scale, bias):
    d = V.shape[1] // len(scores)
    lse = np.asarray(lse, dtype=np.float32)
    assert lse.shape == (scores[0].indptr.size - 1, len(scores))
    return [BackwardReference(s, cut(V, h, d), cut(gY, h, d), np.ascontiguousarray(lse[:, h]), scale, np.ascontiguousarray(bias[:, h])) for h, s in enumerate(scores)]


head_scores, check_forward, check_backward, rounded_forward, rounded_backward = hc.head_scores, hc.check_forward, hc.check_backward, hc.rounded_forward, hc.rounded_backward


def check_gbias(refs, gb, what):
    gb = np.asarray(gb, dtype=np.float32)
    assert gb.shape == (refs[0].GB.size, len(refs)), (what, gb.shape)
    worst = max([r.check_gbias(np.ascontiguousarray(gb[:, h]), f"{what}, head {h}") for h, r in enumerate(refs)] + [0.0])
    print(f"{what}: error / bound = {worst:.3f} (gbias)")
    return worst


def rounded_gbias(refs):
    return np.stack([r.rounded_gbias() for r in refs], axis=1)


def biases(nnz, heads, seed):
    """(nnz, heads) float32, uniform in [-4, 4]"""
    return np.random.default_rng(seed).uniform(-4.0, 4.0, (nnz, heads)).astype(np.float32)


class Plain:
    """the calls WITHOUT a bias on any object, for the forms of heads_cases.py, which call methods (a BiasedMultiHeadAttention's own
    methods take a bias)"""

    def __init__(self, mh):
        self._mh, self.num_rows, self.num_cols = mh, mh.num_rows, mh.num_cols

    def __getattr__(self, name):
        method = getattr(mha.MultiHeadAttention, name)
        return lambda *a, **k: method(self._mh, *a, **k)


class BiasedBF16(heads16.MultiHeadAttentionBF16, mhb.BiasedMultiHeadAttention):
    """an object from hsmhb_create whose methods are the bf16 calls"""


# ---- the forms ---------------------------------------------------------------------------------------------------------------------------
def forward_host(mh, Q, K, V, bias, heads, scale, want_lse=True):
    """(y, lse or None)"""
    if want_lse:
        return mhb.BiasedMultiHeadAttention.forward(mh, Q, K, V, bias, heads, scale)
    return mhb.BiasedMultiHeadAttention.forward(mh, Q, K, V, bias, heads, scale, want_lse=False), None


def _entries_in(mem, a, extra):
    """a (nnz, heads) on the device in rows of heads + extra words, the words h >= heads NaN"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = np.full((a.shape[0], a.shape[1] + extra), NAN_WORD, dtype=np.uint32)
    buf[:, : a.shape[1]] = a.view(np.uint32)
    return mem.alloc(buf), a.shape[1] + extra


def forward_device(mem, mh, Q, K, V, bias, heads, scale, pad=0, extra=0, want_lse=True, what=""):
    """hsmhb_forward_device over fresh buffers: the pads of the inputs (the words h >= heads of bias among them) NaN, y and lse pre-filled
    with a sentinel; the pad words of both must survive"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv) = (wc._features_in(mem, a, pad) for a in (Q, K, V))
    db, ldb = _entries_in(mem, bias, extra)
    ldy, ldl = w + pad, heads + extra
    dy = mem.alloc(np.full((mh.num_rows, ldy), SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full((mh.num_rows, ldl), SENTINEL, dtype=np.uint32)) if want_lse else None
    mhb.BiasedMultiHeadAttention.forward_device(mh, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, db.ptr, ldb, heads, w // heads, scale, dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = wc._features_out(mem, mh, dy, mh.num_rows, w, ldy, what)
    if not want_lse:
        return y, None
    lw = mem.read(mh, dl).reshape(mh.num_rows, ldl)
    assert (lw[:, heads:] == SENTINEL).all(), f"{what}: the pad words of lse were written"
    return y, np.ascontiguousarray(lw[:, :heads]).view(np.float32)


def backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, want_gbias=True):
    """(gq, gk, gv, gbias or None)"""
    return mhb.BiasedMultiHeadAttention.backward(mh, Q, K, V, gY, lse, bias, heads, scale, want_gbias)


def backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, pad=0, extra=0, want_gbias=True, what=""):
    """hsmhb_backward_device over fresh buffers: the pads of the inputs NaN, the four outputs pre-filled with a sentinel; the words h >= heads
    of gbias must survive"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (wc._features_in(mem, a, pad) for a in (Q, K, V, gY))
    dl, ldl = hc._lse_in(mem, lse, extra)
    db, ldb = _entries_in(mem, bias, extra)
    ld, ldgb, nnz = w + pad, heads + extra, bias.shape[0]
    oq = mem.alloc(np.full((mh.num_rows, ld), SENTINEL, dtype=np.uint32))
    ok, ov = (mem.alloc(np.full((mh.num_cols, ld), SENTINEL, dtype=np.uint32)) for _ in range(2))
    ob = mem.alloc(np.full((nnz, ldgb), SENTINEL, dtype=np.uint32)) if want_gbias else None
    mhb.BiasedMultiHeadAttention.backward_device(mh, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, db.ptr, ldb, heads, w // heads, scale, oq.ptr, ld, ok.ptr, ld,
                                                 ov.ptr, ld, ob.ptr if want_gbias else None, ldgb)
    out = tuple(wc._features_out(mem, mh, buf, n, w, ld, f"{what}, {name}") for name, buf, n in (("gq", oq, mh.num_rows), ("gk", ok, mh.num_cols), ("gv", ov, mh.num_cols)))
    if not want_gbias:
        return out + (None,)
    gw = mem.read(mh, ob).reshape(nnz, ldgb)
    assert (gw[:, heads:] == SENTINEL).all(), f"{what}: the words h >= heads of gbias were written"
    return out + (np.ascontiguousarray(gw[:, :heads]).view(np.float32),)


def all_forward_forms(mem, mh, refs, Q, K, V, bias, heads, scale, what):
    """the host form with lse taken and NULL, the device form tight and padded (pad 8, ldl = ldb = heads + 3), the padded one with lse
    NULL too, inside the bounds of one set of references; returns the lse of the host form"""
    y, lse = forward_host(mh, Q, K, V, bias, heads, scale)
    check_forward(refs, y, lse, f"{what}, host form, lse taken")
    check_forward(refs, forward_host(mh, Q, K, V, bias, heads, scale, False)[0], None, f"{what}, host form, lse NULL")
    for pad, extra, want in ((0, 0, True), (8, 3, True), (8, 3, False)):
        tag = f"{what}, device form, pad {pad}, ldl and ldb {heads + extra}, {'lse taken' if want else 'lse NULL'}"
        check_forward(refs, *forward_device(mem, mh, Q, K, V, bias, heads, scale, pad, extra, want, tag), tag)
    return lse


def all_backward_forms(mem, mh, refs, Q, K, V, gY, lse, bias, heads, scale, what):
    """the host form and the device form tight and padded, each with gbias given and with NULL: the same gQ, gK and gV words either way"""
    worst = dict.fromkeys(bc.OUTPUTS + ("gbias",), 0.0)
    for tag, call in ((f"{what}, host form", lambda want: backward_host(mh, Q, K, V, gY, lse, bias, heads, scale, want)),
                      (f"{what}, device form, pad 0", lambda want: backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, 0, 0, want, what)),
                      (f"{what}, device form, pad 8, ld {heads + 3}", lambda want: backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, scale, 8, 3, want, what))):
        gq, gk, gv, gb = call(True)
        w = dict(check_backward(refs, gq, gk, gv, tag), gbias=check_gbias(refs, gb, tag))
        worst = {k: max(worst[k], w[k]) for k in worst}
        without = call(False)
        assert without[3] is None and same_words(without[:3], (gq, gk, gv)), f"{tag}: gbias NULL changes gq, gk or gv"
    return worst


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def general(mem, shapes=SHAPES):
    """300 x 517, 4000 entries, every (heads, d) of heads_cases.SHAPES, scale 0.125, 1 and -2, a bias in [-4, 4]; forward, then backward
    with the lse the forward just wrote"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as mh:
            assert mh.nnz == NNZ
            Q, K, V, gY = operands(shape, heads * d, 9100 + 1000 * heads + d)
            bias = biases(NNZ, heads, 9150 + 1000 * heads + d)
            scores = head_scores(indptr, indices, Q, K, heads)
            for scale in (0.125, 1.0, -2.0):
                what = f"general, {heads} heads of d {d}, scale {scale}"
                lse = all_forward_forms(mem, mh, forward_refs(scores, V, scale, bias), Q, K, V, bias, heads, scale, what)
                w = all_backward_forms(mem, mh, backward_refs(scores, V, gY, lse, scale, bias), Q, K, V, gY, lse, bias, heads, scale, what)
                print(f"{what}: backward worst error / bound = {w['gq']:.3f} (gq), {w['gk']:.3f} (gk), {w['gv']:.3f} (gv), {w['gbias']:.3f} (gbias)")


def edges(mem, heads=3, d=8):
    """every pattern of pattern_cases.edge_patterns() at (3, 8): empty rows and columns, nnz = 0 with NULL indices (bias and gbias are then
    never dereferenced: their buffers hold no word the call may use), unsorted columns, a pair held twice (two entries, two bias words,
    two gbias words)"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as mh:
            assert mh.nnz == indices.size
            Q, K, V, gY = operands(shape, heads * d, 9500)
            bias = biases(indices.size, heads, 9510)
            scores = head_scores(indptr, indices, Q, K, heads)
            fwd = forward_refs(scores, V, 1.5, bias)
            lse = all_forward_forms(mem, mh, fwd, Q, K, V, bias, heads, 1.5, name)
            assert (lse[fwd[0].empty] == -np.inf).all()
            bwd = backward_refs(scores, V, gY, lse, 1.5, bias)
            all_backward_forms(mem, mh, bwd, Q, K, V, gY, lse, bias, heads, 1.5, name)
            if name == "a pair held twice":
                gb = backward_host(mh, Q, K, V, gY, lse, bias, heads, 1.5)[3]
                assert indices[1] == indices[3] and bias[1, 0] != bias[3, 0] and gb.shape == (6, heads) and gb[1, 0] != gb[3, 0]
    # scale = 0: gbias is defined (it carries no factor scale)
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 7)
    shape = (ROWS, COLS)
    with mhb.BiasedMultiHeadAttention((indptr, indices, shape), 4) as mh:
        Q, K, V, gY = operands(shape, 64, 9600)
        bias = biases(NNZ, 4, 9610)
        scores = head_scores(indptr, indices, Q, K, 4)
        y, lse = forward_device(mem, mh, Q, K, V, bias, 4, 0.0, 4, 1, True, "scale 0")
        check_forward(forward_refs(scores, V, 0.0, bias), y, lse, "scale 0")
        bwd = backward_refs(scores, V, gY, lse, 0.0, bias)
        gq, gk, gv, gb = backward_device(mem, mh, Q, K, V, gY, lse, bias, 4, 0.0, 4, 1, True, "scale 0")
        check_backward(bwd, gq, gk, gv, "scale 0")
        check_gbias(bwd, gb, "scale 0")
        assert not (gq != 0).any() and not (gk != 0).any() and (gb != 0).any()


def zero_bias(mem, shapes=((4, 16), (5, 4), (2, 128))):
    """every bias word +0.0: Y, lse, gQ, gK and gV are bit for bit those of hsmh_forward_device and hsmh_backward_device on the same
    object, in both forms; gbias is inside its bound"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as mh:
            Q, K, V, gY = operands(shape, heads * d, 9700 + d)
            zero = np.zeros((NNZ, heads), dtype=np.float32)
            plain = Plain(mh)
            for scale in (0.5, -2.0):
                what = f"zero bias, {heads} heads of d {d}, scale {scale}"
                plain_f = hc.forward_device(mem, plain, Q, K, V, heads, scale, 4, 1, True, what)
                assert same_words(plain_f, forward_device(mem, mh, Q, K, V, zero, heads, scale, 4, 1, True, what)), f"{what}: the forward differs from hsmh_forward_device"
                assert same_words(hc.forward_host(plain, Q, K, V, heads, scale), forward_host(mh, Q, K, V, zero, heads, scale)), f"{what}: the host forward differs"
                lse = plain_f[1]
                plain_b = hc.backward_device(mem, plain, Q, K, V, gY, lse, heads, scale, 4, 1, what)
                got = backward_device(mem, mh, Q, K, V, gY, lse, zero, heads, scale, 4, 1, True, what)
                assert same_words(plain_b, got[:3]), f"{what}: the backward differs from hsmh_backward_device"
                assert same_words(hc.backward_host(plain, Q, K, V, gY, lse, heads, scale), backward_host(mh, Q, K, V, gY, lse, zero, heads, scale)[:3]), f"{what}: the host backward differs"
                check_gbias(backward_refs(head_scores(indptr, indices, Q, K, heads), V, gY, lse, scale, zero), got[3], what)


def mask(mem, heads=4, d=16):
    """A random third of the entries at -inf in every head (at least one entry of every row kept): Y, lse, gQ, gK, gV and the kept words
    of gbias agree with the reference over the pattern WITHOUT those entries and the remaining bias; the masked words of gbias are zero.
    Then, forward only, head 1 of one row fully masked as well: that head of that row is a dead row (Y NaN, lse -inf), its other heads
    and every other row stay inside the bounds of the reference."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 6)
    shape = (ROWS, COLS)
    rng = np.random.default_rng(9800)
    of = pc.entry_rows(indptr)
    masked = rng.random(NNZ) < 1.0 / 3.0
    masked[indptr[:-1][np.diff(indptr.astype(np.int64)) > 0]] = False      # the first entry of every row stays
    keep = ~masked
    assert NNZ // 4 < masked.sum() < NNZ // 2
    kptr = np.zeros(ROWS + 1, dtype=np.uint32)
    kptr[1:] = np.cumsum(np.bincount(of[keep], minlength=ROWS))
    kidx = indices[keep]
    Q, K, V, gY = operands(shape, heads * d, 9810)
    bias = biases(NNZ, heads, 9820)
    scale = 0.5
    scores = head_scores(kptr, kidx, Q, K, heads)
    fwd = forward_refs(scores, V, scale, bias[keep])
    with_mask = bias.copy()
    with_mask[masked] = -np.inf
    with mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as mh:
        for form in ("host", "device"):
            what = f"mask, {form} form"
            y, lse = forward_host(mh, Q, K, V, with_mask, heads, scale) if form == "host" else forward_device(mem, mh, Q, K, V, with_mask, heads, scale, 4, 1, True, what)
            check_forward(fwd, y, lse, what)
            bwd = backward_refs(scores, V, gY, lse, scale, bias[keep])
            got = backward_host(mh, Q, K, V, gY, lse, with_mask, heads, scale) if form == "host" else backward_device(mem, mh, Q, K, V, gY, lse, with_mask, heads, scale, 4, 1, True, what)
            check_backward(bwd, *got[:3], what)
            check_gbias(bwd, got[3][keep], what)
            assert not (got[3][masked] != 0).any(), f"{what}: a masked entry's gbias word is not zero"
        # head 1 of one row fully masked
        n = np.diff(indptr.astype(np.int64))
        r0 = int(np.nonzero(n >= 5)[0][3])
        one = with_mask.copy()
        one[indptr[r0]: indptr[r0 + 1], 1] = -np.inf
        refs = forward_refs(head_scores(indptr, indices, Q, K, heads), V, scale, one)      # over the whole pattern: the forward reference takes -inf scores
        assert refs[1].dead[r0] and refs[1].dead.sum() == 1 and not any(r.dead.any() for h, r in enumerate(refs) if h != 1)
        for y, lse in (forward_host(mh, Q, K, V, one, heads, scale), forward_device(mem, mh, Q, K, V, one, heads, scale, 4, 1, True, "one head of a row masked")):
            check_forward(refs, y, lse, "one head of a row masked")
            assert np.isnan(y[r0, d: 2 * d]).all() and lse[r0, 1] == -np.inf
            assert np.isfinite(np.delete(y[r0], np.s_[d: 2 * d])).all() and np.isfinite(np.delete(lse[r0], 1)).all()
            kept_rows = fwd[0].finite.copy()
            kept_rows[r0] = False
            for h in range(heads):      # and the rest is what the masked pattern alone gives
                assert (np.abs(cut(y, h, d).astype(np.float64) - fwd[h].Y)[kept_rows] <= fwd[h].bound_y[kept_rows]).all()


def heads_do_not_leak(mem, shapes=((4, 16), (5, 4))):
    """a NaN bias word in head 1 of one entry and a +inf bias word in head 1 of another: forward, head 1 of the two rows is NaN in Y and
    lse and every other word is inside the bounds of the reference; backward, with the lse words that forward writes, head 1 of the
    two rows is NaN in gQ, of the columns the rows touch in gK and gV and of the rows' entries in gbias, and every other word of every
    output is finite and inside the bounds of the reference (which takes the two words as 0: they belong to rows whose lse is NaN)."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    n = np.diff(indptr.astype(np.int64))
    of = pc.entry_rows(indptr)
    r_nan, r_inf = (int(r) for r in np.nonzero(n >= 3)[0][[2, 40]])
    e_nan, e_inf = int(indptr[r_nan]) + 1, int(indptr[r_inf]) + 2
    scale = 0.5
    for heads, d in shapes:
        h1 = slice(d, 2 * d)
        with mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as mh:
            Q, K, V, gY = operands(shape, heads * d, 9900 + d)
            clean = biases(NNZ, heads, 9910 + d)
            clean[[e_nan, e_inf], 1] = 0.0
            planted = clean.copy()
            planted[e_nan, 1], planted[e_inf, 1] = np.nan, np.inf
            scores = head_scores(indptr, indices, Q, K, heads)
            refs = forward_refs(scores, V, scale, planted)
            assert refs[1].bad.sum() == 2 and refs[1].bad[[r_nan, r_inf]].all() and not any(r.bad.any() for h, r in enumerate(refs) if h != 1)
            what = f"heads do not leak, forward, {heads} heads of d {d}"
            for y, lse in (forward_host(mh, Q, K, V, planted, heads, scale), forward_device(mem, mh, Q, K, V, planted, heads, scale, 4, 1, True, what)):
                check_forward(refs, y, lse, what)
                assert np.isnan(y[[r_nan, r_inf], h1]).all() and np.isnan(lse[[r_nan, r_inf], 1]).all()
                assert np.isfinite(np.delete(y, np.s_[d: 2 * d], axis=1)[n > 0]).all() and np.isfinite(np.delete(lse, 1, axis=1)[n > 0]).all()
            # backward, with the lse that forward writes (NaN in head 1 of the two rows) and the planted bias
            lse = rounded_forward(refs)[1]
            brefs = backward_refs(scores, V, gY, lse, scale, clean)
            assert brefs[1].bad_r.sum() == 2 and 2 <= brefs[1].bad_c.sum() < COLS // 4 and not any(r.bad_r.any() for h, r in enumerate(brefs) if h != 1)
            what = f"heads do not leak, backward, {heads} heads of d {d}"
            for gq, gk, gv, gb in (backward_host(mh, Q, K, V, gY, lse, planted, heads, scale), backward_device(mem, mh, Q, K, V, gY, lse, planted, heads, scale, 4, 1, True, what)):
                check_backward(brefs, gq, gk, gv, what)
                check_gbias(brefs, gb, what)
                assert np.isnan(gb[brefs[1].bad_r[of], 1]).all()
                for a in (gq, gk, gv, gb):
                    assert np.isfinite(np.delete(a, np.s_[d: 2 * d] if a is not gb else 1, axis=1)).all(), f"{what}: a bias word of head 1 reached another head"


def long_pattern(n):
    """n x n: row 5 holds 600 entries and column 7 holds 700 (each more than 512: a workgroup of its own and the merge of its four
    wavefronts through LDS), 1500 more entries lie in short rows and columns, every other row and column is empty"""
    rng = np.random.default_rng(10000)
    pairs = {(5, int(c)) for c in rng.choice(n, 600, replace=False)} | {(int(r), 7) for r in rng.choice(n, 700, replace=False)}
    pairs |= {(int(r), int(c)) for r, c in zip(rng.integers(0, n, 1500), rng.integers(0, n, 1500))}
    flat = np.sort(np.array([r * n + c for r, c in pairs], dtype=np.int64))
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(np.bincount(flat // n, minlength=n))
    indices = (flat % n).astype(np.uint32)
    assert np.diff(indptr.astype(np.int64)).max() > 512 and np.bincount(indices, minlength=n).max() > 512 and indices.size < 3000
    return indptr, indices


def long_rows_and_columns(mem, n, shapes=((4, 16), (3, 8))):
    """the device forms over long_pattern(n), forward then backward with the lse just written, float64 sums in the references (exact=False)
    as the existing large cases; n is chosen by the caller so that the grid's stride loop runs"""
    indptr, indices = long_pattern(n)
    shape = (n, n)
    for heads, d in shapes:
        what = f"long row and column among {n}, {heads} heads of d {d}"
        Q, K, V, gY = operands(shape, heads * d, 10100 + d)
        bias = biases(indices.size, heads, 10110 + d)
        scores = head_scores(indptr, indices, Q, K, heads, exact=False)
        with mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as mh:
            y, lse = forward_device(mem, mh, Q, K, V, bias, heads, 0.5, 4, 1, True, what)
            check_forward(forward_refs(scores, V, 0.5, bias), y, lse, what)
            bwd = backward_refs(scores, V, gY, lse, 0.5, bias)
            gq, gk, gv, gb = backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, 0.5, 4, 1, True, what)
            check_backward(bwd, gq, gk, gv, what)
            check_gbias(bwd, gb, what)
            assert same_words((gq, gk, gv, gb), backward_device(mem, mh, Q, K, V, gY, lse, bias, heads, 0.5, 4, 1, True, what)), f"{what}: two calls give other words"


def objects(mem, heads=4, d=16):
    """Which object takes which call.  An object from plain hsmh_create: the forward with a bias works, the backward with a bias is
    HS_ERR_BAD_ARG with a message that names hsmhb_create, and the object stays usable.  An object from hsmhb_create: both work, and
    it serves the hsmh_* and hsmh16_* calls with the words a plain object gives.  hsmh_info: hsmh_create's formula plus 4 max(nnz, 1)
    with HSMH_BACKWARD on the device, nothing on the host."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 5)
    shape = (ROWS, COLS)
    Q, K, V, gY = operands(shape, heads * d, 10200)
    bias = biases(NNZ, heads, 10210)
    scores = head_scores(indptr, indices, Q, K, heads)
    fwd = forward_refs(scores, V, 0.25, bias)
    on_device = isinstance(mem, HipMemory)
    with mha.MultiHeadAttention((indptr, indices, shape), heads) as plain, mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads) as full, \
            mhb.BiasedMultiHeadAttention((indptr, indices, shape), heads, backward=False) as no_flag:
        y, lse = forward_host(plain, Q, K, V, bias, heads, 0.25)
        check_forward(fwd, y, lse, "forward on an object from hsmh_create")
        check_forward(fwd, *forward_device(mem, plain, Q, K, V, bias, heads, 0.25, 4, 1, True, "plain object"), "forward_device on an object from hsmh_create")
        assert same_words((y, lse), forward_host(full, Q, K, V, bias, heads, 0.25)) and same_words((y, lse), forward_host(no_flag, Q, K, V, bias, heads, 0.25))
        for obj in (plain, no_flag):
            for call in (lambda: backward_host(obj, Q, K, V, gY, lse, bias, heads, 0.25), lambda: backward_device(mem, obj, Q, K, V, gY, lse, bias, heads, 0.25)):
                try:
                    call()
                except mha.DeviceError as e:
                    assert e.code == BAD_ARG and "hsmhb_create" in str(e), str(e)
                else:
                    raise AssertionError("the backward with a bias ran on an object without the entry map")
            assert same_words((y, lse), forward_host(obj, Q, K, V, bias, heads, 0.25)), "unusable after the refused backward"
        bwd = backward_refs(scores, V, gY, lse, 0.25, bias)
        got = backward_host(full, Q, K, V, gY, lse, bias, heads, 0.25)
        check_backward(bwd, *got[:3], "backward on an object from hsmhb_create")
        check_gbias(bwd, got[3], "backward on an object from hsmhb_create")
        # the calls without a bias, fp32 and bf16, on both objects: the same words
        base = mha.MultiHeadAttention
        pf = base.forward(plain, Q, K, V, heads, 0.25)
        assert same_words(pf, base.forward(full, Q, K, V, heads, 0.25))
        assert same_words(base.backward(plain, Q, K, V, gY, pf[1], heads, 0.25), base.backward(full, Q, K, V, gY, pf[1], heads, 0.25))
        assert same_words(hc.forward_device(mem, plain, Q, K, V, heads, 0.25, 4, 1), hc.forward_device(mem, Plain(full), Q, K, V, heads, 0.25, 4, 1))
        assert same_words(hc.backward_device(mem, plain, Q, K, V, gY, pf[1], heads, 0.25, 4, 1), hc.backward_device(mem, Plain(full), Q, K, V, gY, pf[1], heads, 0.25, 4, 1))
        check_forward(hc.forward_refs(scores, V, 0.25), *pf, "hsmh_forward on an object from hsmhb_create")
        q16, k16, v16, g16 = (heads16.to_bf16(a) for a in (Q, K, V, gY))
        with heads16.MultiHeadAttentionBF16((indptr, indices, shape), heads) as p16, BiasedBF16((indptr, indices, shape), heads) as f16:
            assert f16.entry_map and f16.info() == full.info()
            y16, l16 = p16.forward(q16, k16, v16, heads, 0.25)
            y16f, l16f = f16.forward(q16, k16, v16, heads, 0.25)
            assert np.array_equal(y16, y16f) and same_words((l16,), (l16f,))
            assert all(np.array_equal(a, b) for a, b in zip(p16.backward(q16, k16, v16, g16, l16, heads, 0.25), f16.backward(q16, k16, v16, g16, l16, heads, 0.25)))
            got16 = backward_host(f16, Q, K, V, gY, lse, bias, heads, 0.25)      # and the same object still takes the calls with a bias
            assert same_words(got16, got)
        # hsmh_info
        forward_bytes = 4 * (ROWS + 1) + 4 * NNZ + 4 * ROWS
        backward_bytes = forward_bytes + 4 * (COLS + 1) + 4 * NNZ + 4 * COLS + 8 * ROWS * heads
        want = {plain: backward_bytes, full: backward_bytes + 4 * NNZ, no_flag: forward_bytes}
        for obj, nbytes in want.items():
            assert obj.info() == {"nnz": NNZ, "device_bytes": nbytes if on_device else 0}, (obj.info(), nbytes)
    with mhb.BiasedMultiHeadAttention((np.zeros(6, dtype=np.uint32), np.zeros(0, dtype=np.uint32), (5, 7)), 3) as empty:
        assert empty.info() == {"nnz": 0, "device_bytes": (4 * 6 + 4 + 4 * 5 + 4 * 8 + 4 + 4 * 7 + 8 * 5 * 3 + 4) if on_device else 0}


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
FEATURES = hc.FEATURES


def refusals(mem):
    """every breach of the layout rules of bias and gbias is HS_ERR_BAD_ARG with a message, and the object stays usable"""
    l = mhb.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    heads, d = 2, 4
    w = heads * d
    one = np.zeros(4, dtype=np.float32).ctypes.data
    assert l.hsmhb_forward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 1, 1, 4, 1.0, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsmhb_forward(None, vp(one), vp(one), vp(one), vp(one), 1, 4, 1.0, vp(one), None) == BAD_ARG
    assert l.hsmhb_backward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 1, vp(one), 1, 1, 4, 1.0, vp(one), 4, vp(one), 4, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsmhb_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), vp(one), 1, 4, 1.0, vp(one), vp(one), vp(one), None) == BAD_ARG
    h = C.c_void_p(0xBAD)      # hsmhb_create refuses what hsmh_create refuses, with its codes and its message
    assert l.hsmhb_create(C.byref(h), 0, 6, 9, indptr.ctypes.data, indices.ctypes.data, 4, 2) == BAD_ARG and not h.value and b"HSMH_BACKWARD" in l.hsmh_last_error(None)
    h = C.c_void_p(0xBAD)
    assert l.hsmhb_create(C.byref(h), 0, 6, 9, indptr.ctypes.data, indices.ctypes.data, 65, 1) == BAD_ARG and not h.value
    bad_index = indices.copy()
    bad_index[3] = 9
    assert l.hsmhb_create(C.byref(h), 0, 6, 9, indptr.ctypes.data, bad_index.ctypes.data, 4, 1) == -4 and not h.value
    assert l.hsmhb_create(None, 0, 6, 9, indptr.ctypes.data, indices.ctypes.data, 4, 1) == BAD_ARG
    with mhb.BiasedMultiHeadAttention((indptr, indices, shape), 4) as mh:
        Q, K, V, gY = operands(shape, w, 10300)
        bias = biases(7, heads, 10310)
        want_f = forward_host(mh, Q, K, V, bias, heads, 0.5)
        scores = head_scores(indptr, indices, Q, K, heads)
        check_forward(forward_refs(scores, V, 0.5, bias), *want_f, "refusals")
        want_b = backward_host(mh, Q, K, V, gY, want_f[1], bias, heads, 0.5)
        brefs = backward_refs(scores, V, gY, want_f[1], 0.5, bias)
        check_backward(brefs, *want_b[:3], "refusals")
        check_gbias(brefs, want_b[3], "refusals")

        def still_usable(rc, what):
            assert rc == BAD_ARG and l.hsmh_last_error(mh._h), (what, rc)
            assert same_words(forward_host(mh, Q, K, V, bias, heads, 0.5), want_f), f"unusable after {what}"
            assert same_words(backward_host(mh, Q, K, V, gY, want_f[1], bias, heads, 0.5), want_b), f"unusable after {what}"

        def forward_call(a):
            return l.hsmhb_forward_device(mh._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["bias"]), a["ldb"], a["heads"], a["d"], a["scale"], vp(a["y"]),
                                          a["ldy"], vp(a["lse"]), a["ldl"])

        def backward_call(a):
            return l.hsmhb_backward_device(mh._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["ldl"], vp(a["bias"]), a["ldb"],
                                           a["heads"], a["d"], a["scale"], vp(a["gq"]), a["ldgq"], vp(a["gk"]), a["ldgk"], vp(a["gv"]), a["ldgv"], vp(a["gbias"]), a["ldgb"])

        # buffers of 9 rows x 16 words, 16-byte aligned: larger than any operand; bias and gbias use 7 rows of up to 4 words of theirs
        names = FEATURES + ("y", "lse", "bias", "gbias")
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 8 for name in FEATURES + ("y",)}, heads=heads, d=d, scale=1.0, ldl=2, ldb=2, ldgb=2)
        assert forward_call(ok) == 0 and backward_call(ok) == 0 and backward_call(dict(ok, gbias=None, ldgb=0)) == 0
        for what, change in (("null bias", dict(bias=None)), ("misaligned bias", dict(bias=ok["bias"] + 2)), ("ldb < heads", dict(ldb=1)), ("ldb = 0", dict(ldb=0)),
                             ("y is bias", dict(y=ok["bias"])), ("bias inside y", dict(bias=ok["y"] + 16)), ("lse is bias", dict(lse=ok["bias"])),
                             ("lse over the last bias word", dict(lse=ok["bias"] + (6 * 2 + 1) * 4))):
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("null bias", dict(bias=None)), ("misaligned bias", dict(bias=ok["bias"] + 2)), ("ldb < heads", dict(ldb=1)), ("misaligned gbias", dict(gbias=ok["gbias"] + 2)),
                  ("ldgb < heads", dict(ldgb=1)), ("ldgb = 0", dict(ldgb=0)), ("gbias over the last bias word", dict(gbias=ok["bias"] + (6 * 2 + 1) * 4)),
                  ("gq is bias", dict(gq=ok["bias"])), ("gk is bias", dict(gk=ok["bias"])), ("gv inside bias", dict(gv=ok["bias"] + 16))]
        bcases += [(f"gbias is {name}", dict(gbias=ok[name])) for name in ("q", "k", "v", "gy", "lse", "bias", "gq", "gk", "gv")]
        bcases += [(f"gbias inside {name}", dict(gbias=ok[name] + 16)) for name in ("q", "gq", "gv")]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        # the rules of the plain calls hold as they did
        for what, change in (("d = 5", dict(heads=1, d=5)), ("heads > max_heads", dict(heads=5)), ("scale NaN", dict(scale=float("nan"))), ("null q", dict(q=None)),
                             ("ldl < heads", dict(ldl=1))):
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        still_usable(backward_call(dict(ok, gq=ok["q"])), "backward_device: gq is q")
        # ranges that touch without sharing a byte are fine: gbias right behind bias's 7 entries, bias right behind lse's 6 rows
        assert backward_call(dict(ok, gbias=ok["bias"] + 7 * 2 * 4)) == 0
        assert forward_call(dict(ok, bias=ok["lse"] + 6 * 2 * 4)) == 0
        # the host forms
        host = {name: np.zeros(9 * 8, np.float32) for name in names}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, heads=heads, d=d, scale=1.0)

        def forward_host_call(a):
            return l.hsmhb_forward(mh._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["bias"]), a["heads"], a["d"], a["scale"], vp(a["y"]), vp(a["lse"]))

        def backward_host_call(a):
            return l.hsmhb_backward(mh._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), vp(a["bias"]), a["heads"], a["d"], a["scale"], vp(a["gq"]), vp(a["gk"]),
                                    vp(a["gv"]), vp(a["gbias"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0 and backward_host_call(dict(okh, gbias=None)) == 0
        for what, change in (("null bias", dict(bias=None)), ("y is bias", dict(y=okh["bias"])), ("lse inside bias", dict(lse=okh["bias"] + 8)), ("d = 6", dict(d=6))):
            still_usable(forward_host_call(dict(okh, **change)), "forward: " + what)
        for what, change in (("null bias", dict(bias=None)), ("gbias is bias", dict(gbias=okh["bias"])), ("gbias is gk", dict(gbias=okh["gk"])), ("gbias inside q", dict(gbias=okh["q"] + 8)),
                             ("gq is bias", dict(gq=okh["bias"])), ("null lse", dict(lse=None))):
            still_usable(backward_host_call(dict(okh, **change)), "backward: " + what)
        mh.set_stream(None)
        mh.sync()
