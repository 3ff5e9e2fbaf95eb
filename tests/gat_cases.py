"""The cases of the graph attention (GAT) calls (include/hisparse_gat.h), shared by tests/test_gat_cpu.py (libhisparse_cpu.so, in a child
process) and tests/test_gpu_gat.py (the HIP library, on the device), written against the memory interface of tests/pattern_cases.py.

Reference, one per head, from the header's formulas and BOUNDS.  x = el[row(e)] + er[col(e)] and t = x > 0 ? x : slope * x are formed in
numpy float32, exactly the two fp32 operations of the contract, so a score carries no error term; everything else is float64.  With
u = 2^-24 and rho = expm1(32 * 2^-52):
    forward    M = max t, E = exp(t - M), L = sum E, P = E / L, Y_j = sum P V_j, LSE = M + log L
               |y - Y|     <= u|Y| + rho/(1-rho) sum P|V - Y| + (n_r + 16) 2^-52 sum P|V| + 2^-149
               |lse - LSE| <= u|LSE| + (n_r + 16) 2^-52 (1 + |LSE|) + 2^-149
    backward   P = exp(t - lse[row(e)]) with the lse WORDS AS GIVEN, GP = sum_j fl32(gY_j V_j), D_r = sum P GP, dx = x > 0 ? 1 : slope,
               GX = P (GP - D) dx, gel = sum_r GX, ger = sum_c GX, gV = sum_c P gY
               gam_e  = u|GP_e| + d 2^-52 A'_e + 2^-149        epsD_r = sum_r P(rho|GP| + (1+rho) gam) + (n_r+16) 2^-52 sum_r P|GP|
               eps_e  = rho P|GP - D| + (1+rho) P (gam_e + epsD_r)          mag_e = P(|GP| + |D|)
               |gel - GEL| <= u|GEL| + sum_r eps_e dx_e + (n_r + 16) 2^-52 sum_r mag_e dx_e + 2^-149,   ger the same over the column with m_c
               |gv - GV|   <= u|GV| + sum_c rho P|gY| + (m_c + 16) 2^-52 sum_c P|gY| + 2^-149
These are the bounds of attention_cases.Reference and attention_backward_cases.Reference at scale = 1 and eta_e = 0 with the feature word
that multiplies GS_e replaced by dx_e; no tolerance is introduced here.  Sums are math.fsum with exact=True; exact=False (float64 sums,
the 2^-52 terms doubled) is used by the large cases of the GPU tests only.  The special tables are asserted bit for bit: a row without
entries +0.0 in Y and gel and -inf in lse, a column without entries +0.0 in ger and gV, a NaN or +inf x NaN in Y and lse, only -inf NaN
and -inf, a non-finite lse word NaN in gel[r] and in ger[c] and gV[c] of every column the row touches."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import gat, heads as mha

import attention_cases as ac
import float_contract as fc
import heads_cases as hc
import pattern_cases as pc
import wide_cases as wc
from pattern_cases import HipMemory, HostMemory, edge_patterns, entry_rows, random_pattern  # noqa: F401

BAD_ARG = -1
SENTINEL, NAN_WORD = wc.SENTINEL, wc.NAN_WORD
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
SHAPES = hc.SHAPES
SLOPES = (0.2, 0.0, 1.0)
RHO = math.expm1(32.0 * 2.0 ** -52)
TINY = 2.0 ** -149
OUTPUTS = ("gel", "ger", "gv")


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def leaky(x, slope):
    """t = x > 0 ? x : fl32(slope * x) over float32 words; x == 0 and NaN take the slope branch"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.where(x > 0, x, np.float32(slope) * x).astype(np.float32)


class Reference(ac.Reference):
    """One head's forward: el (rows,), er (cols,), V (cols, d), all float32.  check() and rounded() are attention_cases.Reference's, which
    read the fields set here (eta is 0: a score has no error term)."""

    def __init__(self, indptr, indices, el, er, V, slope, exact=True):
        assert el.dtype == er.dtype == V.dtype == np.float32 and el.ndim == er.ndim == 1 and V.shape[0] == er.size
        self.indptr, self.indices = ip, ix = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        assert el.size == ip.size - 1
        self.of, self.exact, self.d, self.V, self.slope = entry_rows(ip), exact, V.shape[1], V, np.float32(slope)
        of = self.of
        self.n = np.diff(ip)
        kk = 1.0 if exact else 2.0
        seg = ac._seg_fsum if exact else ac._seg_sum
        with np.errstate(all="ignore"):
            self.x = (el[of] + er[ix]).astype(np.float32)                      # one fp32 add
            self.t = leaky(self.x, slope)                                      # one fp32 multiply
            self.dx = np.where(self.x > 0, 1.0, float(np.float32(slope)))
            self.fin = np.isfinite(self.t)
            neg = np.isneginf(self.t)
            bad = ~self.fin & ~neg                                             # NaN or +inf
            T = np.where(self.fin, self.t.astype(np.float64), -np.inf)
            self.T = T
            self.empty = self.n == 0
            self.bad = ac._seg_sum(bad[:, None].astype(np.float64), ip)[:, 0] > 0
            self.dead = ~self.empty & ~self.bad & (ac._seg_sum(self.fin[:, None].astype(np.float64), ip)[:, 0] == 0)
            self.finite = ~self.empty & ~self.bad & ~self.dead
            self.M = ac._seg_max(T, ip, -np.inf)
            live = self.finite[of]
            E = np.where(live, np.exp(T - np.where(live, self.M[of], 0.0)), 0.0)
            V64 = V.astype(np.float64)[ix]
            self.L = seg(E[:, None], ip)[:, 0]
            Lsafe = np.where(self.finite, self.L, 1.0)
            self.P = E / Lsafe[of]
            self.Y = seg(E[:, None] * V64, ip) / Lsafe[:, None]
            self.D = ac._seg_sum(self.P[:, None] * np.abs(V64 - self.Y[of]), ip)
            self.B = ac._seg_sum(self.P[:, None] * np.abs(V64), ip)
            self.LSE = np.where(self.finite, self.M, 0.0) + np.log(Lsafe)
        self.eta = np.zeros(self.n.size)
        self.rho = np.full(self.n.size, RHO)
        n = self.n[:, None]
        self.bound_y = fc.U * np.abs(self.Y) + RHO / (1.0 - RHO) * self.D + kk * (n + 16) * 2.0 ** -52 * self.B + TINY
        self.bound_lse = fc.U * np.abs(self.LSE) + kk * (self.n + 16) * 2.0 ** -52 * (1.0 + np.abs(self.LSE)) + TINY

    def backward(self, gY, lse):
        return Backward(self, gY, lse)


class Backward:
    """One head's backward from a Reference's scores, gY (rows, d) and the lse words (rows,) float32 as the call is given them.  gel and ger
    are kept as (n, 1) arrays so that the three outputs are checked by one loop."""

    def __init__(self, f, gY, lse):
        V = f.V
        assert gY.dtype == np.float32 and gY.shape == (f.n.size, f.d)
        lse = np.asarray(lse, dtype=np.float32)
        assert lse.shape == (f.n.size,)
        ip, ix, of = f.indptr, f.indices, f.of
        assert not (~f.fin & ~np.isneginf(f.t)).any(), "the backward cases hold no NaN or +inf score"
        self.f, self.d = f, f.d
        kk = 1.0 if f.exact else 2.0
        self.seg = seg = ac._seg_fsum if f.exact else ac._seg_sum
        self.n = f.n
        self.perm = pm = np.argsort(ix, kind="stable")
        self.m = np.bincount(ix, minlength=V.shape[0]).astype(np.int64)
        self.cptr = cptr = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.empty_r, self.empty_c = self.n == 0, self.m == 0
        self.bad_r = ~self.empty_r & ~np.isfinite(lse)
        self.bad_c = np.zeros(V.shape[0], dtype=bool)
        self.bad_c[ix[self.bad_r[of]]] = True
        live = ~self.bad_r[of]
        g64 = (gY[of] * V[ix]).astype(np.float64)                                # one fp32 multiply per product
        self.GP = GP = np.array([math.fsum(row) for row in g64.tolist()], dtype=np.float64) if f.exact else g64.sum(axis=1)
        gam = fc.U * np.abs(GP) + kk * self.d * 2.0 ** -52 * np.abs(g64).sum(axis=1) + TINY
        with np.errstate(all="ignore"):
            self.P = P = np.where(live, np.exp(f.T - np.where(live, lse.astype(np.float64)[of], 0.0)), 0.0)      # a -inf score weighs exactly 0
        assert np.isfinite(P).all()
        self.dx = dx = f.dx
        self.G64 = G64 = gY.astype(np.float64)[of]
        self.D = seg((P * GP)[:, None], ip)[:, 0]
        Dof = self.D[of]
        eps_d = ac._seg_sum((P * (RHO * np.abs(GP) + (1.0 + RHO) * gam))[:, None], ip)[:, 0] + kk * (self.n + 16) * 2.0 ** -52 * ac._seg_sum((P * np.abs(GP))[:, None], ip)[:, 0]
        self.GX = GX = P * (GP - Dof) * dx
        self.eps = eps = RHO * P * np.abs(GP - Dof) + (1.0 + RHO) * P * (gam + eps_d[of])
        self.mag = mag = P * (np.abs(GP) + np.abs(Dof))
        self.GEL, self.GER, self.GV = self.gradients(GX, P)
        n, m = self.n[:, None], self.m[:, None]
        self.bound = {"gel": fc.U * np.abs(self.GEL) + ac._seg_sum((eps * dx)[:, None], ip) + kk * (n + 16) * 2.0 ** -52 * ac._seg_sum((mag * dx)[:, None], ip) + TINY,
                      "ger": fc.U * np.abs(self.GER) + ac._seg_sum((eps * dx)[pm][:, None], cptr) + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((mag * dx)[pm][:, None], cptr) + TINY,
                      "gv": fc.U * np.abs(self.GV) + ac._seg_sum((RHO * P[:, None] * np.abs(G64))[pm], cptr)
                      + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((P[:, None] * np.abs(G64))[pm], cptr) + TINY}
        self.want = {"gel": self.GEL, "ger": self.GER, "gv": self.GV}
        self.empty = {"gel": self.empty_r, "ger": self.empty_c, "gv": self.empty_c}
        self.bad = {"gel": self.bad_r, "ger": self.bad_c, "gv": self.bad_c}

    def gradients(self, GX, P):
        """(gel (rows, 1), ger (cols, 1), gV (cols, d)) in float64 from per-entry gx and p, by this reference's sums"""
        pm = self.perm
        return self.seg(GX[:, None], self.f.indptr), self.seg(GX[pm][:, None], self.cptr), self.seg((P[:, None] * self.G64)[pm], self.cptr)

    def check(self, gel, ger, gv, what, extra=None):
        """every word of the three outputs (gel (rows,), ger (cols,), gv (cols, d)); returns the largest error / bound per output"""
        worst = {}
        for name, got in zip(OUTPUTS, (gel, ger, gv)):
            got = np.asarray(got, dtype=np.float32)
            got = got.reshape(got.shape[0], -1)
            want, bound, empty, bad = self.want[name], self.bound[name], self.empty[name], self.bad[name]
            if extra is not None:
                bound = bound + extra[name]
            assert got.shape == want.shape, (what, name, got.shape, want.shape)
            assert not got.view(np.uint32)[empty].any(), f"{what}: {name} of a {'row' if name == 'gel' else 'column'} without entries is not +0.0"
            assert np.isnan(got[bad]).all(), f"{what}: {name} is not NaN in every word that a row with a non-finite lse reaches"
            g = got.astype(np.float64)[~bad]
            assert np.isfinite(g).all(), f"{what}: non-finite words of {name} where no row with a non-finite lse reaches"
            ratio = np.abs(g - want[~bad]) / bound[~bad]
            worst[name] = float(ratio.max()) if ratio.size else 0.0
            if worst[name] > 1.0:
                i, j = (int(k[0]) for k in np.nonzero(ratio > 1.0))
                r = int(np.nonzero(~bad)[0][i])
                raise AssertionError(f"{what}: {int((ratio > 1.0).sum())} of {ratio.size} words of {name} break the contract, worst error / bound {worst[name]:.3f}, "
                                     f"first [{r}][{j}]: got={g[i, j]!r} want={want[r, j]!r} bound={bound[r, j]:.3g}")
        print(f"{what}: error / bound = {worst['gel']:.3f} (gel), {worst['ger']:.3f} (ger), {worst['gv']:.3f} (gv)")
        return worst

    def rounded(self, grads=None):
        """a correct result: the reference's own words rounded once, (gel (rows,), ger (cols,), gv (cols, d))"""
        out = [np.where(self.bad[name][:, None], np.nan, x).astype(np.float32) for name, x in zip(OUTPUTS, grads or (self.GEL, self.GER, self.GV))]
        return out[0][:, 0], out[1][:, 0], out[2]


cut = hc.cut


def col(a, h):
    """head h's word of a head array, contiguous"""
    return np.ascontiguousarray(a[:, h])


def forward_refs(indptr, indices, EL, ER, V, slope, exact=True):
    heads = EL.shape[1]
    d = V.shape[1] // heads
    assert ER.shape[1] == heads and V.shape[1] == heads * d
    return [Reference(indptr, indices, col(EL, h), col(ER, h), cut(V, h, d), slope, exact) for h in range(heads)]


def backward_refs(frefs, gY, lse):
    """lse: (rows, heads) float32, the words the backward call is given"""
    d = frefs[0].d
    lse = np.asarray(lse, dtype=np.float32)
    assert lse.shape == (frefs[0].n.size, len(frefs))
    return [f.backward(cut(gY, h, d), col(lse, h)) for h, f in enumerate(frefs)]


check_forward = hc.check_forward
rounded_forward = hc.rounded_forward


def check_backward(refs, gel, ger, gv, what):
    d = refs[0].d
    gel, ger, gv = (np.asarray(a, dtype=np.float32) for a in (gel, ger, gv))
    assert gel.shape == (refs[0].n.size, len(refs)) and ger.shape == (refs[0].m.size, len(refs)) and gv.shape == (refs[0].m.size, len(refs) * d), (what, gel.shape, ger.shape, gv.shape)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for h, r in enumerate(refs):
        w = r.check(col(gel, h), col(ger, h), cut(gv, h, d), f"{what}, head {h}")
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


def rounded_backward(refs, grads=None):
    parts = [r.rounded(None if grads is None else grads[h]) for h, r in enumerate(refs)]
    return np.stack([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1), np.concatenate([p[2] for p in parts], axis=1)


# ---- inputs and the forms ------------------------------------------------------------------------------------------------------------
def operands(shape, indptr, indices, heads, d, seed):
    """EL (rows, heads), ER (cols, heads), V (cols, heads d), gY (rows, heads d).  er is normal; el of a row with two entries or more lies
    between minus the largest and minus the smallest er word of the row's columns, so that x takes both signs in that row whenever those
    two words differ; el of the other rows is normal."""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    ER = rng.normal(0.0, 1.0, (cols, heads)).astype(np.float32)
    EL = rng.normal(0.0, 1.0, (rows, heads)).astype(np.float32)
    V, gY = (rng.normal(0.0, 1.0, (n, heads * d)).astype(np.float32) for n in (cols, rows))
    ip, ix = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    for r in np.nonzero(np.diff(ip) >= 2)[0]:
        b = ER[ix[ip[r]: ip[r + 1]]].astype(np.float64)
        lo, hi = b.min(axis=0), b.max(axis=0)
        EL[r] = (-(lo + hi) / 2.0 + rng.uniform(-0.25, 0.25, heads) * (hi - lo)).astype(np.float32)
    return EL, ER, V, gY


def both_signs_in_every_row(indptr, indices, EL, ER):
    """x > 0 and x < 0 both occur in every row of two entries or more, in every head"""
    ip, ix = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    x = EL[entry_rows(ip)] + ER[ix]
    two = np.diff(ip) >= 2
    pos = ac._seg_sum((x > 0).astype(np.float64), ip)[two]
    neg = ac._seg_sum((x < 0).astype(np.float64), ip)[two]
    return two.any() and (pos > 0).all() and (neg > 0).all()


words = hc.words
same_words = hc.same_words


def _heads_in(mem, a, extra):
    """a head array (n, heads) on the device in rows of heads + extra words, the pad words NaN"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = np.full((a.shape[0], a.shape[1] + extra), NAN_WORD, dtype=np.uint32)
    buf[:, : a.shape[1]] = a.view(np.uint32)
    return mem.alloc(buf), a.shape[1] + extra


def _heads_out(mem, ga, buf, n, heads, ld, what):
    w = mem.read(ga, buf).reshape(n, ld)
    assert (w[:, heads:] == SENTINEL).all(), f"{what}: the pad words of a head array were written"
    return np.ascontiguousarray(w[:, :heads]).view(np.float32)


def forward_host(ga, EL, ER, V, heads, slope, want_lse=True):
    """(y, lse or None)"""
    if want_lse:
        return ga.forward(EL, ER, V, heads, slope)
    return ga.forward(EL, ER, V, heads, slope, want_lse=False), None


def forward_device(mem, ga, EL, ER, V, heads, slope, pad=0, extra=0, want_lse=True, what=""):
    """hsgat_forward_device over fresh buffers: input pads NaN, y and lse pre-filled with a sentinel; the pad words of both must survive"""
    w = V.shape[1]
    (da, lda), (db, ldb) = _heads_in(mem, EL, extra), _heads_in(mem, ER, extra)
    dv, ldv = wc._features_in(mem, V, pad)
    ldy, ldl = w + pad, heads + extra
    dy = mem.alloc(np.full((ga.num_rows, ldy), SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full((ga.num_rows, ldl), SENTINEL, dtype=np.uint32)) if want_lse else None
    ga.forward_device(da.ptr, lda, db.ptr, ldb, dv.ptr, ldv, heads, w // heads, slope, dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = wc._features_out(mem, ga, dy, ga.num_rows, w, ldy, what)
    return y, (_heads_out(mem, ga, dl, ga.num_rows, heads, ldl, what) if want_lse else None)


def backward_host(ga, EL, ER, V, gY, lse, heads, slope):
    return ga.backward(EL, ER, V, gY, lse, heads, slope)


def backward_device(mem, ga, EL, ER, V, gY, lse, heads, slope, pad=0, extra=0, what=""):
    """hsgat_backward_device over fresh buffers: the pads of the inputs NaN, the three outputs pre-filled with a sentinel"""
    w = V.shape[1]
    (da, lda), (db, ldb), (dl, ldl) = _heads_in(mem, EL, extra), _heads_in(mem, ER, extra), _heads_in(mem, lse, extra)
    (dv, ldv), (dg, ldg) = (wc._features_in(mem, a, pad) for a in (V, gY))
    ld, ldh = w + pad, heads + extra
    oa = mem.alloc(np.full((ga.num_rows, ldh), SENTINEL, dtype=np.uint32))
    ob = mem.alloc(np.full((ga.num_cols, ldh), SENTINEL, dtype=np.uint32))
    ov = mem.alloc(np.full((ga.num_cols, ld), SENTINEL, dtype=np.uint32))
    ga.backward_device(da.ptr, lda, db.ptr, ldb, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, heads, w // heads, slope, oa.ptr, ldh, ob.ptr, ldh, ov.ptr, ld)
    return (_heads_out(mem, ga, oa, ga.num_rows, heads, ldh, f"{what}, gel"), _heads_out(mem, ga, ob, ga.num_cols, heads, ldh, f"{what}, ger"),
            wc._features_out(mem, ga, ov, ga.num_cols, w, ld, f"{what}, gv"))


def all_forward_forms(mem, ga, refs, EL, ER, V, heads, slope, pads, extras, what):
    """the host form and the device form at every pad and head-array ld, each with lse taken and with NULL, inside the bounds of one set of
    references; returns the lse of the host form"""
    y, lse = forward_host(ga, EL, ER, V, heads, slope)
    check_forward(refs, y, lse, f"{what}, host form, lse taken")
    check_forward(refs, forward_host(ga, EL, ER, V, heads, slope, False)[0], None, f"{what}, host form, lse NULL")
    for pad in pads:
        for extra in extras:
            for want in (True, False):
                tag = f"{what}, device form, pad {pad}, head ld {heads + extra}, {'lse taken' if want else 'lse NULL'}"
                check_forward(refs, *forward_device(mem, ga, EL, ER, V, heads, slope, pad, extra, want, tag), tag)
    return lse


def all_backward_forms(mem, ga, refs, EL, ER, V, gY, lse, heads, slope, pads, extras, what):
    worst = check_backward(refs, *backward_host(ga, EL, ER, V, gY, lse, heads, slope), f"{what}, host form")
    for pad in pads:
        for extra in extras:
            tag = f"{what}, device form, pad {pad}, head ld {heads + extra}"
            w = check_backward(refs, *backward_device(mem, ga, EL, ER, V, gY, lse, heads, slope, pad, extra, tag), tag)
            worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def general(mem, shapes=SHAPES):
    """300 x 517, 4000 entries, every (heads, d) of SHAPES, slope 0.2, 0 and 1, pad 0 and 8, head-array ld = heads and heads + 3, lse taken
    and NULL, both forms; forward, then backward with the lse the forward just wrote"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with gat.GraphAttention((indptr, indices, shape), heads) as ga:
            assert ga.nnz == NNZ
            EL, ER, V, gY = operands(shape, indptr, indices, heads, d, 9100 + 1000 * heads + d)
            assert both_signs_in_every_row(indptr, indices, EL, ER)
            for slope in SLOPES:
                what = f"general, {heads} heads of d {d}, slope {slope}"
                frefs = forward_refs(indptr, indices, EL, ER, V, slope)
                lse = all_forward_forms(mem, ga, frefs, EL, ER, V, heads, slope, (0, 8), (0, 3), what)
                w = all_backward_forms(mem, ga, backward_refs(frefs, gY, lse), EL, ER, V, gY, lse, heads, slope, (0, 8), (0, 3), what)
                print(f"{what}: backward worst error / bound = {w['gel']:.3f} (gel), {w['ger']:.3f} (ger), {w['gv']:.3f} (gv)")


def ties(mem, heads=3, d=8):
    """el and er on the 1/8 grid, so that x == 0 occurs (the slope branch of t and of dx): slope 0.25 and 0"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    shape = (ROWS, COLS)
    rng = np.random.default_rng(9300)
    EL, ER = ((rng.integers(-12, 13, (n, heads)) / 8.0).astype(np.float32) for n in shape)
    V, gY = (rng.normal(0.0, 1.0, (n, heads * d)).astype(np.float32) for n in (COLS, ROWS))
    x = EL[entry_rows(indptr)] + ER[indices.astype(np.int64)]
    assert (x == 0).mean() >= 0.01 and (x < 0).mean() >= 0.01, ((x == 0).mean(), (x < 0).mean())
    with gat.GraphAttention((indptr, indices, shape), heads) as ga:
        for slope in (0.25, 0.0):
            what = f"ties, slope {slope}"
            frefs = forward_refs(indptr, indices, EL, ER, V, slope)
            lse = all_forward_forms(mem, ga, frefs, EL, ER, V, heads, slope, (4,), (1,), what)
            all_backward_forms(mem, ga, backward_refs(frefs, gY, lse), EL, ER, V, gY, lse, heads, slope, (4,), (1,), what)


def heads_do_not_leak(mem, shapes=((4, 16), (5, 4))):
    """Forward: head 1's er word of some columns is NaN, of others +inf, of others -inf, head 1's el word of some rows likewise, and head 1's
    words of some V rows are NaN.  Heads 0, 2, ... stay inside their bounds of the CLEAN reference; head 1 follows the special-value table
    through its own reference (built from the planted el and er over the clean V: a -inf x weighs exactly 0), and every row that holds a
    column whose V row is NaN is NaN in all of head 1's words of Y while its lse word stays inside its bound.
    Backward, from clean operands: head 1's lse word of some rows is NaN, of others -inf.  Heads 0, 2, ... stay inside the bounds of
    their references; head 1 is NaN in gel of those rows and in ger and gV of the columns they touch."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    n = np.diff(indptr.astype(np.int64))
    of = pc.entry_rows(indptr)
    c_nan, c_inf, c_ninf, v_nan = np.array([3, 77, 200]), np.array([11, 150, 401]), np.array([8, 120, 300, 444]), np.array([5, 90, 333, 500])
    r_nan, r_inf, r_ninf = np.array([4, 100]), np.array([9, 210]), np.array([17, 250])
    b_nan, b_inf = (np.nonzero(n >= 3)[0][[2, 40]], np.nonzero(n >= 3)[0][[7, 90]])
    slope = 0.2
    for heads, d in shapes:
        h1 = slice(d, 2 * d)
        with gat.GraphAttention((indptr, indices, shape), heads) as ga:
            EL, ER, V, gY = operands(shape, indptr, indices, heads, d, 9500 + 1000 * heads + d)
            clean = forward_refs(indptr, indices, EL, ER, V, slope)
            ELp, ERp, Vp = EL.copy(), ER.copy(), V.copy()
            ERp[c_nan, 1], ERp[c_inf, 1], ERp[c_ninf, 1] = np.nan, np.inf, -np.inf
            ELp[r_nan, 1], ELp[r_inf, 1], ELp[r_ninf, 1] = np.nan, np.inf, -np.inf
            Vp[v_nan, h1] = np.nan
            planted = forward_refs(indptr, indices, ELp, ERp, V, slope)      # head 1: the planted el and er over the clean V
            assert planted[1].bad.sum() >= 3 and planted[1].finite.sum() > ROWS // 2 and (np.isneginf(planted[1].t) & planted[1].finite[of]).sum() >= 3
            refs = [planted[h] if h == 1 else clean[h] for h in range(heads)]
            touched = np.zeros(ROWS, dtype=bool)
            touched[of[np.isin(indices, v_nan)]] = True
            assert 3 <= touched.sum() < ROWS // 4
            what = f"heads do not leak, forward, {heads} heads of d {d}"
            for y, lse in (forward_host(ga, ELp, ERp, Vp, heads, slope), forward_device(mem, ga, ELp, ERp, Vp, heads, slope, 4, 1, True, what)):
                assert np.isnan(y[touched, h1]).all(), f"{what}: a row that holds a NaN row of V is not NaN in head 1"
                y = y.copy()
                y[touched, h1] = rounded_forward(refs)[0][touched, h1]      # checked above; the rest of head 1 against its reference
                check_forward(refs, y, lse, what)
                assert np.isfinite(np.delete(y, np.s_[d: 2 * d], axis=1)[n > 0]).all() and np.isfinite(np.delete(lse, 1, axis=1)[n > 0]).all()
            # backward
            lse = rounded_forward(clean)[1]
            lse[b_nan, 1], lse[b_inf, 1] = np.nan, -np.inf
            brefs = backward_refs(clean, gY, lse)
            assert brefs[1].bad_r.sum() == 4 and 4 <= brefs[1].bad_c.sum() < COLS // 4 and not any(r.bad_r.any() for h, r in enumerate(brefs) if h != 1)
            what = f"heads do not leak, backward, {heads} heads of d {d}"
            for g in (backward_host(ga, EL, ER, V, gY, lse, heads, slope), backward_device(mem, ga, EL, ER, V, gY, lse, heads, slope, 4, 1, what)):
                check_backward(brefs, *g, what)
                assert np.isfinite(np.delete(g[0], 1, axis=1)).all() and np.isfinite(np.delete(g[1], 1, axis=1)).all(), f"{what}: head 1's lse words reached another head"
                assert np.isfinite(np.delete(g[2], np.s_[d: 2 * d], axis=1)).all(), f"{what}: head 1's lse words reached another head"


def edges(mem, heads=3, d=8):
    """every pattern of pattern_cases.edge_patterns() at (3, 8): nnz = 0 ... 7, runs of empty rows, empty columns, one row that holds all
    301 entries, unsorted columns, a pair held twice; rows and columns without entries read +0.0 (and -inf in lse) bit for bit"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with gat.GraphAttention((indptr, indices, shape), heads) as ga:
            assert ga.nnz == indices.size
            EL, ER, V, gY = operands(shape, indptr, indices, heads, d, 9700)
            frefs = forward_refs(indptr, indices, EL, ER, V, 0.2)
            assert all(r.empty.sum() == (np.diff(indptr.astype(np.int64)) == 0).sum() for r in frefs)
            lse = all_forward_forms(mem, ga, frefs, EL, ER, V, heads, 0.2, (8,), (1,), name)
            assert (lse[frefs[0].empty] == -np.inf).all()
            all_backward_forms(mem, ga, backward_refs(frefs, gY, lse), EL, ER, V, gY, lse, heads, 0.2, (8,), (1,), name)


def plain_backward_device(mem, ga, Q, K, V, gY, lse, heads, scale):
    """hsmh_backward_device of the same object (heads_cases.backward_device through the base class): it overwrites the D words"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (wc._features_in(mem, a, 0) for a in (Q, K, V, gY))
    dl, ldl = hc._lse_in(mem, lse, 0)
    oq = mem.alloc(np.full((ga.num_rows, w), SENTINEL, dtype=np.uint32))
    ok, ov = (mem.alloc(np.full((ga.num_cols, w), SENTINEL, dtype=np.uint32)) for _ in range(2))
    mha.MultiHeadAttention.backward_device(ga, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, heads, w // heads, scale, oq.ptr, w, ok.ptr, w, ov.ptr, w)
    return tuple(wc._features_out(mem, ga, buf, n, w, w, name) for name, buf, n in (("gq", oq, ga.num_rows), ("gk", ok, ga.num_cols), ("gv", ov, ga.num_cols)))


def nothing_carried_over(mem):
    """on one object: hsgat at (4, 64), then hsmh_backward_device at (5, 4), which overwrites the D words, then hsgat at (4, 64) again gives
    the bits of the first time, which are the words of a fresh object; the dot-product call in between is inside its own bounds"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with gat.GraphAttention((indptr, indices, shape), 8) as ga, gat.GraphAttention((indptr, indices, shape), 4) as fresh:
        EL, ER, V, gY = operands(shape, indptr, indices, 4, 64, 9800)
        f1 = forward_device(mem, ga, EL, ER, V, 4, 0.2)
        b1 = backward_device(mem, ga, EL, ER, V, gY, f1[1], 4, 0.2)
        frefs = forward_refs(indptr, indices, EL, ER, V, 0.2)
        check_forward(frefs, *f1, "first call")
        check_backward(backward_refs(frefs, gY, f1[1]), *b1, "first call")
        Q2, K2, V2, gY2 = hc.operands(shape, 20, 9810)
        scores = hc.head_scores(indptr, indices, Q2, K2, 5)
        lse2 = hc.rounded_forward(hc.forward_refs(scores, V2, -0.75))[1]
        hc.check_backward(hc.backward_refs(scores, V2, gY2, lse2, -0.75), *plain_backward_device(mem, ga, Q2, K2, V2, gY2, lse2, 5, -0.75), "the dot-product call in between")
        assert same_words(f1, forward_device(mem, ga, EL, ER, V, 4, 0.2)) and same_words(f1, forward_host(ga, EL, ER, V, 4, 0.2))
        assert same_words(b1, backward_device(mem, ga, EL, ER, V, gY, f1[1], 4, 0.2)) and same_words(b1, backward_host(ga, EL, ER, V, gY, f1[1], 4, 0.2))
        assert same_words(f1, forward_device(mem, fresh, EL, ER, V, 4, 0.2)) and same_words(b1, backward_device(mem, fresh, EL, ER, V, gY, f1[1], 4, 0.2))


def large(mem, shape, indptr, indices, heads, d, seed, what, slope=0.2):
    """the device forms over one large pattern, forward then backward with the lse just written, every word of every head inside its bound
    (float64 sums in the references); returns the two lists of references"""
    EL, ER, V, gY = operands(shape, indptr, indices, heads, d, seed)
    fwd = forward_refs(indptr, indices, EL, ER, V, slope, exact=False)
    with gat.GraphAttention((indptr, indices, shape), heads) as ga:
        y, lse = forward_device(mem, ga, EL, ER, V, heads, slope, 4, 1, True, what)
        check_forward(fwd, y, lse, what)
        bwd = backward_refs(fwd, gY, lse)
        check_backward(bwd, *backward_device(mem, ga, EL, ER, V, gY, lse, heads, slope, 4, 1, what), what)
    return fwd, bwd


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
HEAD_ARRAYS = ("el", "er", "lse", "gel", "ger")
FEATURES = ("v", "gy", "gv")


def refusals(mem):
    l = gat.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    one = np.zeros(4, dtype=np.float32).ctypes.data
    # a null object
    assert l.hsgat_forward_device(None, vp(one), 1, vp(one), 1, vp(one), 4, 1, 4, 0.2, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsgat_forward(None, vp(one), vp(one), vp(one), 1, 4, 0.2, vp(one), None) == BAD_ARG
    assert l.hsgat_backward_device(None, vp(one), 1, vp(one), 1, vp(one), 4, vp(one), 4, vp(one), 1, 1, 4, 0.2, vp(one), 1, vp(one), 1, vp(one), 4) == BAD_ARG
    assert l.hsgat_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), 1, 4, 0.2, vp(one), vp(one), vp(one)) == BAD_ARG

    heads, d = 2, 4
    with gat.GraphAttention((indptr, indices, shape), 4) as ga, gat.GraphAttention((indptr, indices, shape), 4, backward=False) as fwd_only:
        EL, ER, V, gY = operands(shape, indptr, indices, heads, d, 9900)
        want_y, want_l = forward_host(ga, EL, ER, V, heads, 0.5)
        frefs = forward_refs(indptr, indices, EL, ER, V, 0.5)
        check_forward(frefs, want_y, want_l, "refusals")
        want_g = backward_host(ga, EL, ER, V, gY, want_l, heads, 0.5)
        check_backward(backward_refs(frefs, gY, want_l), *want_g, "refusals")

        def still_usable(rc, what, obj=ga):
            assert rc == BAD_ARG and l.hsmh_last_error(obj._h), (what, rc)
            assert same_words(forward_host(obj, EL, ER, V, heads, 0.5), (want_y, want_l)), f"unusable after {what}"
            if obj is ga:
                assert same_words(backward_host(ga, EL, ER, V, gY, want_l, heads, 0.5), want_g), f"unusable after {what}"

        def forward_call(a, obj=ga):
            return l.hsgat_forward_device(obj._h, vp(a["el"]), a["ldel"], vp(a["er"]), a["lder"], vp(a["v"]), a["ldv"], a["heads"], a["d"], a["slope"], vp(a["y"]), a["ldy"], vp(a["lse"]),
                                          a["ldlse"])

        def backward_call(a, obj=ga):
            return l.hsgat_backward_device(obj._h, vp(a["el"]), a["ldel"], vp(a["er"]), a["lder"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["ldlse"], a["heads"],
                                           a["d"], a["slope"], vp(a["gel"]), a["ldgel"], vp(a["ger"]), a["ldger"], vp(a["gv"]), a["ldgv"])

        # features: 9 rows x 16 words (ld up to 16), 16-byte aligned; head arrays: 9 rows of up to 4 words
        names = FEATURES + ("y",) + HEAD_ARRAYS
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 8 for name in FEATURES + ("y",)}, **{"ld" + name: 2 for name in HEAD_ARRAYS}, heads=heads, d=d, slope=0.2)
        assert forward_call(ok) == 0 and backward_call(ok) == 0
        el, er, v, gy, y, ls, gel, ger, gv = (ok[n] for n in ("el", "er", "v", "gy", "y", "lse", "gel", "ger", "gv"))
        nan, inf = float("nan"), float("inf")
        wide_ld = lambda names_, ld: {"ld" + n: ld for n in names_}      # noqa: E731
        # slope, SHAPES ACCEPTED (the object's max_heads is 4), lse: the rules both calls share
        shared = [("slope NaN", dict(slope=nan)), ("slope inf", dict(slope=inf)), ("slope -inf", dict(slope=-inf)), ("slope -0.5", dict(slope=-0.5)),
                  ("slope -2^-149", dict(slope=-1.4e-45)), ("d = 0", dict(d=0)), ("d = 1", dict(d=1)), ("d = 2", dict(d=2)), ("d = 3", dict(d=3)), ("d = 5", dict(heads=1, d=5)),
                  ("d = 12", dict(heads=1, d=12)), ("d = 24", dict(heads=1, d=24)), ("d = 512", dict(heads=1, d=512)), ("d = 2^31", dict(heads=1, d=2 ** 31)),
                  ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5, d=4)), ("heads * d = 512", dict(heads=4, d=128)),
                  ("heads * d = 512 at d = 256", dict(heads=2, d=256)), ("null el", dict(el=None)), ("null er", dict(er=None)), ("misaligned el", dict(el=el + 2)),
                  ("misaligned er", dict(er=er + 1)), ("misaligned lse", dict(lse=ls + 2)), ("ldel < heads", dict(ldel=1)), ("lder < heads", dict(lder=1)), ("lder = 0", dict(lder=0)),
                  ("ldl < heads", dict(ldlse=1)), ("ldl = 0", dict(ldlse=0)), ("null v", dict(v=None)), ("misaligned v", dict(v=v + 4)), ("misaligned v by 8", dict(v=v + 8)),
                  ("ldv % 4", dict(ldv=10)), ("ldv < heads * d", dict(ldv=4))]
        for what, change in shared:
            if "heads * d" in what or "d = 512" in what or "2^31" in what:
                change = dict(wide_ld(FEATURES + ("y",), 512), **change)
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        fcases = [("null y", dict(y=None)), ("misaligned y", dict(y=y + 4)), ("ldy % 4", dict(ldy=10)), ("ldy < heads * d", dict(ldy=4)), ("y is v", dict(y=v)),
                  ("y is el", dict(y=el)), ("y over the last er word", dict(y=er + 32 + 4 * 4, er=er + 4 * 4)), ("lse inside y", dict(lse=y + 4 * 4)), ("lse is el", dict(lse=el)),
                  ("lse over the last er word", dict(lse=er + 8 * 2 * 4 + 4)), ("lse inside v", dict(lse=v + 8)), ("y's last row in v", dict(v=gy + 16, y=gy + 16 + 8 * 8 * 4))]
        for what, change in fcases:
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("null lse", dict(lse=None)), ("null gy", dict(gy=None)), ("misaligned gy", dict(gy=gy + 4)), ("ldgy % 4", dict(ldgy=10)), ("ldgy < heads * d", dict(ldgy=4)),
                  ("null gel", dict(gel=None)), ("null ger", dict(ger=None)), ("null gv", dict(gv=None)), ("misaligned gel", dict(gel=gel + 2)), ("misaligned ger", dict(ger=ger + 3)),
                  ("misaligned gv", dict(gv=gv + 4)), ("ldgel < heads", dict(ldgel=1)), ("ldger < heads", dict(ldger=1)), ("ldgv % 4", dict(ldgv=10)), ("ldgv < heads * d", dict(ldgv=4)),
                  ("gel is el", dict(gel=el)), ("ger is er", dict(ger=er)), ("gv is v", dict(gv=v)), ("gv is gy", dict(gv=gy)), ("gel is lse", dict(gel=ls)), ("ger is gel", dict(ger=gel)),
                  ("gv is ger", dict(gv=ger)), ("gel inside gy", dict(gel=gy + 8)), ("ger over the last lse word", dict(ger=ls + 5 * 2 * 4 + 4)),
                  ("gel's last word in el", dict(el=el + 64, gel=el + 64 - 5 * 2 * 4 - 4)), ("gv's first word in ger's last", dict(gv=gv + 80, ger=gv + 80 - 8 * 2 * 4 - 4))]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        # the host forms
        host = {name: np.zeros(9 * 8, np.float32) for name in names}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, heads=heads, d=d, slope=0.2)

        def forward_host_call(a, obj=ga):
            return l.hsgat_forward(obj._h, vp(a["el"]), vp(a["er"]), vp(a["v"]), a["heads"], a["d"], a["slope"], vp(a["y"]), vp(a["lse"]))

        def backward_host_call(a, obj=ga):
            return l.hsgat_backward(obj._h, vp(a["el"]), vp(a["er"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), a["heads"], a["d"], a["slope"], vp(a["gel"]), vp(a["ger"]), vp(a["gv"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0
        both = [("d = 0", dict(d=0)), ("d = 6", dict(d=6)), ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5)), ("heads * d = 512", dict(heads=4, d=128)),
                ("slope NaN", dict(slope=nan)), ("slope inf", dict(slope=inf)), ("slope -1", dict(slope=-1.0))]
        for what, change in both + [(f"null {n}", {n: None}) for n in ("el", "er", "v", "y")] + [("y is v", dict(y=okh["v"])), ("lse inside y", dict(lse=okh["y"] + 8)),
                                                                                                  ("lse is el", dict(lse=okh["el"]))]:
            still_usable(forward_host_call(dict(okh, **change)), "forward: " + what)
        for what, change in both + [(f"null {n}", {n: None}) for n in FEATURES + HEAD_ARRAYS] + [("gel is el", dict(gel=okh["el"])), ("ger is gel", dict(ger=okh["gel"])),
                                                                                                 ("gv inside lse", dict(gv=okh["lse"] + 8)), ("gel inside gy", dict(gel=okh["gy"] + 8))]:
            still_usable(backward_host_call(dict(okh, **change)), "backward: " + what)
        # backward on an object created without HSMH_BACKWARD: refused in both forms with the flag named, and the forward of that object still runs
        still_usable(backward_call(ok, fwd_only), "backward_device without HSMH_BACKWARD", fwd_only)
        assert b"HSMH_BACKWARD" in l.hsmh_last_error(fwd_only._h)
        still_usable(backward_host_call(okh, fwd_only), "backward without HSMH_BACKWARD", fwd_only)
        assert b"HSMH_BACKWARD" in l.hsmh_last_error(fwd_only._h)
        assert forward_call(ok, fwd_only) == 0
        # the messages name the rule
        assert forward_call(dict(ok, slope=-1.0)) == BAD_ARG and b"slope" in l.hsmh_last_error(ga._h)
        assert forward_call(dict(ok, d=5)) == BAD_ARG and b"4, 8, 16, 32, 64, 128, 256" in l.hsmh_last_error(ga._h)
        # fine: slope -0.0 and 0; ranges that touch without sharing a byte (lse right behind y's 6 rows, er right behind el's 6 rows of 2 words, gv right behind
        # ger's 9 rows, gel right behind lse's 6 rows); a NULL lse
        assert forward_call(dict(ok, slope=-0.0)) == 0 and backward_call(dict(ok, slope=-0.0)) == 0 and forward_call(dict(ok, slope=0.0)) == 0
        assert forward_call(dict(ok, lse=y + (5 * 8 + 8) * 4)) == 0
        assert forward_call(dict(ok, er=el + (5 * 2 + 2) * 4)) == 0
        assert forward_call(dict(ok, lse=None, ldlse=0)) == 0
        assert backward_call(dict(ok, gv=gv + 80, ger=gv + 80 - (8 * 2 + 2) * 4)) == 0
        assert backward_call(dict(ok, gel=ls + (5 * 2 + 2) * 4)) == 0
        for obj in (ga, fwd_only):
            obj.set_stream(None)
            obj.sync()
