"""The cases of the fused attention backward step (include/hisparse_attention_backward.h), shared by tests/test_attention_backward_cpu.py
(libhisparse_cpu.so, in a child process) and tests/test_gpu_attention_backward.py (the HIP library, on the device), written against the
memory interface of tests/pattern_cases.py.

Reference, from the header's ARITHMETIC block.  The fp32 products Q[row(e)][j] K[col(e)][j] and gY[row(e)][j] V[col(e)][j] are formed in
numpy float32 and widened to float64.  Per entry S_e and GP_e = math.fsum of the products, A_e and A'_e = the sums of their magnitudes,
and with u = 2^-24 (delta_e, eta_e as in tests/attention_cases.py, whose Scores class supplies S, A and delta)
    T_e = scale S_e,   P_e = exp(T_e - lse[row(e)]) with the lse WORDS AS GIVEN,   D_r = sum_{e in r} P_e GP_e,   GS_e = scale P_e (GP_e - D_r)
    gam_e  = u |GP_e| + d 2^-52 A'_e + 2^-149
    rho_e  = expm1(eta_e + 32 2^-52)
    epsD_r = sum_{e in r} P_e (rho_e |GP_e| + (1 + rho_e) gam_e) + (n_r + 16) 2^-52 sum_{e in r} P_e |GP_e|
    eps_e  = |scale| (rho_e P_e |GP_e - D_r| + (1 + rho_e) P_e (gam_e + epsD_r))
    mag_e  = |scale| P_e (|GP_e| + |D_r|)
    |gq[r][j] - gQ| <= u |gQ| + sum_{e in r} eps_e |K_ej| + (n_r + 16) 2^-52 sum_{e in r} mag_e |K_ej| + 2^-149
    |gk[c][j] - gK| <= u |gK| + sum_{col = c} eps_e |Q_ej| + (m_c + 16) 2^-52 sum_{col = c} mag_e |Q_ej| + 2^-149
    |gv[c][j] - gV| <= u |gV| + sum_{col = c} rho_e P_e |gY_ej| + (m_c + 16) 2^-52 sum_{col = c} P_e |gY_ej| + 2^-149
D, gQ, gK and gV are math.fsum too (exact=True); in the large cases of the GPU tests every sum is a float64 sum and the 2^-52 terms are
doubled, as attention_cases.Reference(exact=False) does.  Every word of the three outputs is held to its bound.  A row without entries
reads +0.0 in gQ and a column without entries +0.0 in gK and gV, bit for bit; a row with entries whose lse word is not finite reads NaN
in all of gQ[r] and in all of gK[c] and gV[c] of every column it touches, and the other words are computed without it.
INPUT CONDITION: every entry of a row with a finite lse has rho_e <= 2^-12 (asserted here), so that the bounds cannot go slack unnoticed.
Every score of every case is finite."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import attention_backward

import attention_cases as ac
import float_contract as fc
import pattern_cases as pc
import wide_cases as wc
from pattern_cases import HipMemory, HostMemory, edge_patterns, entry_rows, random_pattern  # noqa: F401

BAD_ARG, BAD_MATRIX = -1, -4
SENTINEL = wc.SENTINEL
DS = ac.DS
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
RHO_MAX = ac.RHO_MAX
TINY = 2.0 ** -149
OUTPUTS = ("gq", "gk", "gv")


# ---- reference -----------------------------------------------------------------------------------------------------------------------
class Reference:
    def __init__(self, scores, V, gY, lse, scale):
        """scores: scores_of(indptr, indices, Q, K); lse: float32 words, one per row, as the call is given them"""
        s, sc = scores, float(np.float32(scale))
        self.scores, self.sc, self.d = s, sc, V.shape[1]
        ip, ix, of = s.indptr, s.indices, s.of
        assert s.fin.all() and gY.dtype == np.float32 and V.dtype == np.float32 and gY.shape[1] == V.shape[1] == s.d
        lse = np.asarray(lse, dtype=np.float32)
        assert lse.shape == (ip.size - 1,)
        self.kk = kk = 1.0 if s.exact else 2.0
        self.seg = ac._seg_fsum if s.exact else ac._seg_sum
        self.n = np.diff(ip)
        self.perm = np.argsort(ix, kind="stable")                       # the entries in column order, a column's in ascending CSR index
        self.m = np.bincount(ix, minlength=V.shape[0]).astype(np.int64)
        self.cptr = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.empty_r, self.empty_c = self.n == 0, self.m == 0
        self.bad_r = ~self.empty_r & ~np.isfinite(lse)
        self.bad_c = np.zeros(V.shape[0], dtype=bool)
        self.bad_c[ix[self.bad_r[of]]] = True
        live = ~self.bad_r[of]                                            # entries that count; the others are NaN wherever they reach
        g64 = (gY[of] * V[ix]).astype(np.float64)                       # one fp32 multiply per product
        self.GP = np.array([math.fsum(row) for row in g64.tolist()], dtype=np.float64) if s.exact else g64.sum(axis=1)
        gam = fc.U * np.abs(self.GP) + kk * self.d * 2.0 ** -52 * np.abs(g64).sum(axis=1) + TINY
        T = sc * s.S
        assert np.isfinite(T).all()
        eta = (1.0 + fc.U) * abs(sc) * s.delta + fc.U * np.abs(T) + TINY
        self.rho = rho = np.expm1(eta + 32.0 * 2.0 ** -52)
        assert (rho[live] <= RHO_MAX).all(), f"input condition: rho_e reaches {rho[live].max():.3g}"
        with np.errstate(all="ignore"):
            self.P = P = np.where(live, np.exp(T - np.where(live, lse.astype(np.float64)[of], 0.0)), 0.0)
        assert np.isfinite(P).all()
        self.K64, self.Q64, self.G64 = K64, Q64, G64 = s.K64[ix], s.Q64[of], gY.astype(np.float64)[of]      # per entry (scores_of keeps Q and K in float64)
        self.D = self.seg((P * self.GP)[:, None], ip)[:, 0]
        Dof = self.D[of]
        eps_d = ac._seg_sum((P * (rho * np.abs(self.GP) + (1.0 + rho) * gam))[:, None], ip)[:, 0] + kk * (self.n + 16) * 2.0 ** -52 * ac._seg_sum((P * np.abs(self.GP))[:, None], ip)[:, 0]
        self.GS = sc * P * (self.GP - Dof)
        eps = abs(sc) * (rho * P * np.abs(self.GP - Dof) + (1.0 + rho) * P * (gam + eps_d[of]))
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

    def gradients(self, GS, P):
        """(gQ, gK, gV) in float64 from per-entry gs and p, by this reference's sums"""
        ip, pm = self.scores.indptr, self.perm
        return self.seg(GS[:, None] * self.K64, ip), self.seg((GS[:, None] * self.Q64)[pm], self.cptr), self.seg((P[:, None] * self.G64)[pm], self.cptr)

    def check(self, gq, gk, gv, what, extra=None):
        """every word of the three outputs; returns the largest error / bound per output; `extra` (a dict of arrays) widens the bounds"""
        worst = {}
        for name, got in zip(OUTPUTS, (gq, gk, gv)):
            got = np.asarray(got, dtype=np.float32)
            want, bound, empty, bad = self.want[name], self.bound[name], self.empty[name], self.bad[name]
            if extra is not None:
                bound = bound + extra[name]
            assert got.shape == want.shape, (what, name, got.shape, want.shape)
            assert not got.view(np.uint32)[empty].any(), f"{what}: {name} of a {'row' if name == 'gq' else 'column'} without entries is not +0.0"
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
        print(f"{what}: error / bound = {worst['gq']:.3f} (gq), {worst['gk']:.3f} (gk), {worst['gv']:.3f} (gv)")
        return worst

    def rounded(self, grads=None):
        """a correct result: the reference's own words rounded once (what the planted defects are applied to)"""
        out = []
        for name, x in zip(OUTPUTS, grads or (self.GQ, self.GK, self.GV)):
            out.append(np.where(self.bad[name][:, None], np.nan, x).astype(np.float32))
        return tuple(out)


def scores_of(indptr, indices, Q, K, exact=True):
    s = ac.Scores(indptr, indices, Q, K, exact)
    s.Q64, s.K64 = Q.astype(np.float64), K.astype(np.float64)
    return s


def forward_lse(scores, V, scale):
    """lse as the forward writes it: the reference forward's, rounded to fp32 (-inf for a row without entries)"""
    return ac.Reference(scores, V, scale).rounded()[1]


def reference(indptr, indices, Q, K, V, gY, lse, scale, exact=True):
    return Reference(scores_of(indptr, indices, Q, K, exact), V, gY, lse, scale)


# ---- inputs and the two forms --------------------------------------------------------------------------------------------------------
def operands(shape, d, seed):
    """Q, K, V, gY"""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(0.0, 1.0, (n, d)).astype(np.float32) for n in (rows, cols, cols, rows))


def host_form(pb, Q, K, V, gY, lse, scale):
    return pb.backward(Q, K, V, gY, lse, scale)


def device_form(mem, pb, Q, K, V, gY, lse, scale, pad=0, what=""):
    """hsab_backward_device over fresh buffers: input pads NaN, the three outputs pre-filled with a sentinel; their pad words must survive"""
    d = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (wc._features_in(mem, a, pad) for a in (Q, K, V, gY))
    dl = mem.alloc(np.ascontiguousarray(lse, dtype=np.float32).view(np.uint32))
    ld = wc.round_up4(d) + pad
    oq = mem.alloc(np.full((pb.num_rows, ld), SENTINEL, dtype=np.uint32))
    ok, ov = (mem.alloc(np.full((pb.num_cols, ld), SENTINEL, dtype=np.uint32)) for _ in range(2))
    pb.backward_device(dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, d, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld)
    return tuple(wc._features_out(mem, pb, buf, n, d, ld, f"{what}, {name}") for name, buf, n in (("gq", oq, pb.num_rows), ("gk", ok, pb.num_cols), ("gv", ov, pb.num_cols)))


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_words(a, b):
    return all(np.array_equal(words(x), words(y)) for x, y in zip(a, b))


def all_forms(mem, pb, ref, Q, K, V, gY, lse, scale, pads, what):
    """the host form and the device form at every pad inside the bounds of one reference; the largest error / bound per output"""
    worst = ref.check(*host_form(pb, Q, K, V, gY, lse, scale), f"{what}, host form")
    for pad in pads:
        w = ref.check(*device_form(mem, pb, Q, K, V, gY, lse, scale, pad, what), f"{what}, device form, pad {pad}")
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def general(mem, ds=DS):
    """300 x 517, 4000 entries, every d of DS, scale 0.125, 1 and -2, pad 0 and 8, both forms; lse from the reference forward, rounded"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        assert pb.nnz == NNZ and pb.info()["nnz"] == NNZ
        for d in ds:
            Q, K, V, gY = operands(shape, d, 3100 + d)
            scores = scores_of(indptr, indices, Q, K)
            for scale in (0.125, 1.0, -2.0):
                lse = forward_lse(scores, V, scale)
                w = all_forms(mem, pb, Reference(scores, V, gY, lse, scale), Q, K, V, gY, lse, scale, (0, 8), f"general, d {d}, scale {scale}")
                worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"general: worst error / bound = {worst['gq']:.3f} (gq), {worst['gk']:.3f} (gk), {worst['gv']:.3f} (gv)")


def edges(mem):
    """every pattern of pattern_cases.edge_patterns() at d = 1 and 5, and 1 x 1 with its one entry: nnz = 0 ... 7, runs of empty rows, empty
    columns, one row that holds all 301 entries, unsorted columns, a pair held twice; rows and columns without entries read +0.0 bit for
    bit (Reference.check)"""
    one = [("1 x 1", 1, 1, np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32))]
    for name, rows, cols, indptr, indices in edge_patterns() + one:
        shape = (rows, cols)
        with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
            assert pb.nnz == indices.size
            for d in (1, 5):
                Q, K, V, gY = operands(shape, d, 3300 + d)
                scores = scores_of(indptr, indices, Q, K)
                lse = forward_lse(scores, V, 1.5)
                ref = Reference(scores, V, gY, lse, 1.5)
                assert ref.empty_r.sum() == (np.diff(indptr.astype(np.int64)) == 0).sum() and ref.empty_c.sum() == cols - np.unique(indices).size
                assert not ref.bad_r.any()
                all_forms(mem, pb, ref, Q, K, V, gY, lse, 1.5, (8,), f"{name}, d {d}")


def special_rows(mem, ds=(5, 64)):
    """an lse word of NaN planted on one row with entries and of -inf on another (a bad and a dead row of the forward): NaN in all of gQ of
    the two rows and in all of gK and gV of every column they touch, every other word inside its bound, computed without them"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    n = np.diff(indptr.astype(np.int64))
    r_nan, r_inf = (int(r) for r in np.nonzero(n >= 3)[0][[2, 40]])
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        for d in ds:
            Q, K, V, gY = operands(shape, d, 3500 + d)
            scores = scores_of(indptr, indices, Q, K)
            lse = forward_lse(scores, V, 0.5)
            lse[r_nan], lse[r_inf] = np.nan, -np.inf
            ref = Reference(scores, V, gY, lse, 0.5)
            touched = np.unique(np.concatenate([indices[indptr[r]: indptr[r + 1]] for r in (r_nan, r_inf)]))
            assert ref.bad_r.sum() == 2 and np.array_equal(np.nonzero(ref.bad_c)[0], touched) and 2 <= touched.size < COLS // 4
            what = f"special rows, d {d}"
            for gq, gk, gv in (host_form(pb, Q, K, V, gY, lse, 0.5), device_form(mem, pb, Q, K, V, gY, lse, 0.5, 4, what)):
                ref.check(gq, gk, gv, what)
                assert np.isnan(gq[[r_nan, r_inf]]).all() and np.isnan(gk[touched]).all() and np.isnan(gv[touched]).all()
                assert np.isfinite(np.delete(gq, [r_nan, r_inf], axis=0)).all() and np.isfinite(np.delete(gk, touched, axis=0)).all()
                assert np.isfinite(np.delete(gv, touched, axis=0)).all()


def scale_zero(mem):
    """scale = 0: gQ = gK = 0 in every word, and gV[c] = sum_{col(e) = c} gY[row(e)] / n_row(e), the column's share of the rows' means"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 7)
    shape = (ROWS, COLS)
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        for d in (5, 64):
            Q, K, V, gY = operands(shape, d, 3600 + d)
            scores = scores_of(indptr, indices, Q, K)
            lse = forward_lse(scores, V, 0.0)
            ref = Reference(scores, V, gY, lse, 0.0)
            assert not ref.GQ.any() and not ref.GK.any()
            of, ix = entry_rows(indptr), indices.astype(np.int64)
            mean = np.zeros((COLS, d))
            np.add.at(mean, ix, gY.astype(np.float64)[of] / ref.n[of][:, None])
            assert np.allclose(ref.GV, mean, rtol=1e-5, atol=1e-6)         # lse = log n rounded to fp32: P = 1 / n within a few u
            what = f"scale 0, d {d}"
            for gq, gk, gv in (host_form(pb, Q, K, V, gY, lse, 0.0), device_form(mem, pb, Q, K, V, gY, lse, 0.0, 4, what)):
                ref.check(gq, gk, gv, what)
                assert not (gq != 0).any() and not (gk != 0).any()


def heads(mem):
    """H = 3 heads of d = 8 stored [index][head][feature]: three calls with ld = 24 and pointers offset by h d words over interleaved
    buffers; each head against its own reference, the other heads' words in the pad (those of the inputs are read by no result, those
    of the outputs survive the call)"""
    H, d = 3, 8
    ld = H * d
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 8)
    shape = (ROWS, COLS)
    Q, K, V, gY = operands(shape, ld, 3700)
    cuts = [slice(h * d, (h + 1) * d) for h in range(H)]
    per_head = [tuple(np.ascontiguousarray(a[:, c]) for a in (Q, K, V, gY)) for c in cuts]
    refs, lses = [], []
    for q, k, v, g in per_head:
        scores = scores_of(indptr, indices, q, k)
        lses.append(forward_lse(scores, v, 0.5))
        refs.append(Reference(scores, v, g, lses[-1], 0.5))
    dq, dk, dv, dg = (mem.alloc(words(a)) for a in (Q, K, V, gY))
    dl = [mem.alloc(words(l)) for l in lses]
    outs = [mem.alloc(np.full((n, ld), SENTINEL, dtype=np.uint32)) for n in (ROWS, COLS, COLS)]
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        before = None
        for h in range(H):
            off = 4 * h * d
            pb.backward_device(dq.ptr + off, ld, dk.ptr + off, ld, dv.ptr + off, ld, dg.ptr + off, ld, dl[h].ptr, d, 0.5, outs[0].ptr + off, ld, outs[1].ptr + off, ld,
                               outs[2].ptr + off, ld)
            got = [mem.read(pb, o).reshape(-1, ld) for o in outs]
            for i, g in enumerate(got):
                assert (g[:, (h + 1) * d:] == SENTINEL).all() and (g[:, cuts[h]] != SENTINEL).any(), f"head {h} wrote another head's words of {OUTPUTS[i]}"
                if h:
                    assert np.array_equal(g[:, : h * d], before[i][:, : h * d]), f"head {h} changed an earlier head's words of {OUTPUTS[i]}"
            before = got
        for h in range(H):
            refs[h].check(*(np.ascontiguousarray(g[:, cuts[h]]).view(np.float32) for g in got), f"head {h} of {H}")


def nothing_carried_over(mem):
    """two different d and scale on one object, then the first again: the same bits as the first time, and the second call the words of a
    fresh object (the D words of one call reach no other)"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb, attention_backward.PatternAttentionBackward((indptr, indices, shape)) as fresh:
        Q, K, V, gY = operands(shape, 64, 3800)
        lse = forward_lse(scores_of(indptr, indices, Q, K), V, 1.0)
        first = device_form(mem, pb, Q, K, V, gY, lse, 1.0)
        Q2, K2, V2, gY2 = operands(shape, 5, 3810)
        lse2 = forward_lse(scores_of(indptr, indices, Q2, K2), V2, -0.75)
        second = device_form(mem, pb, Q2, K2, V2, gY2, lse2, -0.75, 4)
        assert same_words(second, device_form(mem, fresh, Q2, K2, V2, gY2, lse2, -0.75, 4))
        reference(indptr, indices, Q2, K2, V2, gY2, lse2, -0.75).check(*second, "second call")
        assert same_words(first, device_form(mem, pb, Q, K, V, gY, lse, 1.0))
        assert same_words(first, host_form(pb, Q, K, V, gY, lse, 1.0))


def _create(rows, cols, indptr, indices):
    l = attention_backward.lib()
    h = C.c_void_p(0xBAD)
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint32)
    indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    rc = l.hsab_create(C.byref(h), 0, rows, cols, None if indptr is None else indptr.ctypes.data, None if indices is None else indices.ctypes.data)
    return rc, h


FEATURES = ("q", "k", "v", "gy", "gq", "gk", "gv")


def refusals(mem):
    l = attention_backward.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    bad_index = indices.copy()
    bad_index[3] = 9
    down = np.array([0, 3, 2, 4, 5, 6, 7], dtype=np.uint32)
    shifted = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
    for what, args, code in (("null indptr", (6, 9, None, indices), BAD_ARG), ("null indices", (6, 9, indptr, None), BAD_ARG), ("no rows", (0, 9, indptr, indices), BAD_ARG),
                             ("no columns", (6, 0, indptr, indices), BAD_ARG), ("index = num_cols", (6, 9, indptr, bad_index), BAD_MATRIX),
                             ("indptr decreases", (6, 9, down, indices), BAD_MATRIX), ("indptr[0] = 1", (6, 9, shifted, indices), BAD_MATRIX)):
        rc, h = _create(*args)
        assert rc == code and not h.value and l.hsab_last_error(None), (what, rc, h.value)
    assert l.hsab_create(None, 0, 6, 9, indptr.ctypes.data, indices.ctypes.data) == BAD_ARG and l.hsab_last_error(None)
    # null-object calls
    one = np.zeros(4, dtype=np.float32).ctypes.data
    assert l.hsab_info(None, None, None) == BAD_ARG and l.hsab_sync(None) == BAD_ARG and l.hsab_set_stream(None, None) == BAD_ARG
    assert l.hsab_backward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 4, vp(one), 1, 1.0, vp(one), 4, vp(one), 4, vp(one), 4) == BAD_ARG
    assert l.hsab_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), 1, 1.0, vp(one), vp(one), vp(one)) == BAD_ARG
    assert l.hsab_destroy(None) == 0

    d = 5
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        Q, K, V, gY = operands(shape, d, 3900)
        lse = forward_lse(scores_of(indptr, indices, Q, K), V, 0.5)
        want = host_form(pb, Q, K, V, gY, lse, 0.5)
        reference(indptr, indices, Q, K, V, gY, lse, 0.5).check(*want, "refusals")

        def still_usable(rc, what):
            assert rc == BAD_ARG and l.hsab_last_error(pb._h), (what, rc)
            assert same_words(host_form(pb, Q, K, V, gY, lse, 0.5), want), f"unusable after {what}"

        def device_call(a):
            return l.hsab_backward_device(pb._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], vp(a["gy"]), a["ldgy"], vp(a["lse"]), a["d"], a["scale"],
                                          vp(a["gq"]), a["ldgq"], vp(a["gk"]), a["ldgk"], vp(a["gv"]), a["ldgv"])

        # buffers of 9 rows x 16 words (the larger dimension, ld up to 16), 16-byte aligned
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in FEATURES + ("lse",)}
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 8 for name in FEATURES}, d=d, scale=1.0)
        q, k, v, gy, ls, gq, gk = (ok[n] for n in ("q", "k", "v", "gy", "lse", "gq", "gk"))
        nan, inf = float("nan"), float("inf")
        cases = [("d = 0", dict(d=0)), ("d = 257", dict({"ld" + n: 260 for n in FEATURES}, d=257)), ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf)),
                 ("scale -inf", dict(scale=-inf)), ("null lse", dict(lse=None)), ("misaligned lse", dict(lse=ls + 2)), ("gq is q", dict(gq=q)), ("gk inside k", dict(gk=k + 16 * 4)),
                 ("gv is v", dict(gv=v)), ("gq is gy", dict(gq=gy)), ("gk is q", dict(gk=q)), ("gv is gk", dict(gv=gk)), ("gk is gq", dict(gk=gq)),
                 ("gv's first row in gq's last", dict(gv=gq + 5 * 8 * 4)), ("gq is lse", dict(gq=ls)), ("gv over the last lse word", dict(gv=ls + 16)),
                 ("gq's last row in v", dict(v=q + 16, gq=q + 16 + 8 * 8 * 4))]
        for name in FEATURES:
            ptr, ld = ok[name], "ld" + name
            cases += [(f"null {name}", {name: None}), (f"misaligned {name}", {name: ptr + 4}), (f"misaligned {name} by 8", {name: ptr + 8}), (f"{ld} % 4", {ld: 10}),
                      (f"{ld} < d", {ld: 4})]
        for what, change in cases:
            still_usable(device_call(dict(ok, **change)), "device form: " + what)
        # the host form
        host = {name: np.zeros(9 * 8, np.float32) for name in FEATURES + ("lse",)}
        okh = dict({name: a.ctypes.data for name, a in host.items()}, d=d, scale=1.0)
        changes = [("d = 0", dict(d=0)), ("d = 257", dict(d=257)), ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf)), ("gk is k", dict(gk=okh["k"])),
                   ("gq is gk", dict(gq=okh["gk"])), ("gv inside lse", dict(gv=okh["lse"] + 8)), ("gq inside gy", dict(gq=okh["gy"] + 8))]
        changes += [(f"null {name}", {name: None}) for name in FEATURES + ("lse",)]
        for what, change in changes:
            a = dict(okh, **change)
            still_usable(l.hsab_backward(pb._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["gy"]), vp(a["lse"]), a["d"], a["scale"], vp(a["gq"]), vp(a["gk"]), vp(a["gv"])),
                         "host form: " + what)
        # ranges that touch without sharing a byte are fine: gv right behind the 9 rows of gk, gq right behind the 6 words of lse
        assert device_call(dict(ok, gv=gk + (8 * 8 + 8) * 4)) == 0
        assert device_call(dict(ok, gq=ls + 32)) == 0
        pb.set_stream(None)
        pb.sync()
