"""The cases of the fused attention step (include/hisparse_attention.h), shared by tests/test_attention_cpu.py (libhisparse_cpu.so, in a
child process) and tests/test_gpu_attention.py (the HIP library, on the device), written against the memory interface of
tests/pattern_cases.py.

Reference, from the header's ARITHMETIC block.  The fp32 products p[e][j] = Q[row(e)][j] K[col(e)][j] are formed in numpy float32 and
widened to float64.  Per entry S_e = math.fsum of its products, A_e = the sum of their magnitudes, and with u = 2^-24
    delta_e = u |S_e| + d 2^-52 A_e + 2^-149,    T_e = scale S_e,    eta_e = (1 + u) |scale| delta_e + u |T_e| + 2^-149.
Per row, in float64 from the T_e: M = max T, E = exp(T - M), L = sum E, P = E / L, Y_j = sum_e P_e V_ej, LSE = M + log L,
D_j = sum_e P_e |V_ej - Y_j|, B_j = sum_e P_e |V_ej|, eta_r = max_e eta_e, rho_r = expm1(eta_r), n = the row's length, and
    |y[r][j] - Y_j| <= u |Y_j| + rho_r / (1 - rho_r) D_j + (n + 16) 2^-52 B_j + 2^-149
    |lse[r] - LSE|  <= u |LSE| + eta_r + (n + 16) 2^-52 (1 + |LSE|) + 2^-149.
L and Y are math.fsum too (exact=True); in the two large cases of the GPU tests every sum is a float64 sum and the 2^-52 terms are
doubled, as wide_cases.Reference(exact=False) does.  Every output word and every lse word is held to its bound.  A score with a
non-finite product is the IEEE double sum of its products times scale in fp32 (-inf, +inf or NaN), and its row follows the header's
table: no entries -> +0.0 and -inf bit for bit; only -inf -> NaN and -inf; a NaN or a +inf -> NaN and NaN; a -inf score under a finite
maximum weighs exactly 0.
INPUT CONDITION: every finite row of every case has expm1(eta_r) <= 2^-12 (asserted here), so that the bound cannot go slack unnoticed."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import attention

import float_contract as fc
import pattern_cases as pc
import wide_cases as wc
from pattern_cases import HipMemory, HostMemory, edge_patterns, entry_rows, random_pattern  # noqa: F401

BAD_ARG, BAD_MATRIX = -1, -4
SENTINEL = wc.SENTINEL
NEG_INF_WORD = 0xFF800000
DS = wc.DS
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
RHO_MAX = 2.0 ** -12


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def _seg_sum(x, indptr):
    """float64 sums of the rows' segments of x (entries x width); zeros for rows without entries"""
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.zeros((indptr.size - 1,) + x.shape[1:], dtype=np.float64)
    live = np.diff(indptr) > 0
    if x.shape[0] and live.any():
        out[live] = np.add.reduceat(x, indptr[:-1][live], axis=0)
    return out


def _seg_fsum(x, indptr):
    """the same sums, correctly rounded"""
    ip = np.asarray(indptr, dtype=np.int64).tolist()
    x = x.reshape(x.shape[0], int(np.prod(x.shape[1:])))
    cols = x.T.tolist()
    return np.array([[math.fsum(col[ip[i]: ip[i + 1]]) for col in cols] for i in range(len(ip) - 1)], dtype=np.float64).reshape(len(ip) - 1, x.shape[1])


def _seg_max(x, indptr, empty):
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.full(indptr.size - 1, empty, dtype=np.float64)
    live = np.diff(indptr) > 0
    if x.size and live.any():
        out[live] = np.maximum.reduceat(x, indptr[:-1][live])
    return out


class Scores:
    """what depends on the pattern, Q and K alone (shared by the references of every scale and V): S_e, A_e and the non-finite scores"""

    def __init__(self, indptr, indices, Q, K, exact=True):
        assert Q.dtype == np.float32 and K.dtype == np.float32 and Q.shape[1] == K.shape[1]
        self.indptr, self.indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        self.of, self.d, self.exact = entry_rows(indptr), Q.shape[1], exact
        with np.errstate(all="ignore"):
            p64 = (Q[self.of] * K[self.indices]).astype(np.float64)      # one fp32 multiply per product
            self.fin = np.isfinite(p64).all(axis=1)
            self.ieee = p64.sum(axis=1).astype(np.float32)                # of a non-finite score: -inf, +inf or NaN whatever the order
        clean = np.where(self.fin[:, None], p64, 0.0)
        self.A = np.abs(clean).sum(axis=1)
        self.S = np.array([math.fsum(row) for row in clean.tolist()], dtype=np.float64) if exact else clean.sum(axis=1)
        self.delta = fc.U * np.abs(self.S) + (1.0 if exact else 2.0) * self.d * 2.0 ** -52 * self.A + 2.0 ** -149


class Reference:
    def __init__(self, scores, V, scale):
        sc, s = float(np.float32(scale)), scores
        self.scores, ip, of = s, s.indptr, s.of
        self.n = np.diff(ip)
        self.d = V.shape[1]
        kk = 1.0 if s.exact else 2.0
        with np.errstate(all="ignore"):
            t_bad = np.float32(scale) * s.ieee                                # the non-finite scores' t, in fp32
            neg = ~s.fin & np.isneginf(t_bad)
            bad = ~s.fin & ~neg                                               # NaN or +inf
            assert not (s.fin & ~np.isfinite(sc * s.S)).any()
            T = np.where(s.fin, sc * s.S, -np.inf)
            eta = np.where(s.fin, (1.0 + fc.U) * abs(sc) * s.delta + fc.U * np.abs(T) + 2.0 ** -149, 0.0)
            self.empty = self.n == 0
            self.bad = _seg_sum(bad[:, None].astype(np.float64), ip)[:, 0] > 0             # Y NaN, lse NaN
            self.dead = ~self.empty & ~self.bad & (_seg_sum(s.fin[:, None].astype(np.float64), ip)[:, 0] == 0)      # only -inf: Y NaN, lse -inf
            self.finite = ~self.empty & ~self.bad & ~self.dead
            self.M = _seg_max(T, ip, -np.inf)
            live = self.finite[of]
            E = np.where(live, np.exp(T - np.where(live, self.M[of], 0.0)), 0.0)
            V64 = V.astype(np.float64)[s.indices]
            seg = _seg_fsum if s.exact else _seg_sum
            self.L = seg(E[:, None], ip)[:, 0]
            Lsafe = np.where(self.finite, self.L, 1.0)
            self.P = E / Lsafe[of]
            self.Y = seg(E[:, None] * V64, ip) / Lsafe[:, None]
            self.D = _seg_sum(self.P[:, None] * np.abs(V64 - self.Y[of]), ip)
            self.B = _seg_sum(self.P[:, None] * np.abs(V64), ip)
            self.LSE = np.where(self.finite, self.M, 0.0) + np.log(Lsafe)
            self.eta = _seg_max(eta, ip, 0.0)
        self.rho = np.expm1(self.eta)
        assert (self.rho[self.finite] <= RHO_MAX).all(), f"input condition: expm1(eta_r) reaches {self.rho[self.finite].max():.3g}"
        rho, n = self.rho[:, None], self.n[:, None]
        self.bound_y = fc.U * np.abs(self.Y) + rho / (1.0 - rho) * self.D + kk * (n + 16) * 2.0 ** -52 * self.B + 2.0 ** -149
        self.bound_lse = fc.U * np.abs(self.LSE) + self.eta + kk * (self.n + 16) * 2.0 ** -52 * (1.0 + np.abs(self.LSE)) + 2.0 ** -149

    def check(self, y, lse, what):
        """every word of y (rows x d float32) and, unless None, of lse; returns the largest error / bound seen"""
        y = np.asarray(y, dtype=np.float32)
        assert y.shape == self.Y.shape, (what, y.shape, self.Y.shape)
        f = self.finite
        assert not y.view(np.uint32)[self.empty].any(), f"{what}: a row without entries is not +0.0"
        assert np.isnan(y[self.bad | self.dead]).all(), f"{what}: a row with a NaN or +inf score, or with only -inf scores, is not NaN in every word"
        g = y.astype(np.float64)[f]
        assert np.isfinite(g).all(), f"{what}: non-finite words in finite rows"
        ratio_y = np.abs(g - self.Y[f]) / self.bound_y[f]
        worst = float(ratio_y.max()) if ratio_y.size else 0.0
        if worst > 1.0:
            i, j = (int(k[0]) for k in np.nonzero(ratio_y > 1.0))
            r = int(np.nonzero(f)[0][i])
            raise AssertionError(f"{what}: {int((ratio_y > 1.0).sum())} of {ratio_y.size} words of y break the contract, worst error / bound {worst:.3f}, first [{r}][{j}]: "
                                 f"got={g[i, j]!r} Y={self.Y[r, j]!r} bound={self.bound_y[r, j]:.3g} n={int(self.n[r])} rho={self.rho[r]:.3g}")
        worst_l = 0.0
        if lse is not None:
            lse = np.asarray(lse, dtype=np.float32)
            assert lse.shape == self.LSE.shape, (what, lse.shape)
            assert (lse.view(np.uint32)[self.empty | self.dead] == NEG_INF_WORD).all(), f"{what}: lse of a row without entries or with only -inf scores is not -inf"
            assert np.isnan(lse[self.bad]).all(), f"{what}: lse of a row with a NaN or +inf score is not NaN"
            gl = lse.astype(np.float64)[f]
            assert np.isfinite(gl).all(), f"{what}: non-finite lse words in finite rows"
            ratio_l = np.abs(gl - self.LSE[f]) / self.bound_lse[f]
            worst_l = float(ratio_l.max()) if ratio_l.size else 0.0
            if worst_l > 1.0:
                i = int(np.nonzero(ratio_l > 1.0)[0][0])
                r = int(np.nonzero(f)[0][i])
                raise AssertionError(f"{what}: {int((ratio_l > 1.0).sum())} of {ratio_l.size} lse words break the contract, worst error / bound {worst_l:.3f}, first [{r}]: "
                                     f"got={gl[i]!r} LSE={self.LSE[r]!r} bound={self.bound_lse[r]:.3g} n={int(self.n[r])} eta={self.eta[r]:.3g}")
        print(f"{what}: error / bound = {worst:.3f} (y), {worst_l:.3f} (lse) over {int(f.sum())} finite rows")
        return max(worst, worst_l)

    def rounded(self):
        """a correct result: the reference's own words rounded once (what the planted defects are applied to)"""
        y = np.where(self.finite[:, None], self.Y, np.where(self.empty[:, None], 0.0, np.nan)).astype(np.float32)
        lse = np.where(self.finite, self.LSE, np.where(self.bad, np.nan, -np.inf)).astype(np.float32)
        return y, lse


def reference(indptr, indices, Q, K, V, scale, exact=True):
    return Reference(Scores(indptr, indices, Q, K, exact), V, scale)


# ---- inputs and the two forms --------------------------------------------------------------------------------------------------------
def operands(shape, d, seed):
    rows, cols = shape
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(0.0, 1.0, (n, d)).astype(np.float32) for n in (rows, cols, cols))


def host_form(pa, Q, K, V, scale, want_lse=True):
    """(y, lse or None)"""
    if want_lse:
        return pa.forward(Q, K, V, scale)
    return pa.forward(Q, K, V, scale, want_lse=False), None


def device_form(mem, pa, Q, K, V, scale, pad=0, want_lse=True, what=""):
    """hsat_forward_device over fresh buffers: input pads NaN, y and lse pre-filled with a sentinel; y's pad words must survive"""
    d = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv) = (wc._features_in(mem, a, pad) for a in (Q, K, V))
    ldy = wc.round_up4(d) + pad
    dy = mem.alloc(np.full((pa.num_rows, ldy), SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full(pa.num_rows, SENTINEL, dtype=np.uint32)) if want_lse else None
    pa.forward_device(dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, d, scale, dy.ptr, ldy, dl.ptr if want_lse else None)
    y = wc._features_out(mem, pa, dy, pa.num_rows, d, ldy, what)
    return y, (mem.read(pa, dl).view(np.float32) if want_lse else None)


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def all_forms(mem, pa, ref, Q, K, V, scale, pads, what):
    """the host form and the device form at every pad, each with lse taken and with NULL, inside the bounds of one reference"""
    for want in (True, False):
        tag = "lse taken" if want else "lse NULL"
        ref.check(*host_form(pa, Q, K, V, scale, want), f"{what}, host form, {tag}")
        for pad in pads:
            ref.check(*device_form(mem, pa, Q, K, V, scale, pad, want, what), f"{what}, device form, pad {pad}, {tag}")


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def general(mem, ds=DS):
    """300 x 517, 4000 entries, every d of DS, scale 0.125, 1 and -2, pad 0 and 8, lse taken and NULL, both forms"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    with attention.PatternAttention((indptr, indices, shape)) as pa:
        assert pa.nnz == NNZ and pa.info()["nnz"] == NNZ
        for d in ds:
            Q, K, V = operands(shape, d, 1100 + d)
            scores = Scores(indptr, indices, Q, K)
            for scale in (0.125, 1.0, -2.0):
                all_forms(mem, pa, Reference(scores, V, scale), Q, K, V, scale, (0, 8), f"general, d {d}, scale {scale}")


def edges(mem):
    """every pattern of pattern_cases.edge_patterns() at d = 1 and 5: nnz = 0 ... 7, runs of empty rows, one row that holds all 301 entries,
    unsorted columns, a pair held twice; the rows without entries read +0.0 and -inf bit for bit (Reference.check)"""
    for name, rows, cols, indptr, indices in edge_patterns():
        shape = (rows, cols)
        with attention.PatternAttention((indptr, indices, shape)) as pa:
            assert pa.nnz == indices.size
            for d in (1, 5):
                Q, K, V = operands(shape, d, 1300 + d)
                ref = reference(indptr, indices, Q, K, V, 1.5)
                assert ref.empty.sum() == (np.diff(indptr.astype(np.int64)) == 0).sum()
                all_forms(mem, pa, ref, Q, K, V, 1.5, (8,), f"{name}, d {d}")


ORDER_LENGTHS = (5, 17, 65, 513, 1025, 3000)
ORDERS = ("ascending", "descending", "maximum last", "maximum first")


def ordered_pattern(order, Q, K, seed):
    """one row each of ORDER_LENGTHS over K's rows as columns, the entries of a row arranged by their scores"""
    rng = np.random.default_rng(seed)
    indices = []
    indptr = np.concatenate([[0], np.cumsum(ORDER_LENGTHS)]).astype(np.uint32)
    for r, n in enumerate(ORDER_LENGTHS):
        cols = rng.choice(K.shape[0], n, replace=False)
        s = (Q[r] * K[cols]).astype(np.float64).sum(axis=1)      # from the fp32 products, as the reference's S
        if order == "ascending":
            cols = cols[np.argsort(s, kind="stable")]
        elif order == "descending":
            cols = cols[np.argsort(-s, kind="stable")]
        else:
            at, to = int(np.argmax(s)), (n - 1 if order == "maximum last" else 0)
            cols[[at, to]] = cols[[to, at]]
        indices.append(cols)
    return indptr, np.concatenate(indices).astype(np.uint32)


def score_order(mem, ds=(4, 64)):
    """rows of 5, 17, 65, 513, 1025 and 3000 entries over 4096 columns, scale 8 (a peaked softmax), the scores ascending (a rescale on every
    trip), descending (none), with the maximum at the very last entry and at entry 0"""
    shape = (len(ORDER_LENGTHS), 4096)
    for d in ds:
        Q, K, V = operands(shape, d, 1400 + d)
        for k, order in enumerate(ORDERS):
            indptr, indices = ordered_pattern(order, Q, K, 1410 + k)
            ref = reference(indptr, indices, Q, K, V, 8.0)
            t = 8.0 * ref.scores.S
            for r in range(shape[0]):
                row = t[indptr[r]: indptr[r + 1]]
                assert {"ascending": (np.diff(row) >= 0).all(), "descending": (np.diff(row) <= 0).all(), "maximum last": row.argmax() == row.size - 1,
                        "maximum first": row.argmax() == 0}[order], (order, r)
            with attention.PatternAttention((indptr, indices, shape)) as pa:
                what = f"score order {order}, d {d}"
                ref.check(*host_form(pa, Q, K, V, 8.0), what + ", host form")
                ref.check(*device_form(mem, pa, Q, K, V, 8.0, 4, True, what), what + ", device form")


def non_finite(mem, ds=(5, 64, 256)):
    """Scores made non-finite through K (a -inf, +inf or NaN feature against a positive word of Q).  Row 1: its first 40 entries score -inf, the
    other 30 are finite (the state is still empty when whole trips of -inf pass); row 2: only -inf; row 3: one NaN; row 4: one +inf; row 5:
    600 entries, the first 300 of them -inf (the same on a long row); row 0 has no entries and rows 6 ... 29 are ordinary ones, some with
    a -inf entry.  Exactly the header's table; every other row finite and within bound."""
    n_rows, n_cols = 30, 400
    rng = np.random.default_rng(1500)
    ninf_cols, pinf_col, nan_col = np.arange(300, 345), 345, 346      # columns 0 ... 299 and 347 ... are finite
    fin_cols = np.concatenate([np.arange(300), np.arange(347, n_cols)])
    rows = [np.zeros(0, dtype=np.int64),
            np.concatenate([rng.choice(ninf_cols, 40, replace=False), rng.choice(fin_cols, 30, replace=False)]),
            rng.choice(ninf_cols, 7, replace=False),
            rng.permutation(np.concatenate([rng.choice(fin_cols, 20, replace=False), [nan_col]])),
            rng.permutation(np.concatenate([rng.choice(fin_cols, 20, replace=False), [pinf_col]])),
            np.concatenate([rng.choice(ninf_cols, 300, replace=True), rng.choice(fin_cols, 300, replace=False)])]
    for r in range(6, n_rows):
        cols = rng.choice(fin_cols, int(rng.integers(1, 40)), replace=False)
        if r % 3 == 0:
            cols = rng.permutation(np.concatenate([cols, rng.choice(ninf_cols, 2)]))
        rows.append(cols)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.uint32)
    indices = np.concatenate(rows).astype(np.uint32)
    shape = (n_rows, n_cols)
    with attention.PatternAttention((indptr, indices, shape)) as pa:
        for d in ds:
            Q, K, V = operands(shape, d, 1510 + d)
            j0 = d - 1                                          # the last feature: in the last, partly used chunk when d % 4 != 0
            Q[:, j0] = np.abs(Q[:, j0]) + 0.5
            K[ninf_cols, j0], K[pinf_col, j0], K[nan_col, j0] = -np.inf, np.inf, np.nan
            for scale in (1.0, 0.25):
                ref = reference(indptr, indices, Q, K, V, scale)
                assert ref.empty[0] and ref.finite[1] and ref.dead[2] and ref.bad[3] and ref.bad[4] and ref.finite[5] and ref.finite[6:].all()
                what = f"non-finite scores, d {d}, scale {scale}"
                for y, lse in (host_form(pa, Q, K, V, scale), device_form(mem, pa, Q, K, V, scale, 4, True, what)):
                    ref.check(y, lse, what)
                    assert np.isnan(y[2:5]).all() and lse[2] == -np.inf and np.isnan(lse[3:5]).all() and lse[0] == -np.inf and not y[0].any()
                    assert np.isfinite(np.delete(y, [2, 3, 4], axis=0)).all() and np.isfinite(np.delete(lse, [0, 2, 3, 4])).all()


def scale_zero(mem):
    """scale = 0: every weight of a row is equal, Y is the mean of the row's rows of V and lse = log n, within the contract (eta = 2^-149)"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 7)
    shape = (ROWS, COLS)
    with attention.PatternAttention((indptr, indices, shape)) as pa:
        for d in (5, 64):
            Q, K, V = operands(shape, d, 1600 + d)
            ref = reference(indptr, indices, Q, K, V, 0.0)
            f = ref.finite
            assert (ref.eta[f] == 2.0 ** -149).all() and np.allclose(ref.LSE[f], np.log(ref.n[f]), rtol=1e-14, atol=0)
            mean = _seg_sum(V.astype(np.float64)[indices.astype(np.int64)], indptr)[f] / ref.n[f][:, None]
            assert np.allclose(ref.Y[f], mean, rtol=1e-12, atol=1e-14)
            all_forms(mem, pa, ref, Q, K, V, 0.0, (4,), f"scale 0, d {d}")


def heads(mem):
    """H = 3 heads of d = 8 stored [index][head][feature]: three calls with ld = 24 and pointers offset by h d words over interleaved
    buffers; each head against its own reference, the other heads' words in the part of the pad (those of the inputs are read by no
    result, those of y survive the call)"""
    H, d = 3, 8
    ld = H * d
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 8)
    shape = (ROWS, COLS)
    Q, K, V = operands(shape, ld, 1700)
    dq, dk, dv = (mem.alloc(words(a)) for a in (Q, K, V))
    dy = mem.alloc(np.full((ROWS, ld), SENTINEL, dtype=np.uint32))
    dl = [mem.alloc(np.full(ROWS, SENTINEL, dtype=np.uint32)) for _ in range(H)]
    with attention.PatternAttention((indptr, indices, shape)) as pa:
        for h in range(H):
            off = 4 * h * d
            pa.forward_device(dq.ptr + off, ld, dk.ptr + off, ld, dv.ptr + off, ld, d, 0.5, dy.ptr + off, ld, dl[h].ptr)
            got = mem.read(pa, dy).reshape(ROWS, ld)
            assert (got[:, (h + 1) * d:] == SENTINEL).all() and (got[:, h * d: (h + 1) * d] != SENTINEL).any(), f"head {h} wrote another head's words"
            if h:
                assert np.array_equal(got[:, : h * d], before[:, : h * d]), f"head {h} changed an earlier head's words"
            before = got
        for h in range(H):
            cut = slice(h * d, (h + 1) * d)
            ref = reference(indptr, indices, *(np.ascontiguousarray(a[:, cut]) for a in (Q, K, V)), 0.5)
            ref.check(np.ascontiguousarray(got[:, cut]).view(np.float32), mem.read(pa, dl[h]).view(np.float32), f"head {h} of {H}")


def nothing_carried_over(mem):
    """two calls with the same inputs give the same words; a call with another d and scale on the same object gives the words of a fresh one"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with attention.PatternAttention((indptr, indices, shape)) as pa, attention.PatternAttention((indptr, indices, shape)) as fresh:
        Q, K, V = operands(shape, 64, 1800)
        y1, l1 = device_form(mem, pa, Q, K, V, 1.0)
        y2, l2 = device_form(mem, pa, Q, K, V, 1.0)
        assert np.array_equal(words(y1), words(y2)) and np.array_equal(words(l1), words(l2))
        Q2, K2, V2 = operands(shape, 5, 1810)
        y3, l3 = device_form(mem, pa, Q2, K2, V2, -0.75, 4)
        y4, l4 = device_form(mem, fresh, Q2, K2, V2, -0.75, 4)
        assert np.array_equal(words(y3), words(y4)) and np.array_equal(words(l3), words(l4))
        reference(indptr, indices, Q2, K2, V2, -0.75).check(y3, l3, "second call")


def _create(rows, cols, indptr, indices):
    l = attention.lib()
    h = C.c_void_p(0xBAD)
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint32)
    indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    rc = l.hsat_create(C.byref(h), 0, rows, cols, None if indptr is None else indptr.ctypes.data, None if indices is None else indices.ctypes.data)
    return rc, h


def refusals(mem):
    l = attention.lib()
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
        assert rc == code and not h.value and l.hsat_last_error(None), (what, rc, h.value)
    assert l.hsat_create(None, 0, 6, 9, indptr.ctypes.data, indices.ctypes.data) == BAD_ARG and l.hsat_last_error(None)
    # null-object calls
    one = np.zeros(4, dtype=np.float32).ctypes.data
    assert l.hsat_info(None, None, None) == BAD_ARG and l.hsat_sync(None) == BAD_ARG and l.hsat_set_stream(None, None) == BAD_ARG
    assert l.hsat_forward_device(None, vp(one), 4, vp(one), 4, vp(one), 4, 1, 1.0, vp(one), 4, None) == BAD_ARG
    assert l.hsat_forward(None, vp(one), vp(one), vp(one), 1, 1.0, vp(one), None) == BAD_ARG
    assert l.hsat_destroy(None) == 0

    d = 5
    with attention.PatternAttention((indptr, indices, shape)) as pa:
        Q, K, V = operands(shape, d, 1900)
        want_y, want_l = host_form(pa, Q, K, V, 0.5)
        reference(indptr, indices, Q, K, V, 0.5).check(want_y, want_l, "refusals")

        def still_usable(rc, what):
            assert rc == BAD_ARG and l.hsat_last_error(pa._h), (what, rc)
            y, lse = host_form(pa, Q, K, V, 0.5)
            assert np.array_equal(words(y), words(want_y)) and np.array_equal(words(lse), words(want_l)), f"unusable after {what}"

        # buffers of 9 rows x 16 words (the larger dimension, ld up to 16), 16-byte aligned
        bq, bk, bv, by, bl = (mem.alloc(np.zeros(9 * 16, np.uint32)) for _ in range(5))
        q, k, v, y, ls = bq.ptr, bk.ptr, bv.ptr, by.ptr, bl.ptr
        nan, inf = float("nan"), float("inf")
        ok = dict(q=q, ldq=8, k=k, ldk=8, v=v, ldv=8, d=d, scale=1.0, y=y, ldy=8, lse=ls)
        cases = [("d = 0", dict(d=0)), ("d = 257", dict(d=257, ldq=260, ldk=260, ldv=260, ldy=260)), ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf)),
                 ("scale -inf", dict(scale=-inf)), ("misaligned lse", dict(lse=ls + 2)), ("y is q", dict(y=q)), ("y inside k", dict(y=k + 16 * 4)), ("y is v", dict(y=v)),
                 ("y's last row in v", dict(v=q + 16, y=q + 16 + 8 * 8 * 4)), ("lse inside y", dict(lse=y + 4 * 4)), ("lse is y's last word", dict(lse=y + (5 * 8 + d - 1) * 4)),
                 ("lse inside q", dict(lse=q + 8))]
        for name in ("q", "k", "v", "y"):
            ptr, ld = ok[name], "ld" + name
            cases += [(f"null {name}", {name: None}), (f"misaligned {name}", {name: ptr + 4}), (f"misaligned {name} by 8", {name: ptr + 8}), (f"{ld} % 4", {ld: 10}),
                      (f"{ld} < d", {ld: 4})]
        for what, change in cases:
            a = dict(ok, **change)
            still_usable(l.hsat_forward_device(pa._h, vp(a["q"]), a["ldq"], vp(a["k"]), a["ldk"], vp(a["v"]), a["ldv"], a["d"], a["scale"], vp(a["y"]), a["ldy"], vp(a["lse"])),
                         "device form: " + what)
        # the host form
        hq, hk, hv, hy, hl = (np.zeros(9 * 8, np.float32) for _ in range(5))
        okh = dict(q=hq.ctypes.data, k=hk.ctypes.data, v=hv.ctypes.data, d=d, scale=1.0, y=hy.ctypes.data, lse=hl.ctypes.data)
        for what, change in (("d = 0", dict(d=0)), ("d = 257", dict(d=257)), ("null q", dict(q=None)), ("null k", dict(k=None)), ("null v", dict(v=None)), ("null y", dict(y=None)),
                             ("scale NaN", dict(scale=nan)), ("scale inf", dict(scale=inf)), ("y is k", dict(y=okh["k"])), ("lse inside y", dict(lse=okh["y"] + 8))):
            a = dict(okh, **change)
            still_usable(l.hsat_forward(pa._h, vp(a["q"]), vp(a["k"]), vp(a["v"]), a["d"], a["scale"], vp(a["y"]), vp(a["lse"])), "host form: " + what)
        # ranges that touch without sharing a byte are fine, and so is a NULL lse
        assert l.hsat_forward_device(pa._h, vp(q), 8, vp(k), 8, vp(v), 8, d, 1.0, vp(y), 8, vp(y + (5 * 8 + 8) * 4)) == 0
        assert l.hsat_forward_device(pa._h, vp(q), 8, vp(k), 8, vp(v), 8, d, 1.0, vp(y), 8, None) == 0
        pa.set_stream(None)
        pa.sync()
