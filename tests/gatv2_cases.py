"""The cases of the GATv2 calls (include/hisparse_gatv2.h), shared by tests/test_gatv2_cpu.py (libhisparse_cpu.so, in a child process) and
tests/test_gpu_gatv2.py (the HIP library, on the device), written against the memory interface of tests/pattern_cases.py.

Reference, one per head, from the header's formulas and BOUNDS.  z = XD[row(e)] + XS[col(e)], w = z > 0 ? z : slope * z and the products
a_j w_j are formed in numpy float32, exactly the fp32 operations of the contract; everything else is float64.  `Scores` holds what
attention_cases.Scores holds, for the operands a and w: S_e = math.fsum of the products, A_e = the sum of their magnitudes and
delta_e = u|S_e| + d 2^-52 A_e + 2^-149.  The forward IS attention_cases.Reference over these scores at scale = 1 with V = XS: its eta,
its bounds of Y and lse and its special-value table unchanged.  The backward restates attention_backward_cases.Reference at scale = 1
(rho_e, gam_e, epsD_r, eps_e and mag_e are its own) with the feature word that multiplies GS_e replaced by a_j dz_ej (gXD, gXS) or w_ej (ga):
    |gxd - GXD| <= u|GXD| + sum_r eps_e |a_j| dz_ej + (n_r + 16) 2^-52 sum_r mag_e |a_j| dz_ej + 2^-149
    |gxs - GXS| <= u|GXS| + sum_c (rho_e P|gY_j| + eps_e |a_j| dz_ej) + (m_c + 16) 2^-52 sum_c (P|gY_j| + mag_e |a_j| dz_ej) + 2^-149
    |ga - GA|   <= u|GA| + sum_e eps_e |w_ej| + sum_r (n_r + 16) 2^-52 sum_r mag_e |w_ej| + ((R + 16) + (G + 16)) 2^-52 sum_e mag_e |w_ej| + 2^-149
with R the rows that hold entries and G = 2048, the most workgroup vectors the header allows.  No tolerance is introduced here.  Sums are
math.fsum with exact=True; exact=False (float64 sums, the 2^-52 terms doubled) is used by the large cases of the GPU tests only.  The
special tables are asserted bit for bit: a row without entries +0.0 in Y and gXD and -inf in lse, a column without entries +0.0 in gXS, ga
all +0.0 at nnz = 0, a NaN or +inf t NaN in Y and lse, a non-finite lse word NaN in gXD[r], in gXS[c] of every column the row touches and
in all of ga.

`reference_against_autograd` holds the reference's exact values against torch.autograd in float64 over the plain dense-gather
expression; both test files run it before any library is tested."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import gatv2, heads as mha

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
TINY = 2.0 ** -149
G_MAX = 2048                   # the most workgroup vectors of the row side: 8 per compute unit, 256 compute units
OUTPUTS = ("gxd", "gxs", "ga")


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def leaky(z, slope):
    """w = z > 0 ? z : fl32(slope * z) over float32 words; z == 0 and NaN take the slope branch"""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.where(z > 0, z, np.float32(slope) * z).astype(np.float32)


class Scores:
    """attention_cases.Scores for one head of the GATv2 score: the operands of the dot are a (d,) and w[e] = LeakyReLU(XD[row(e)] +
    XS[col(e)]), both float32.  z, w and dz are exact; S, A and delta are those of the d fp32 products a_j w_ej."""

    def __init__(self, indptr, indices, XD, XS, a, slope, exact=True):
        assert XD.dtype == XS.dtype == a.dtype == np.float32 and XD.shape[1] == XS.shape[1] == a.size and a.ndim == 1
        self.indptr, self.indices = ip, ix = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        assert XD.shape[0] == ip.size - 1
        self.of, self.d, self.exact, self.slope, self.a, self.XS = entry_rows(ip), a.size, exact, np.float32(slope), a, XS
        with np.errstate(all="ignore"):
            self.z = (XD[self.of] + XS[ix]).astype(np.float32)                  # one fp32 add
            self.w = leaky(self.z, slope)                                         # one fp32 multiply
            p64 = (a[None, :] * self.w).astype(np.float64)                        # one fp32 multiply per product
            self.fin = np.isfinite(p64).all(axis=1)
            self.ieee = p64.sum(axis=1).astype(np.float32)                        # of a non-finite score: -inf, +inf or NaN whatever the order
        self.dz = np.where(self.z > 0, 1.0, float(np.float32(slope)))
        clean = np.where(self.fin[:, None], p64, 0.0)
        self.A = np.abs(clean).sum(axis=1)
        self.S = np.array([math.fsum(row) for row in clean.tolist()], dtype=np.float64) if exact else clean.sum(axis=1)
        self.delta = fc.U * np.abs(self.S) + (1.0 if exact else 2.0) * self.d * 2.0 ** -52 * self.A + TINY


class Backward:
    """One head's backward from a forward reference (attention_cases.Reference over Scores), gY (rows, d) and the lse words (rows,) as
    the call is given them (float32; float64 only where the reference itself is held against autograd).  ga is kept as a (1, d) array so
    that the three outputs are checked by one loop.  u and delta are arguments so that bounds(0, 0) gives the 2^-52 terms alone."""

    def __init__(self, f, gY, lse):
        s = f.scores
        XS = s.XS
        assert gY.dtype == np.float32 and gY.shape == (f.n.size, s.d) and s.fin.all(), "the backward cases hold no non-finite score"
        lse = np.asarray(lse)
        assert lse.shape == (f.n.size,) and lse.dtype in (np.float32, np.float64)
        ip, ix, of = s.indptr, s.indices, s.of
        self.f, self.s, self.d = f, s, s.d
        self.kk = 1.0 if s.exact else 2.0
        self.seg = seg = ac._seg_fsum if s.exact else ac._seg_sum
        self.n = f.n
        self.perm = pm = np.argsort(ix, kind="stable")
        self.m = np.bincount(ix, minlength=XS.shape[0]).astype(np.int64)
        self.cptr = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.empty_r, self.empty_c = self.n == 0, self.m == 0
        self.bad_r = ~self.empty_r & ~np.isfinite(lse)
        self.bad_c = np.zeros(XS.shape[0], dtype=bool)
        self.bad_c[ix[self.bad_r[of]]] = True
        self.live = live = ~self.bad_r[of]
        self.g64 = g64 = (gY[of] * XS[ix]).astype(np.float64)                      # one fp32 multiply per product
        self.GP = GP = np.array([math.fsum(row) for row in g64.tolist()], dtype=np.float64) if s.exact else g64.sum(axis=1)
        with np.errstate(all="ignore"):
            self.P = P = np.where(live, np.exp(s.S - np.where(live, lse.astype(np.float64)[of], 0.0)), 0.0)
        assert np.isfinite(P).all()
        self.G64 = gY.astype(np.float64)[of]
        self.D = seg((P * GP)[:, None], ip)[:, 0]
        self.GT = P * (GP - self.D[of])
        self.C = s.a.astype(np.float64)[None, :] * s.dz                            # a_j dz_ej, exact in float64
        self.W = s.w.astype(np.float64)
        self.GXD, self.GXS, self.GA = self.gradients(self.GT, P)
        self.want = {"gxd": self.GXD, "gxs": self.GXS, "ga": self.GA}
        self.empty = {"gxd": self.empty_r, "gxs": self.empty_c, "ga": np.array([ix.size == 0])}
        self.bad = {"gxd": self.bad_r, "gxs": self.bad_c, "ga": np.array([bool(self.bad_r.any())])}
        self.bound = self.bounds(fc.U, s.delta)

    def gradients(self, GT, P):
        """(gXD (rows, d), gXS (cols, d), ga (1, d)) in float64 from per-entry gt and p, by this reference's sums"""
        pm, ip = self.perm, self.s.indptr
        live = self.live[:, None]
        x = np.where(live, GT[:, None] * self.W, 0.0)
        ga = np.array([[math.fsum(c) for c in x.T.tolist()]]) if self.s.exact else x.sum(axis=0)[None, :]
        return self.seg(GT[:, None] * self.C, ip), self.seg((P[:, None] * self.G64 + GT[:, None] * self.C)[pm], self.cptr), ga.reshape(1, self.d)

    def bounds(self, u, delta):
        s, ip, of, pm, kk, P, GP = self.s, self.s.indptr, self.s.of, self.perm, self.kk, self.P, self.GP
        eta = (1.0 + u) * delta + u * np.abs(s.S) + (TINY if u else 0.0)
        rho = np.expm1(eta + 32.0 * 2.0 ** -52)
        assert (rho[self.live] <= ac.RHO_MAX).all(), f"input condition: rho_e reaches {rho[self.live].max():.3g}"
        gam = u * np.abs(GP) + kk * self.d * 2.0 ** -52 * np.abs(self.g64).sum(axis=1) + TINY
        Dof = self.D[of]
        eps_d = ac._seg_sum((P * (rho * np.abs(GP) + (1.0 + rho) * gam))[:, None], ip)[:, 0] + kk * (self.n + 16) * 2.0 ** -52 * ac._seg_sum((P * np.abs(GP))[:, None], ip)[:, 0]
        eps = (rho * P * np.abs(GP - Dof) + (1.0 + rho) * P * (gam + eps_d[of]))[:, None]
        mag = (P * (np.abs(GP) + np.abs(Dof)))[:, None]
        aC, aW, aG = np.abs(self.C), np.abs(self.W), np.abs(self.G64)
        n, m = self.n[:, None], self.m[:, None]
        rows_with_entries = int((self.n > 0).sum())
        mag_w = ac._seg_sum(mag * aW, ip)
        return {"gxd": u * np.abs(self.GXD) + ac._seg_sum(eps * aC, ip) + kk * (n + 16) * 2.0 ** -52 * ac._seg_sum(mag * aC, ip) + TINY,
                "gxs": u * np.abs(self.GXS) + ac._seg_sum(((rho * P)[:, None] * aG + eps * aC)[pm], self.cptr)
                + kk * (m + 16) * 2.0 ** -52 * ac._seg_sum((P[:, None] * aG + mag * aC)[pm], self.cptr) + TINY,
                "ga": u * np.abs(self.GA) + (eps * aW).sum(axis=0)[None, :] + (kk * (n + 16) * 2.0 ** -52 * mag_w).sum(axis=0)[None, :]
                + kk * ((rows_with_entries + 16) + (G_MAX + 16)) * 2.0 ** -52 * mag_w.sum(axis=0)[None, :] + TINY}

    def check(self, gxd, gxs, ga, what, extra=None):
        """every word of the three outputs (gxd (rows, d), gxs (cols, d), ga (d,)); returns the largest error / bound per output"""
        worst = {}
        for name, got in zip(OUTPUTS, (gxd, gxs, np.asarray(ga).reshape(1, -1))):
            got = np.asarray(got, dtype=np.float32)
            want, bound, empty, bad = self.want[name], self.bound[name], self.empty[name], self.bad[name]
            if extra is not None:
                bound = bound + extra[name]
            assert got.shape == want.shape, (what, name, got.shape, want.shape)
            assert not got.view(np.uint32)[empty].any(), f"{what}: {name} is not +0.0 where no entry reaches it"
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
        print(f"{what}: error / bound = {worst['gxd']:.3f} (gxd), {worst['gxs']:.3f} (gxs), {worst['ga']:.3f} (ga)")
        return worst

    def rounded(self, grads=None):
        """a correct result: the reference's own words rounded once, (gxd (rows, d), gxs (cols, d), ga (d,))"""
        out = [np.where(self.bad[name][:, None], np.nan, x).astype(np.float32) for name, x in zip(OUTPUTS, grads or (self.GXD, self.GXS, self.GA))]
        return out[0], out[1], out[2][0]


cut = hc.cut


def forward_refs(indptr, indices, XD, XS, a, heads, slope, exact=True):
    """attention_cases.Reference per head over this file's Scores, scale = 1, V = XS"""
    d = XS.shape[1] // heads
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(heads, d)
    assert XD.shape[1] == XS.shape[1] == heads * d
    return [ac.Reference(Scores(indptr, indices, cut(XD, h, d), cut(XS, h, d), a[h], slope, exact), cut(XS, h, d), 1.0) for h in range(heads)]


def backward_refs(frefs, gY, lse):
    """lse: (rows, heads), the words the backward call is given"""
    d = frefs[0].d
    lse = np.asarray(lse)
    assert lse.shape == (frefs[0].n.size, len(frefs))
    return [Backward(f, cut(gY, h, d), np.ascontiguousarray(lse[:, h])) for h, f in enumerate(frefs)]


check_forward = hc.check_forward
rounded_forward = hc.rounded_forward


def check_backward(refs, gxd, gxs, ga, what):
    d = refs[0].d
    gxd, gxs = (np.asarray(x, dtype=np.float32) for x in (gxd, gxs))
    ga = np.asarray(ga, dtype=np.float32).reshape(len(refs), d)
    assert gxd.shape == (refs[0].n.size, len(refs) * d) and gxs.shape == (refs[0].m.size, len(refs) * d), (what, gxd.shape, gxs.shape)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for h, r in enumerate(refs):
        w = r.check(cut(gxd, h, d), cut(gxs, h, d), ga[h], f"{what}, head {h}")
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


def rounded_backward(refs, grads=None):
    parts = [r.rounded(None if grads is None else grads[h]) for h, r in enumerate(refs)]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1), np.stack([p[2] for p in parts], axis=0)


def reference_against_autograd(slope=0.25):
    """The formulas, ga above all, ARE the gradient: on the 300 x 517, 4000-entry pattern at 3 heads of d = 8 the reference's exact values
    (Y, LSE, GXD, GXS, GA, the backward from its own float64 LSE) against torch.autograd in float64 on the CPU over the plain dense-gather
    expression.  XD holds multiples of 1/4 and XS odd multiples of 1/8, so every z is an odd multiple of 1/8, never 0, and with a on the
    1/8 grid and slope 1/4 the fp32 sums and products of the contract are exact: the contract's function is autograd's.  Agreement is
    within the 2^-52 terms of the bounds alone (u = 0 and delta = 0 in Backward.bounds; rho = expm1(32 * 2^-52) in the forward's)."""
    import torch
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    H, d = 3, 8
    rng = np.random.default_rng(14000)
    XD = (rng.integers(-15, 16, (ROWS, H * d)) / 4.0).astype(np.float32)
    XS = ((2 * rng.integers(-15, 16, (COLS, H * d)) + 1) / 8.0).astype(np.float32)
    a, gY = wc.grid_values(rng, (H, d)) / np.float32(4.0), wc.grid_values(rng, (ROWS, H * d))      # a: six significant bits, so that a w stays exact
    frefs = forward_refs(indptr, indices, XD, XS, a, H, slope)
    assert all((f.scores.z != 0).all() and (f.scores.z < 0).any() and (f.scores.z > 0).any() for f in frefs)
    brefs = backward_refs(frefs, gY, np.stack([f.LSE for f in frefs], axis=1))
    of, ix = torch.tensor(frefs[0].scores.of), torch.tensor(frefs[0].scores.indices)
    txd, txs = (torch.tensor(x.astype(np.float64).reshape(-1, H, d), requires_grad=True) for x in (XD, XS))
    ta = torch.tensor(a.astype(np.float64), requires_grad=True)
    t = (torch.nn.functional.leaky_relu(txd[of] + txs[ix], slope) * ta).sum(dim=2)                       # (nnz, H)
    m = torch.full((ROWS, H), -np.inf, dtype=torch.float64).scatter_reduce(0, of[:, None].expand(-1, H), t.detach(), "amax")
    E = torch.exp(t - m[of])
    L = torch.zeros((ROWS, H), dtype=torch.float64).index_add(0, of, E)
    ty = torch.zeros((ROWS, H, d), dtype=torch.float64).index_add(0, of, (E / L[of])[:, :, None] * txs[ix])
    (ty * torch.tensor(gY.astype(np.float64).reshape(ROWS, H, d))).sum().backward()
    auto_y, auto_l = ty.detach().numpy().reshape(ROWS, H * d), (m + torch.log(L)).detach().numpy()
    auto = {"gxd": txd.grad.numpy().reshape(ROWS, H * d), "gxs": txs.grad.numpy().reshape(COLS, H * d), "ga": ta.grad.numpy()}
    rho0 = math.expm1(32.0 * 2.0 ** -52)
    worst = dict.fromkeys(("y", "lse") + OUTPUTS, 0.0)
    for h, (f, r) in enumerate(zip(frefs, brefs)):
        assert f.finite.sum() == (f.n > 0).sum() and not r.bad_r.any()
        n = f.n[:, None]
        by = rho0 / (1.0 - rho0) * f.D + (n + 16) * 2.0 ** -52 * f.B + TINY
        bl = (f.n + 16) * 2.0 ** -52 * (1.0 + np.abs(f.LSE)) + TINY
        live = f.finite
        worst["y"] = max(worst["y"], float((np.abs(f.Y - cut(auto_y, h, d))[live] / by[live]).max()))
        worst["lse"] = max(worst["lse"], float((np.abs(f.LSE - auto_l[:, h])[live] / bl[live]).max()))
        b0 = r.bounds(0.0, 0.0)
        for name, got in (("gxd", cut(auto["gxd"], h, d)), ("gxs", cut(auto["gxs"], h, d)), ("ga", auto["ga"][h][None, :])):
            worst[name] = max(worst[name], float((np.abs(r.want[name] - got) / b0[name]).max()))
    print("the reference against float64 autograd, difference / the 2^-52 terms of the bound: " + ", ".join(f"{v:.3f} ({k})" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    return worst


# ---- inputs and the forms ------------------------------------------------------------------------------------------------------------
def operands(shape, heads, d, seed):
    """XD (rows, heads d), XS (cols, heads d), a (heads, d), gY (rows, heads d): normal, a scaled by 1 / sqrt(d) so that t is of order 1;
    z = XD + XS takes both signs in every head of every entry with overwhelming probability (asserted by the callers per case)"""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    XD, XS, gY = (rng.normal(0.0, 1.0, (n, heads * d)).astype(np.float32) for n in (rows, cols, rows))
    a = (rng.normal(0.0, 1.0, (heads, d)) / math.sqrt(d)).astype(np.float32)
    return XD, XS, a, gY


def both_signs(frefs):
    """z > 0 and z < 0 both occur in every head"""
    return all((f.scores.z > 0).any() and (f.scores.z < 0).any() for f in frefs if f.scores.z.size)


words = hc.words
same_words = hc.same_words


def _vector_in(mem, a):
    return mem.alloc(np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32))


def forward_host(ga, XD, XS, a, heads, slope, want_lse=True):
    """(y, lse or None)"""
    if want_lse:
        return ga.forward(XD, XS, a, heads, slope)
    return ga.forward(XD, XS, a, heads, slope, want_lse=False), None


def forward_device(mem, ga, XD, XS, a, heads, slope, pad=0, extra=0, want_lse=True, what=""):
    """hsgat2_forward_device over fresh buffers: input pads NaN, y and lse pre-filled with a sentinel; the pad words of both must survive"""
    w = XS.shape[1]
    (dd, ldd), (ds, lds) = wc._features_in(mem, XD, pad), wc._features_in(mem, XS, pad)
    da = _vector_in(mem, a)
    ldy, ldl = w + pad, heads + extra
    dy = mem.alloc(np.full((ga.num_rows, ldy), SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full((ga.num_rows, ldl), SENTINEL, dtype=np.uint32)) if want_lse else None
    ga.forward_device(dd.ptr, ldd, ds.ptr, lds, da.ptr, heads, w // heads, slope, dy.ptr, ldy, dl.ptr if want_lse else None, ldl)
    y = wc._features_out(mem, ga, dy, ga.num_rows, w, ldy, what)
    if not want_lse:
        return y, None
    lw = mem.read(ga, dl).reshape(ga.num_rows, ldl)
    assert (lw[:, heads:] == SENTINEL).all(), f"{what}: the pad words of lse were written"
    return y, np.ascontiguousarray(lw[:, :heads]).view(np.float32)


def backward_host(ga, XD, XS, a, gY, lse, heads, slope):
    return ga.backward(XD, XS, a, gY, lse, heads, slope)


def backward_device(mem, ga, XD, XS, a, gY, lse, heads, slope, pad=0, extra=0, what=""):
    """hsgat2_backward_device over fresh buffers: the pads of the inputs NaN, the three outputs pre-filled with a sentinel, the workspace of
    exactly hsgat2_work_bytes bytes pre-filled with NaN and followed by a guard that must survive"""
    w = XS.shape[1]
    (dd, ldd), (ds, lds), (dg, ldg) = (wc._features_in(mem, x, pad) for x in (XD, XS, gY))
    da = _vector_in(mem, a)
    dl, ldl = hc._lse_in(mem, lse, extra)
    ld = w + pad
    od = mem.alloc(np.full((ga.num_rows, ld), SENTINEL, dtype=np.uint32))
    os_ = mem.alloc(np.full((ga.num_cols, ld), SENTINEL, dtype=np.uint32))
    oa = mem.alloc(np.full(w + 4, SENTINEL, dtype=np.uint32))
    nbytes = ga.work_bytes(heads, w // heads)
    assert nbytes % 8 == 0 and w * 8 <= nbytes <= G_MAX * w * 8, nbytes
    work = mem.alloc(np.concatenate([np.full(nbytes // 4, NAN_WORD, dtype=np.uint32), np.full(4, SENTINEL, dtype=np.uint32)]))
    ga.backward_device(dd.ptr, ldd, ds.ptr, lds, da.ptr, dg.ptr, ldg, dl.ptr, ldl, heads, w // heads, slope, od.ptr, ld, os_.ptr, ld, oa.ptr, work.ptr, nbytes)
    aw = mem.read(ga, oa)
    assert (aw[w:] == SENTINEL).all() and (mem.read(ga, work)[nbytes // 4:] == SENTINEL).all(), f"{what}: words behind ga or behind the workspace were written"
    return (wc._features_out(mem, ga, od, ga.num_rows, w, ld, f"{what}, gxd"), wc._features_out(mem, ga, os_, ga.num_cols, w, ld, f"{what}, gxs"),
            np.ascontiguousarray(aw[:w]).view(np.float32).reshape(heads, w // heads))


def all_forward_forms(mem, ga, refs, XD, XS, a, heads, slope, pads, what):
    """the host form and the device form at every pad, each with lse taken and with NULL, inside the bounds of one set of references;
    returns the lse of the host form"""
    y, lse = forward_host(ga, XD, XS, a, heads, slope)
    check_forward(refs, y, lse, f"{what}, host form, lse taken")
    check_forward(refs, forward_host(ga, XD, XS, a, heads, slope, False)[0], None, f"{what}, host form, lse NULL")
    for pad in pads:
        for want in (True, False):
            tag = f"{what}, device form, pad {pad}, {'lse taken' if want else 'lse NULL'}"
            check_forward(refs, *forward_device(mem, ga, XD, XS, a, heads, slope, pad, 3 if pad else 0, want, tag), tag)
    return lse


def all_backward_forms(mem, ga, refs, XD, XS, a, gY, lse, heads, slope, pads, what):
    worst = check_backward(refs, *backward_host(ga, XD, XS, a, gY, lse, heads, slope), f"{what}, host form")
    for pad in pads:
        tag = f"{what}, device form, pad {pad}"
        w = check_backward(refs, *backward_device(mem, ga, XD, XS, a, gY, lse, heads, slope, pad, 3 if pad else 0, tag), tag)
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def general(mem, shapes=SHAPES):
    """300 x 517, 4000 entries, every (heads, d) of SHAPES, slope 0.2, 0 and 1, pad 0 and 8 (lse ld = heads and heads + 3), lse taken and
    NULL, both forms; forward, then backward with the lse the forward just wrote; two backward calls give the same words, ga included"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    for heads, d in shapes:
        with gatv2.GraphAttentionV2((indptr, indices, shape), heads) as ga:
            assert ga.nnz == NNZ
            XD, XS, a, gY = operands(shape, heads, d, 14100 + 1000 * heads + d)
            for slope in SLOPES:
                what = f"general, {heads} heads of d {d}, slope {slope}"
                frefs = forward_refs(indptr, indices, XD, XS, a, heads, slope)
                assert both_signs(frefs)
                lse = all_forward_forms(mem, ga, frefs, XD, XS, a, heads, slope, (0, 8), what)
                w = all_backward_forms(mem, ga, backward_refs(frefs, gY, lse), XD, XS, a, gY, lse, heads, slope, (0, 8), what)
                print(f"{what}: backward worst error / bound = {w['gxd']:.3f} (gxd), {w['gxs']:.3f} (gxs), {w['ga']:.3f} (ga)")
            first = backward_device(mem, ga, XD, XS, a, gY, lse, heads, SLOPES[-1], 4)
            assert same_words(first, backward_device(mem, ga, XD, XS, a, gY, lse, heads, SLOPES[-1], 4)), f"{heads} heads of d {d}: two backward calls differ"
            assert same_words(first, backward_host(ga, XD, XS, a, gY, lse, heads, SLOPES[-1])), f"{heads} heads of d {d}: the two forms differ"


def ties(mem, heads=3, d=8):
    """XD and XS on the 1/8 grid, so that z == 0 occurs (the slope branch of w and of dz): slope 0.25 and 0"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    shape = (ROWS, COLS)
    rng = np.random.default_rng(14300)
    XD, XS = ((rng.integers(-12, 13, (n, heads * d)) / 8.0).astype(np.float32) for n in shape)
    a = wc.grid_values(rng, (heads, d)) / np.float32(4.0)
    gY = rng.normal(0.0, 1.0, (ROWS, heads * d)).astype(np.float32)
    with gatv2.GraphAttentionV2((indptr, indices, shape), heads) as ga:
        for slope in (0.25, 0.0):
            what = f"ties, slope {slope}"
            frefs = forward_refs(indptr, indices, XD, XS, a, heads, slope)
            z = np.concatenate([f.scores.z for f in frefs], axis=1)
            assert (z == 0).mean() >= 0.01 and (z < 0).mean() >= 0.2, ((z == 0).mean(), (z < 0).mean())
            lse = all_forward_forms(mem, ga, frefs, XD, XS, a, heads, slope, (4,), what)
            all_backward_forms(mem, ga, backward_refs(frefs, gY, lse), XD, XS, a, gY, lse, heads, slope, (4,), what)


def heads_do_not_leak(mem, shapes=((4, 16), (5, 4))):
    """A NaN in one head of XD, XS, a and lse in turn; the other heads stay inside the bounds of the CLEAN references.
    Forward: head 1's first word of XD is NaN in some rows (those rows' head 1 is NaN in Y and lse), head 1's first word of XS in some
    columns (every row that holds one is NaN in head 1), then a[1][0] (all of head 1).  Head 1 follows its own reference, built from the
    planted operands.  Backward, from clean operands: head 1's lse word of some rows is NaN, of others -inf: head 1 is NaN in gXD of those
    rows, in gXS of the columns they touch and in all of ga[1]; then a NaN in a[1][0]: all of head 1's words of the three outputs are NaN
    wherever an entry reaches, and +0.0 where none does."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    n = np.diff(indptr.astype(np.int64))
    m = np.bincount(indices, minlength=COLS)
    r_nan, c_nan = np.array([4, 100, 250]), np.array([5, 90, 333, 500])
    b_nan, b_inf = (np.nonzero(n >= 3)[0][[2, 40]], np.nonzero(n >= 3)[0][[7, 90]])
    slope = 0.2
    for heads, d in shapes:
        h1 = slice(d, 2 * d)
        others = np.r_[0:d, 2 * d: heads * d]
        with gatv2.GraphAttentionV2((indptr, indices, shape), heads) as ga:
            XD, XS, a, gY = operands(shape, heads, d, 14500 + 1000 * heads + d)
            clean = forward_refs(indptr, indices, XD, XS, a, heads, slope)
            for name in ("xd", "xs", "a"):
                XDp, XSp, ap = XD.copy(), XS.copy(), a.copy()
                if name == "xd":
                    XDp[r_nan, d] = np.nan
                elif name == "xs":
                    XSp[c_nan, d] = np.nan
                else:
                    ap[1, 0] = np.nan
                planted = forward_refs(indptr, indices, XDp, XSp, ap, heads, slope)
                assert planted[1].bad.sum() >= 3 and (name == "a" or planted[1].finite.sum() > ROWS // 2)
                refs = [planted[h] if h == 1 else clean[h] for h in range(heads)]
                what = f"heads do not leak, forward, NaN in {name}, {heads} heads of d {d}"
                for y, lse in (forward_host(ga, XDp, XSp, ap, heads, slope), forward_device(mem, ga, XDp, XSp, ap, heads, slope, 4, 1, True, what)):
                    check_forward(refs, y, lse, what)
                    assert np.isfinite(y[:, others][n > 0]).all() and np.isfinite(np.delete(lse, 1, axis=1)[n > 0]).all(), f"{what}: head 1's NaN reached another head"
            # backward: lse
            lse = rounded_forward(clean)[1]
            lse[b_nan, 1], lse[b_inf, 1] = np.nan, -np.inf
            brefs = backward_refs(clean, gY, lse)
            assert brefs[1].bad_r.sum() == 4 and 4 <= brefs[1].bad_c.sum() < COLS // 4 and not any(r.bad_r.any() for h, r in enumerate(brefs) if h != 1)
            what = f"heads do not leak, backward, NaN in lse, {heads} heads of d {d}"
            for g in (backward_host(ga, XD, XS, a, gY, lse, heads, slope), backward_device(mem, ga, XD, XS, a, gY, lse, heads, slope, 4, 1, what)):
                check_backward(brefs, *g, what)
                assert np.isnan(g[2][1]).all() and np.isfinite(np.delete(g[2], 1, axis=0)).all(), f"{what}: ga"
                assert np.isfinite(g[0][:, others]).all() and np.isfinite(g[1][:, others]).all(), f"{what}: head 1's lse words reached another head"
            # backward: a
            lse = rounded_forward(clean)[1]
            brefs = backward_refs(clean, gY, lse)
            ap = a.copy()
            ap[1, 0] = np.nan
            what = f"heads do not leak, backward, NaN in a, {heads} heads of d {d}"
            for g in (backward_host(ga, XD, XS, ap, gY, lse, heads, slope), backward_device(mem, ga, XD, XS, ap, gY, lse, heads, slope, 4, 1, what)):
                assert np.isnan(g[0][:, h1][n > 0]).all() and np.isnan(g[1][:, h1][m > 0]).all() and np.isnan(g[2][1]).all(), f"{what}: head 1 is not NaN throughout"
                assert not words(g[0][:, h1][n == 0]).any() and not words(g[1][:, h1][m == 0]).any(), f"{what}: a row or column without entries is not +0.0"
                rest, good = [x.copy() for x in g], rounded_backward(brefs)      # head 1 is checked above; the other heads against the clean references
                rest[0][:, h1], rest[1][:, h1], rest[2][1] = good[0][:, h1], good[1][:, h1], good[2][1]
                check_backward(brefs, *rest, what)


def edges(mem, heads=3, d=8):
    """every pattern of pattern_cases.edge_patterns() at (3, 8): nnz = 0 ... 7, one row, one column, runs of empty rows, empty columns, one
    row that holds all 301 entries, unsorted columns, a pair held twice; rows and columns without entries read +0.0 (and -inf in lse) bit
    for bit, and ga is all +0.0 at nnz = 0"""
    seen_empty = False
    more = [("one row", 1, 9, np.array([0, 5], dtype=np.uint32), np.array([0, 2, 3, 7, 8], dtype=np.uint32)),
            ("one column", 7, 1, np.array([0, 1, 1, 2, 3, 3, 3, 4], dtype=np.uint32), np.zeros(4, dtype=np.uint32))]
    for name, rows, cols, indptr, indices in edge_patterns() + more:
        shape = (rows, cols)
        with gatv2.GraphAttentionV2((indptr, indices, shape), heads) as ga:
            assert ga.nnz == indices.size
            XD, XS, a, gY = operands(shape, heads, d, 14700)
            frefs = forward_refs(indptr, indices, XD, XS, a, heads, 0.2)
            assert all(r.empty.sum() == (np.diff(indptr.astype(np.int64)) == 0).sum() for r in frefs)
            lse = all_forward_forms(mem, ga, frefs, XD, XS, a, heads, 0.2, (8,), name)
            assert (lse[frefs[0].empty] == -np.inf).all()
            all_backward_forms(mem, ga, backward_refs(frefs, gY, lse), XD, XS, a, gY, lse, heads, 0.2, (8,), name)
            if indices.size == 0:
                seen_empty = True
                for g in (backward_host(ga, XD, XS, a, gY, lse, heads, 0.2), backward_device(mem, ga, XD, XS, a, gY, lse, heads, 0.2, 8, 1, name)):
                    assert not words(g[2]).any() and not words(g[0]).any() and not words(g[1]).any(), f"{name}: not +0.0 throughout at nnz = 0"
    assert seen_empty


def plain_backward_device(mem, ga, Q, K, V, gY, lse, heads, scale):
    """hsmh_backward_device of the same object (through the base class): it overwrites the D words"""
    w = Q.shape[1]
    (dq, ldq), (dk, ldk), (dv, ldv), (dg, ldg) = (wc._features_in(mem, x, 0) for x in (Q, K, V, gY))
    dl, ldl = hc._lse_in(mem, lse, 0)
    oq = mem.alloc(np.full((ga.num_rows, w), SENTINEL, dtype=np.uint32))
    ok, ov = (mem.alloc(np.full((ga.num_cols, w), SENTINEL, dtype=np.uint32)) for _ in range(2))
    mha.MultiHeadAttention.backward_device(ga, dq.ptr, ldq, dk.ptr, ldk, dv.ptr, ldv, dg.ptr, ldg, dl.ptr, ldl, heads, w // heads, scale, oq.ptr, w, ok.ptr, w, ov.ptr, w)
    return tuple(wc._features_out(mem, ga, buf, n_, w, w, name) for name, buf, n_ in (("gq", oq, ga.num_rows), ("gk", ok, ga.num_cols), ("gv", ov, ga.num_cols)))


def nothing_carried_over(mem):
    """on one object: hsgat2 at (4, 64), then hsmh_backward_device at (5, 4), which overwrites the D words, then hsgat2 at (4, 64) again
    gives the bits of the first time, which are the words of a fresh object; the dot-product call in between is inside its own bounds"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with gatv2.GraphAttentionV2((indptr, indices, shape), 8) as ga, gatv2.GraphAttentionV2((indptr, indices, shape), 4) as fresh:
        XD, XS, a, gY = operands(shape, 4, 64, 14800)
        f1 = forward_device(mem, ga, XD, XS, a, 4, 0.2)
        b1 = backward_device(mem, ga, XD, XS, a, gY, f1[1], 4, 0.2)
        frefs = forward_refs(indptr, indices, XD, XS, a, 4, 0.2)
        check_forward(frefs, *f1, "first call")
        check_backward(backward_refs(frefs, gY, f1[1]), *b1, "first call")
        Q2, K2, V2, gY2 = hc.operands(shape, 20, 14810)
        scores = hc.head_scores(indptr, indices, Q2, K2, 5)
        lse2 = hc.rounded_forward(hc.forward_refs(scores, V2, -0.75))[1]
        hc.check_backward(hc.backward_refs(scores, V2, gY2, lse2, -0.75), *plain_backward_device(mem, ga, Q2, K2, V2, gY2, lse2, 5, -0.75), "the dot-product call in between")
        assert same_words(f1, forward_device(mem, ga, XD, XS, a, 4, 0.2)) and same_words(f1, forward_host(ga, XD, XS, a, 4, 0.2))
        assert same_words(b1, backward_device(mem, ga, XD, XS, a, gY, f1[1], 4, 0.2)) and same_words(b1, backward_host(ga, XD, XS, a, gY, f1[1], 4, 0.2))
        assert same_words(f1, forward_device(mem, fresh, XD, XS, a, 4, 0.2)) and same_words(b1, backward_device(mem, fresh, XD, XS, a, gY, f1[1], 4, 0.2))


def large(mem, shape, indptr, indices, heads, d, seed, what, slope=0.2):
    """the device forms over one large pattern, forward then backward with the lse just written, every word of every head inside its bound
    (float64 sums in the references), and a second backward call with the same words; returns the two lists of references"""
    XD, XS, a, gY = operands(shape, heads, d, seed)
    fwd = forward_refs(indptr, indices, XD, XS, a, heads, slope, exact=False)
    with gatv2.GraphAttentionV2((indptr, indices, shape), heads) as ga:
        y, lse = forward_device(mem, ga, XD, XS, a, heads, slope, 4, 1, True, what)
        check_forward(fwd, y, lse, what)
        bwd = backward_refs(fwd, gY, lse)
        g = backward_device(mem, ga, XD, XS, a, gY, lse, heads, slope, 4, 1, what)
        check_backward(bwd, *g, what)
        assert same_words(g, backward_device(mem, ga, XD, XS, a, gY, lse, heads, slope, 0, 0, what)), f"{what}: two backward calls differ"
    return fwd, bwd


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
FEATURES = ("xd", "xs", "gy", "gxd", "gxs")


def refusals(mem):
    l = gatv2.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    one = np.zeros(64, dtype=np.float32).ctypes.data
    nbytes = C.c_uint64(0)
    # a null object
    assert l.hsgat2_forward_device(None, vp(one), 4, vp(one), 4, vp(one), 1, 4, 0.2, vp(one), 4, None, 1) == BAD_ARG
    assert l.hsgat2_forward(None, vp(one), vp(one), vp(one), 1, 4, 0.2, vp(one), None) == BAD_ARG
    assert l.hsgat2_backward_device(None, vp(one), 4, vp(one), 4, vp(one), vp(one), 4, vp(one), 1, 1, 4, 0.2, vp(one), 4, vp(one), 4, vp(one), vp(one), 64) == BAD_ARG
    assert l.hsgat2_backward(None, vp(one), vp(one), vp(one), vp(one), vp(one), 1, 4, 0.2, vp(one), vp(one), vp(one)) == BAD_ARG
    assert l.hsgat2_work_bytes(None, 1, 4, C.byref(nbytes)) == BAD_ARG

    heads, d = 2, 4
    with gatv2.GraphAttentionV2((indptr, indices, shape), 4) as ga, gatv2.GraphAttentionV2((indptr, indices, shape), 4, backward=False) as fwd_only:
        XD, XS, a, gY = operands(shape, heads, d, 14900)
        want_y, want_l = forward_host(ga, XD, XS, a, heads, 0.5)
        frefs = forward_refs(indptr, indices, XD, XS, a, heads, 0.5)
        check_forward(frefs, want_y, want_l, "refusals")
        want_g = backward_host(ga, XD, XS, a, gY, want_l, heads, 0.5)
        check_backward(backward_refs(frefs, gY, want_l), *want_g, "refusals")

        def still_usable(rc, what, obj=ga):
            assert rc == BAD_ARG and l.hsmh_last_error(obj._h), (what, rc)
            assert same_words(forward_host(obj, XD, XS, a, heads, 0.5), (want_y, want_l)), f"unusable after {what}"
            if obj is ga:
                assert same_words(backward_host(ga, XD, XS, a, gY, want_l, heads, 0.5), want_g), f"unusable after {what}"

        def forward_call(k, obj=ga):
            return l.hsgat2_forward_device(obj._h, vp(k["xd"]), k["ldxd"], vp(k["xs"]), k["ldxs"], vp(k["a"]), k["heads"], k["d"], k["slope"], vp(k["y"]), k["ldy"], vp(k["lse"]), k["ldlse"])

        def backward_call(k, obj=ga):
            return l.hsgat2_backward_device(obj._h, vp(k["xd"]), k["ldxd"], vp(k["xs"]), k["ldxs"], vp(k["a"]), vp(k["gy"]), k["ldgy"], vp(k["lse"]), k["ldlse"], k["heads"], k["d"],
                                            k["slope"], vp(k["gxd"]), k["ldgxd"], vp(k["gxs"]), k["ldgxs"], vp(k["ga"]), vp(k["work"]), k["work_bytes"])

        # the workspace's size: refused for a shape the calls refuse, the same for both objects, a whole number of vectors of heads * d doubles
        assert l.hsgat2_work_bytes(ga._h, heads, d, None) == BAD_ARG
        for bad in ((0, 4), (5, 4), (1, 5), (1, 2), (4, 128), (2, 256)):
            assert l.hsgat2_work_bytes(ga._h, bad[0], bad[1], C.byref(nbytes)) == BAD_ARG, bad
        need = ga.work_bytes(heads, d)
        assert need == fwd_only.work_bytes(heads, d) and need % (heads * d * 8) == 0 and 0 < need <= G_MAX * heads * d * 8
        # features: 9 rows x 16 words (ld up to 16), 16-byte aligned; a and ga: 16 words; lse: 9 rows of up to 4 words
        names = FEATURES + ("y", "a", "ga", "lse")
        bufs = {name: mem.alloc(np.zeros(9 * 16, np.uint32)) for name in names}
        bufs["work"] = mem.alloc(np.zeros(need // 4 + 64, np.uint32))
        ok = {name: b.ptr for name, b in bufs.items()}
        ok.update({"ld" + name: 8 for name in FEATURES + ("y",)}, ldlse=2, heads=heads, d=d, slope=0.2, work_bytes=need)
        assert forward_call(ok) == 0 and backward_call(ok) == 0
        xd, xs, av, gy, y, ls, gxd, gxs, gav, work = (ok[k] for k in ("xd", "xs", "a", "gy", "y", "lse", "gxd", "gxs", "ga", "work"))
        nan, inf = float("nan"), float("inf")
        wide_ld = lambda names_, ld: {"ld" + k: ld for k in names_}      # noqa: E731
        # slope, SHAPES ACCEPTED (the object's max_heads is 4), the inputs both calls share
        shared = [("slope NaN", dict(slope=nan)), ("slope inf", dict(slope=inf)), ("slope -inf", dict(slope=-inf)), ("slope -0.5", dict(slope=-0.5)),
                  ("slope -2^-149", dict(slope=-1.4e-45)), ("d = 0", dict(d=0)), ("d = 1", dict(d=1)), ("d = 2", dict(d=2)), ("d = 3", dict(d=3)), ("d = 5", dict(heads=1, d=5)),
                  ("d = 12", dict(heads=1, d=12)), ("d = 24", dict(heads=1, d=24)), ("d = 512", dict(heads=1, d=512)), ("d = 2^31", dict(heads=1, d=2 ** 31)),
                  ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5, d=4)), ("heads * d = 512", dict(heads=4, d=128)),
                  ("heads * d = 512 at d = 256", dict(heads=2, d=256)), ("null xd", dict(xd=None)), ("null xs", dict(xs=None)), ("null a", dict(a=None)),
                  ("misaligned xd", dict(xd=xd + 4)), ("misaligned xs by 8", dict(xs=xs + 8)), ("misaligned a", dict(a=av + 4)), ("misaligned lse", dict(lse=ls + 2)),
                  ("ldxd % 4", dict(ldxd=10)), ("ldxd < heads * d", dict(ldxd=4)), ("ldxs % 4", dict(ldxs=10)), ("ldxs < heads * d", dict(ldxs=4)), ("ldxs = 0", dict(ldxs=0)),
                  ("ldl < heads", dict(ldlse=1)), ("ldl = 0", dict(ldlse=0))]
        for what, change in shared:
            if "heads * d" in what or "d = 512" in what or "2^31" in what:
                change = dict(wide_ld(FEATURES + ("y",), 512), **change)
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        fcases = [("null y", dict(y=None)), ("misaligned y", dict(y=y + 4)), ("ldy % 4", dict(ldy=10)), ("ldy < heads * d", dict(ldy=4)), ("y is xs", dict(y=xs)),
                  ("y is xd", dict(y=xd)), ("y is a", dict(y=av)), ("y over the last word of a", dict(y=av + 16)), ("lse inside y", dict(lse=y + 4 * 4)), ("lse is a", dict(lse=av)),
                  ("lse inside xs", dict(lse=xs + 8)), ("y's last row in xs", dict(xs=gy + 16, y=gy + 16 + 8 * 8 * 4))]
        for what, change in fcases:
            still_usable(forward_call(dict(ok, **change)), "forward_device: " + what)
        bcases = [("null lse", dict(lse=None)), ("null gy", dict(gy=None)), ("misaligned gy", dict(gy=gy + 4)), ("ldgy % 4", dict(ldgy=10)), ("ldgy < heads * d", dict(ldgy=4)),
                  ("null gxd", dict(gxd=None)), ("null gxs", dict(gxs=None)), ("null ga", dict(ga=None)), ("misaligned gxd", dict(gxd=gxd + 8)), ("misaligned gxs", dict(gxs=gxs + 4)),
                  ("misaligned ga", dict(ga=gav + 4)), ("ldgxd % 4", dict(ldgxd=10)), ("ldgxd < heads * d", dict(ldgxd=4)), ("ldgxs % 4", dict(ldgxs=10)),
                  ("ldgxs < heads * d", dict(ldgxs=4)), ("gxd is xd", dict(gxd=xd)), ("gxs is xs", dict(gxs=xs)), ("ga is a", dict(ga=av)), ("gxs is gy", dict(gxs=gy)),
                  ("gxd is gxs", dict(gxd=gxs)), ("ga inside gxd", dict(ga=gxd + 16)), ("ga inside lse", dict(ga=ls)), ("ga over the last word of a", dict(ga=av + 16)),
                  ("gxd's last row in xd", dict(xd=gy + 16, gxd=gy + 16 + 5 * 8 * 4)),
                  # the workspace: null, too small by a byte and by a vector, zero, misaligned, over an input, over each output, an output inside it
                  ("null workspace", dict(work=None)), ("workspace one byte short", dict(work_bytes=need - 1)), ("workspace a vector short", dict(work_bytes=need - heads * d * 8)),
                  ("workspace of no bytes", dict(work_bytes=0)), ("misaligned workspace", dict(work=work + 8)), ("misaligned workspace by 4", dict(work=work + 4)),
                  ("workspace is xs", dict(work=xs)), ("workspace is a", dict(work=av)), ("workspace is gxd", dict(work=gxd)), ("workspace is gxs", dict(work=gxs)),
                  ("workspace is ga", dict(work=gav)), ("ga inside the workspace", dict(ga=work + 16)), ("lse inside the workspace", dict(lse=work + 32)),
                  ("the workspace's last bytes in gy", dict(gy=work + need - 16))]
        for what, change in bcases:
            still_usable(backward_call(dict(ok, **change)), "backward_device: " + what)
        # a workspace laid over an output whatever its size: the output at the workspace's first and last bytes
        still_usable(backward_call(dict(ok, ga=work)), "backward_device: ga at the workspace's first byte")
        still_usable(backward_call(dict(ok, ga=work + need - 16)), "backward_device: ga over the workspace's last bytes")
        assert backward_call(dict(ok, work_bytes=need - 1)) == BAD_ARG and b"hsgat2_work_bytes" in l.hsmh_last_error(ga._h)
        # the host forms
        host = {name: np.zeros(9 * 8, np.float32) for name in names}
        okh = dict({name: x.ctypes.data for name, x in host.items()}, heads=heads, d=d, slope=0.2)

        def forward_host_call(k, obj=ga):
            return l.hsgat2_forward(obj._h, vp(k["xd"]), vp(k["xs"]), vp(k["a"]), k["heads"], k["d"], k["slope"], vp(k["y"]), vp(k["lse"]))

        def backward_host_call(k, obj=ga):
            return l.hsgat2_backward(obj._h, vp(k["xd"]), vp(k["xs"]), vp(k["a"]), vp(k["gy"]), vp(k["lse"]), k["heads"], k["d"], k["slope"], vp(k["gxd"]), vp(k["gxs"]), vp(k["ga"]))

        assert forward_host_call(okh) == 0 and backward_host_call(okh) == 0
        both = [("d = 0", dict(d=0)), ("d = 6", dict(d=6)), ("heads = 0", dict(heads=0)), ("heads > max_heads", dict(heads=5)), ("heads * d = 512", dict(heads=4, d=128)),
                ("slope NaN", dict(slope=nan)), ("slope inf", dict(slope=inf)), ("slope -1", dict(slope=-1.0))]
        for what, change in both + [(f"null {k}", {k: None}) for k in ("xd", "xs", "a", "y")] + [("y is xs", dict(y=okh["xs"])), ("lse inside y", dict(lse=okh["y"] + 8)),
                                                                                                  ("lse is a", dict(lse=okh["a"]))]:
            still_usable(forward_host_call(dict(okh, **change)), "forward: " + what)
        for what, change in both + [(f"null {k}", {k: None}) for k in FEATURES + ("a", "ga", "lse")] + [("gxd is xd", dict(gxd=okh["xd"])), ("gxs is gxd", dict(gxs=okh["gxd"])),
                                                                                                       ("ga inside lse", dict(ga=okh["lse"] + 8)), ("ga is a", dict(ga=okh["a"]))]:
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
        # fine: slope -0.0 and 0; ranges that touch without sharing a byte (lse right behind y's 6 rows, ga right behind a's 8 words, the workspace right behind ga,
        # a larger workspace); a NULL lse
        assert forward_call(dict(ok, slope=-0.0)) == 0 and backward_call(dict(ok, slope=-0.0)) == 0 and forward_call(dict(ok, slope=0.0)) == 0
        assert forward_call(dict(ok, lse=y + (5 * 8 + 8) * 4)) == 0
        assert forward_call(dict(ok, lse=None, ldlse=0)) == 0
        assert backward_call(dict(ok, ga=av + 8 * 4)) == 0
        assert backward_call(dict(ok, ga=work + need, work_bytes=need)) == 0
        assert backward_call(dict(ok, work_bytes=need + 64)) == 0
        for obj in (ga, fwd_only):
            obj.set_stream(None)
            obj.sync()
