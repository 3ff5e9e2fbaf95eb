"""The float contract of the kernels, as a float64 reference with a rounding bound per path (test helper, like cases.py).

The reference is built from the STORED elements of the matrix as formatted (an explicit zero is an element): per element the fp32
product p_e = fl32(a_e * x_e) (numpy float32: exact in float64), per row E = math.fsum(p_e) (the exactly rounded sum), A = sum |p_e| and
n = the number of stored elements.  u = 2^-24.  gamma(k) = k u / (1 - k u) bounds k fp32 roundings in a chain (Higham, Thm 3.1).

Rounding classes -- L = the longest chain of fp32 additions a product passes through before it joins a double sum:
  D   L = 1: every product joins a double sum as it is (hisparse_amd/csrc/spmv_device.h, Rows<true>::add / add_sum: ds_add_f64 of the fp32
      product; spmv_kernels.hip consume_step PAIRS dense rows: the wavefront's register sum is a double (Rows::sum_t), spmv_light_kernel:
      double lane sums; spmv_sweep.hip / spmm_sweep.hip FloatAcc: ds_add_f64; spmspv.hip accumulate: R::add of the fp32 product).
  DL  DELTA with per-lane register sums (spmv_kernels.hip consume_step, kDelta && kDense): Rows<true>::lane_t = float, a lane sums its
      consecutive slots of ONE row in fp32 and hands the sum over when the row or the unit (a sub-tile of at most 8192 columns) changes.
      A lane's run in a unit is run_len slots (stream_tiles.cpp: the unit's ceil(slots / 64) chunks dealt over 14 wavefronts), which the
      image shows as 2 x records - 1 per (unit, wavefront) (a head slot, then two slots per record): L = min(the row's elements inside
      8192 columns, the image's longest run) (dl_chain, delta_lane_cap).
  B8  BITMAP (spmv_bitmap.hip consume, spmm_bitmap.hip): the 8 products of a batch are added in fp32 -- two interleaved chains of four
      (v_pk_add_f32) and one add of the two, depth 4; the plain loop of odd batches is a chain of 8 -- then joins the double sum: L = 8.
  F   OWNER / OWNER24 float (spmv_kernels.hip OwnerOps<true>: fp32 lane sums flushed into fp32 LDS accumulators): the whole row is one fp32
      running sum, L = n.  Matrix engine (spmm_mfma.hip): fp32 FMAs over the row tile's elements of one column chunk, the chunk tiles summed
      in double by spmm_mfma_reduce_kernel, with the UNROUNDED products a x (an FMA does not round the product): the chain starts from a
      zero accumulator, so the first FMA already rounds and n products take n roundings, L = n + 1.
A sum over S column slices (combine_slices_kernel, carried_combine) or S passes of hs_spmspv (kAdd) rounds every partial once and adds
the S partials in fp32 from the first: S more roundings of at most A each.

  one slice:  |y - E| <= u |E| + (1 + u) gamma(L - 1) A + n 2^-52 A + L 2^-149
  S slices:   |y - E| <= gamma(L - 1 + S) A + n 2^-52 A + (L + S) 2^-149
(n 2^-52 A covers the double sums in any order, 2^-149 per fp32 rounding the subnormal range, where the error is absolute.)

Non-finite rows follow IEEE float64 summation of the p_e: NaN if any product is NaN or both +inf and -inf occur, +-inf if one infinity
occurs; a finite E whose bound reaches past the fp32 range may round to the infinity of its sign.
"""
import math

import numpy as np

U = 2.0 ** -24
F32_OVERFLOW = float(np.float32(np.finfo(np.float32).max)) * (1.0 + 2.0 ** -25)     # |s| >= this rounds to inf in fp32
WINDOW = 8192                                          # columns of a sub-tile / unit (stream_tiles.h kSubTileCols)


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


class Reference:
    """Per-row float64 facts of y = A x for a scipy CSR matrix `m` (float32 data, stored elements as formatted) and a float32 x.
    num_rows >= m.shape[0]: the padded rows beyond the matrix have no element (E = 0, n = 0).  exact_products: the matrix engine's
    unrounded products a * x instead of fl32(a * x)."""

    def __init__(self, m, x, num_rows=None, exact_products=False):
        m = m.tocsr()
        rows = m.shape[0]
        self.num_rows = num_rows = rows if num_rows is None else num_rows
        x = np.asarray(x, dtype=np.float32)
        ip, ix = m.indptr.astype(np.int64), m.indices.astype(np.int64)
        a = np.asarray(m.data, dtype=np.float32)
        with np.errstate(all="ignore"):
            p = a.astype(np.float64) * x[ix].astype(np.float64) if exact_products else (a * x[ix]).astype(np.float64)
        self.E = np.zeros(num_rows)
        self.A = np.zeros(num_rows)
        self.n = np.zeros(num_rows, dtype=np.int64)
        self.nan = np.zeros(num_rows, dtype=bool)
        self.inf = np.zeros(num_rows)                  # +1 / -1: the row's sum is that infinity
        self.min_abs = np.full(num_rows, np.inf)       # smallest |p_e| of the row (a dropped or doubled product moves y by at least this)
        self.products = []
        for r in range(rows):
            pr = p[ip[r]: ip[r + 1]]
            self.products.append(pr)
            self.n[r] = pr.size
            if not pr.size:
                continue
            if np.isnan(pr).any() or (np.isposinf(pr).any() and np.isneginf(pr).any()):
                self.nan[r] = True
            elif np.isinf(pr).any():
                self.inf[r] = 1.0 if np.isposinf(pr).any() else -1.0
            else:
                self.E[r] = math.fsum(pr)
                self.A[r] = float(np.abs(pr).sum())
                self.min_abs[r] = float(np.abs(pr).min())
        self.finite = ~self.nan & (self.inf == 0)

    def bound(self, L=1, slices=1):
        """|y - E| allowed per row for chains of L fp32 additions (scalar or per row) and `slices` partials added in fp32."""
        L = np.asarray(L, dtype=np.float64)
        if L.ndim and L.size < self.num_rows:          # per-row chains of the matrix's rows: the padded rows have none
            L = np.pad(L, (0, self.num_rows - L.size), constant_values=1.0)
        L = np.broadcast_to(L, self.E.shape)
        dbl = self.n * 2.0 ** -52 * self.A
        if slices <= 1:
            return U * np.abs(self.E) + (1.0 + U) * gamma(np.maximum(L - 1, 0)) * self.A + dbl + L * 2.0 ** -149
        return gamma(np.maximum(L - 1, 0) + slices) * self.A + dbl + (L + slices) * 2.0 ** -149

    def violations(self, y_words, L=1, slices=1):
        """Boolean per row: y (packed fp32 words) breaks the contract."""
        y = np.asarray(y_words, dtype=np.uint32)[: self.num_rows].view(np.float32).astype(np.float64)
        assert y.size == self.num_rows
        b = self.bound(L, slices)
        bad = np.zeros(self.num_rows, dtype=bool)
        bad |= self.nan & ~np.isnan(y)
        inf = self.inf != 0
        bad |= inf & (y != np.where(self.inf > 0, np.inf, -np.inf))
        f = self.finite
        with np.errstate(invalid="ignore"):
            err = np.abs(y - self.E)
            may_overflow = np.abs(self.E) + b >= F32_OVERFLOW
            ok_inf = np.isinf(y) & may_overflow & (np.sign(y) == np.sign(self.E))
            bad |= f & ~ok_inf & ~(np.isfinite(y) & (err <= b))
        return bad

    def check(self, y_words, L=1, slices=1, what=""):
        bad = self.violations(y_words, L, slices)
        if bad.any():
            y = np.asarray(y_words, dtype=np.uint32)[: self.num_rows].view(np.float32)
            r = np.nonzero(bad)[0][:6]
            detail = ", ".join(f"row {i}: y={float(y[i])!r} E={self.E[i]!r} bound={float(np.atleast_1d(self.bound(L, slices))[i]):.3g} "
                               f"n={int(self.n[i])}" for i in r)
            raise AssertionError(f"{what}: {int(bad.sum())} rows break the float contract (L={np.max(L)}, slices={slices}): {detail}")


def dl_chain(m):
    """DL: per row, the most elements inside any 8192 consecutive columns -- an upper bound of a DELTA lane's fp32 run on the row
    inside one unit (a unit is one sub-tile of at most 8192 columns; the lane's slots are consecutive elements of the unit)."""
    m = m.tocsr()
    L = np.ones(m.shape[0], dtype=np.int64)
    for r in range(m.shape[0]):
        c = np.sort(m.indices[m.indptr[r]: m.indptr[r + 1]].astype(np.int64))
        if c.size:
            L[r] = int((np.searchsorted(c, c + WINDOW) - np.arange(c.size)).max())
    return L


def delta_lane_cap(tiles):
    """The longest run of slots a DELTA lane walks inside one unit: 2 x records - 1 over every (unit, wavefront) of the image
    (hs_debug_read_tiles / build_tiles; Unit.end_step[w] counts records from the block's start)."""
    cap = 1
    blocks, units = tiles["blocks"], tiles["units"]
    for blk in blocks:
        prev = np.zeros(units["end_step"].shape[1], dtype=np.int64)
        for u in range(int(blk["unit_begin"]), int(blk["unit_end"])):
            end = units[u]["end_step"].astype(np.int64)
            cap = max(cap, int((2 * (end - prev) - 1).max()))
            prev = end
    return cap


def chain(variant, m, tiles=None):
    """L of a forced stream-format variant (test_gpu_parity's names) for SpMV in the float modes; tiles: the loaded image, whose DELTA
    runs cap a lane's chain."""
    fmt = variant.split("-")[0]
    if variant in ("delta", "delta-lane-sums"):          # "delta": the block's density decides whether lanes sum in registers
        L = dl_chain(m)
        return L if tiles is None else np.minimum(L, delta_lane_cap(tiles))
    if fmt == "bitmap":
        return 8
    if fmt in ("owner", "owner24"):
        return np.maximum(np.diff(m.tocsr().indptr), 1)
    return 1                                             # pairs, pairs24, light, sweep, delta-no-lane-sums


def magnitudes(rng, n):
    """+-2^U(-6,6) * (1 + U): nothing near zero, twelve binades of range."""
    return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-6, 6, n) * (1.0 + rng.uniform(0, 1, n))).astype(np.float32)


def designed(rows, cols, seed, hubs=2, hub_len=None):
    """(scipy CSR, x, dict of row sets): rows of length 1, 2, 7, 8, 9, 63, 64, 65, 300 and empty ones in turn, a cancellation family of
    +v, -v (1 + d) pairs (|E| << A, 64 or 300 elements), and `hubs` rows over all the columns (several 8192-column sub-tiles)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    x = magnitudes(rng, cols)
    lengths = [1, 2, 7, 8, 9, 63, 64, 65, 300, 0]
    indptr, indices, data = [0], [], []
    kinds = {"long": [], "cancel": [], "hub": [], "empty": []}
    hub_len = hub_len or min(cols, 3 * cols // 4)
    for r in range(rows):
        if r < hubs:
            n, kind = hub_len, "hub"
        elif r % 11 == 10:
            n, kind = (64 if r % 2 else 300), "cancel"
        else:
            n = min(lengths[r % len(lengths)], cols)
            kind = "empty" if n == 0 else ("long" if n >= 63 else None)
        c = np.sort(rng.choice(cols, n, replace=False)).astype(np.int64)
        v = magnitudes(rng, n)
        if kind == "cancel" and n >= 2:
            # pair (2k, 2k+1): a_{2k+1} x_{c2k+1} = -a_{2k} x_{c2k} (1 + d), d ~ 2^-12: the products cancel to a few bits
            d = 2.0 ** rng.uniform(-14, -10, n // 2)
            p0 = v[0::2][: n // 2].astype(np.float64) * x[c[0::2][: n // 2]]
            v[1::2][: n // 2] = (-p0 * (1.0 + d) / x[c[1::2][: n // 2]]).astype(np.float32)
        if kind:
            kinds[kind].append(r)
        indices.extend(c.tolist())
        data.extend(v.tolist())
        indptr.append(len(indices))
    m = sp.csr_matrix((np.array(data, dtype=np.float32), np.array(indices, dtype=np.int64), np.array(indptr, dtype=np.int64)), shape=(rows, cols))
    return m, x, {k: np.array(v, dtype=np.int64) for k, v in kinds.items()}
