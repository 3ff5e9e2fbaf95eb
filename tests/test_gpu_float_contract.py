"""The float contract on the GPU (tests/float_contract.py): every float path against the float64 sum of its fp32 products, within the
rounding bound of its class -- not within csim's 1e-4 -- at designed inputs (twelve binades, rows of 1 ... 300 elements, cancelling
pairs, hub rows over several sub-tiles), every forced stream format, column slices 1 / 3 / 12, and every entry point; IEEE edges."""
import numpy as np
import pytest
import scipy.sparse as sp

from hisparse_amd import device, host
from oracle import oracle as orc

import cases
import float_contract as fc
from test_gpu_parity import _assert_forced_plan
from test_spmm import _Hip

pytestmark = pytest.mark.gpu

VARIANTS = ["pairs", "delta", "delta-lane-sums", "delta-no-lane-sums", "bitmap", "owner", "pairs24", "owner24", "light", "sweep"]
D_VARIANTS = ["pairs", "pairs24", "light", "sweep", "delta-no-lane-sums"]


def _force(monkeypatch, variant, slices=1):
    # the parity fixture's ten variants (test_gpu_parity.stream_format)
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "pairs" if variant in ("pairs24", "light") else variant.split("-")[0])
    monkeypatch.setenv("HISPARSE_LIGHT", "1" if variant == "light" else "0")
    monkeypatch.setenv("HISPARSE_AUX_BITS", "24" if variant == "pairs24" else "32")
    if variant.endswith("-lane-sums"):
        monkeypatch.setenv("HISPARSE_ROW_RUNS", "0" if "-no-" in variant else "1")
    monkeypatch.setenv("HISPARSE_COL_SLICES", str(slices))


_MADE = {}


def _designed(impl):
    # 1100 x 110000 (14 sub-tiles of x, several row blocks; small output banks: several row partitions), formatted once per mode
    if impl not in _MADE:
        m, x, kinds = fc.designed(1100, 110000, 11 + impl, hubs=3, hub_len=30000)
        v, _ = host.default_banks(impl)
        _, cp = cases.formatted(m, impl, v, 8 if impl == 2 else 1, True)
        assert cp.num_row_partitions > 1
        xp = np.zeros(cp.num_cols, dtype=np.float32)
        xp[: x.size] = x
        xw = host.pack_vector(impl, xp)
        ref = fc.Reference(m, xp, cp.num_rows)
        want = orc.spmv(impl, [cp.channel(c) for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                        cp.ob_bank, cp.vb_bank)
        _MADE[impl] = (m, cp, xp, xw, kinds, ref, want)
    return _MADE[impl]


def _teeth(ref, kinds, want):
    # the data can tell: csim's fp32 running sum breaks the one-slice D bound on most cancellation rows and many long rows, and a lost
    # or doubled product moves a long row by more than its bound
    bad = ref.violations(want, L=1)
    assert bad[kinds["cancel"]].mean() >= 0.9 and bad[kinds["long"]].mean() >= 0.3
    assert (ref.min_abs[kinds["long"]] > ref.bound(1)[kinds["long"]]).mean() >= 0.9


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("slices", [1, 3, 12])
def test_spmv_entry_points_keep_the_bound(impl, variant, slices, monkeypatch):
    m, cp, xp, xw, kinds, ref, want = _designed(impl)
    _teeth(ref, kinds, want)
    _force(monkeypatch, variant, slices)
    empty = kinds["empty"]
    hip = _Hip()
    with device.SpmvEngine(impl, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
        eng.set_option("carry_combine", "1")
        eng.load_matrix(cp)
        st = eng.stats()
        _assert_forced_plan(st, cp, impl, m.nnz)
        S = int(st["col_slices"])
        L = fc.chain(variant, m, eng.read_tiles())
        if variant.startswith("pairs") or variant.startswith("delta"):
            assert S == slices
        eng.load_vector(xw)
        outs = {}
        eng.run()
        outs["run"] = eng.read_result()
        eng.run()
        outs["run again"] = eng.read_result()
        y_dev = eng.device_result()
        for burst in (2, 3):                 # back to back: the combine of each step but the last is carried into the next kernel
            poison = np.full(cp.num_rows, 0x7fc0dead, dtype=np.uint32)     # nothing left over may pass for the carried sum
            assert hip.rt.hipMemcpy(y_dev, poison.ctypes.data, poison.nbytes, 1) == 0
            for k in range(burst):
                eng.run()
            # y as the last kernel left it: the step before, combined by that kernel (the last step's own sum is still owed --
            # hs_run; the device pointer is read past the library, which would settle it first)
            assert hip.rt.hipDeviceSynchronize() == 0
            outs[f"burst {burst} step {burst - 2} (carried)"] = hip.download(y_dev, (cp.num_rows,))
            outs[f"burst {burst} step {burst - 1} (stand-alone)"] = eng.read_result()
        eng.load_matrix(cp)                  # (y zeroed) the reference's partition loop
        eng.load_vector(xw)
        for j in range(cp.num_row_partitions):
            eng.run_partition(j, cp.part_len(j))
        outs["partitions"] = eng.read_result()
        eng.run_batch(3)
        outs["batch"] = eng.read_result()
        eng.set_option("batch_graph", "1")
        eng.run_batch(3)
        outs["batch graph"] = eng.read_result()
    for what, y in outs.items():
        ref.check(y, L=L, slices=S, what=f"{variant} S={S} {what}")
        assert (y[empty] == 0).all() and (y[m.shape[0]:] == 0).all(), what     # empty and padded rows: exactly +0.0


@pytest.mark.parametrize("impl", [1, 2])
def test_spmm_routes_keep_the_bound(impl, monkeypatch):
    # fused BITMAP (4 columns), matrix engine (16), four vectors over a SWEEP image, and the SpMV loop (spmm_fused = 0)
    m, x, kinds = fc.designed(600, 9000, 21 + impl, hubs=2, hub_len=6000)
    v, o = host.default_banks(impl)
    _, cp = cases.formatted(m, impl, v, o, True)
    rng = np.random.default_rng(5)
    Xf = np.zeros((16, cp.num_cols), dtype=np.float32)
    Xf[:, :9000] = np.stack([fc.magnitudes(rng, 9000) for _ in range(16)])
    X = np.stack([host.pack_vector(impl, Xf[j]) for j in range(16)])
    refs = [fc.Reference(m, Xf[j], cp.num_rows) for j in range(16)]
    exact = [fc.Reference(m, Xf[j], cp.num_rows, exact_products=True) for j in range(16)]
    n = np.maximum(np.diff(m.indptr), 1)
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "bitmap")
    monkeypatch.setenv("HISPARSE_COL_SLICES", "1")
    with device.SpmvEngine(impl) as eng:
        eng.load_matrix(cp)
        assert device.STREAM_FORMATS[eng.stats()["stream_format"]] == "bitmap"
        assert eng.read_mfma_image().size > 0
        Y16 = eng.spmm(X)                                        # the matrix engine
        monkeypatch.setenv("HISPARSE_SPMM_MFMA", "0")
        Y4 = eng.spmm(X[:4])                                     # the fused BITMAP kernel
        monkeypatch.delenv("HISPARSE_SPMM_MFMA")
        eng.set_option("spmm_fused", "0")
        Yloop = eng.spmm(X[:3])
    # the route: hs_spmm takes the matrix engine for >= 5 float columns whenever the second image exists (hs_spmm.cpp, hs_spmm_device; asserted
    # above) -- and its words are not the fused kernel's: FMAs over unrounded products against fp32 batches summed in double
    assert not np.array_equal(Y16[:4], Y4)
    for j in range(16):
        exact[j].check(Y16[j], L=n + 1, what=f"matrix engine column {j}")    # n FMAs from a zero accumulator: n roundings
    for j in range(4):
        refs[j].check(Y4[j], L=8, what=f"fused bitmap column {j}")
    for j in range(3):
        refs[j].check(Yloop[j], L=8, what=f"spmm_fused=0 column {j}")
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "sweep")
    for slices in ("", "3"):
        with device.SpmvEngine(impl) as eng:
            eng.set_option("spmm_vectors", "4")
            if slices:
                eng.set_option("col_slices", slices)
            eng.load_matrix(cp)
            st = eng.stats()
            assert device.STREAM_FORMATS[st["stream_format"]] == "sweep"
            Y = eng.spmm(X[:7])
            eng.set_option("spmm_fused", "0")
            Yl = eng.spmm(X[:2])
        for j in range(7):
            refs[j].check(Y[j], L=1, slices=int(st["col_slices"]), what=f"spmm_vectors=4 S={st['col_slices']} column {j}")
        for j in range(2):
            refs[j].check(Yl[j], L=1, slices=int(st["col_slices"]), what=f"sweep spmm_fused=0 column {j}")


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("repeated", [False, True])
def test_spmspv_keeps_the_bound(impl, repeated):
    m, x, kinds = fc.designed(3000, 20000, 31 + impl, hubs=2, hub_len=12000)
    indptr, ridx, words = host.csr_to_csc(host.CSRMatrix.from_scipy(m), impl)
    rng = np.random.default_rng(7)
    xi = np.sort(rng.choice(20000, 4000, replace=False))
    if repeated:                                 # some columns twice and three times: passes of unique columns, added in fp32 (kAdd)
        xi = np.concatenate([xi, xi[::3], xi[::7]])
    xv = fc.magnitudes(rng, xi.size)
    with device.SpmvEngine(impl) as eng:
        eng.load_matrix_csc(indptr, ridx, words, 3000)
        y = eng.spmspv(xi.astype(np.uint32), host.pack_vector(impl, xv))
    # the same products as a matrix with one column per entry
    ref = fc.Reference(m.tocsc()[:, xi].tocsr(), xv, 3000)
    passes = int(np.unique(xi, return_counts=True)[1].max())
    ref.check(y, L=1, slices=passes, what=f"spmspv passes={passes}")
    if not repeated:
        assert (ref.min_abs[kinds["long"]] > ref.bound(1)[kinds["long"]]).mean() >= 0.5


_EDGES = {}


def _edge_case(impl):
    """A designed matrix over 3 sub-tiles (20003 columns: the formatter pads x to 20008 words) plus rows that meet the IEEE edges, and an x
    with inf / -inf / NaN at sub-tile (8191 | 8192), 64-column group (63 | 64, 16383 | 16384) and column-slice borders (3 slices: the
    sub-tile borders), at a column no element uses and in the padded words beyond the real columns.  Returns
    (m, xp, cp, ref, r0, kinds): r0 .. r0 + 5 non-finite rows, r0 + 6 / r0 + 7 overflow rows, r0 + 8 .. r0 + 15 subnormal rows,
    r0 + 16 .. empty rows."""
    if impl in _EDGES:
        return _EDGES[impl]
    rows, cols = 420, 20003
    m, x, kinds = fc.designed(400, cols, 41 + impl, hubs=2, hub_len=15000)
    m = sp.vstack([m, sp.csr_matrix((20, cols), dtype=np.float32)]).tolil()
    nonfinite = {63: np.inf, 64: -np.inf, 8191: np.nan, 8192: np.inf, 16383: -np.inf, 16384: np.nan}
    unused = 19999
    m[:, unused] = 0
    m = m.tocsr()
    m.eliminate_zeros()
    dense_extra = {}
    r0 = 400
    dense_extra[r0] = {63: 1.5, 10: 2.0}                              # + inf
    dense_extra[r0 + 1] = {63: 1.0, 64: 1.0}                          # inf - inf
    dense_extra[r0 + 2] = {8191: 1.0, 5: 1.0}                         # NaN
    dense_extra[r0 + 3] = {8192: 0.0, 7: 1.0}                         # explicit stored zero under inf: NaN
    dense_extra[r0 + 4] = {16383: 3.0}                                # - inf
    dense_extra[r0 + 5] = {16384: 0.0}                                # 0 x NaN
    big = 2.0 ** 125                                                  # x = 4: products of +-2^127
    dense_extra[r0 + 6] = {100: big, 101: big, 102: -big}             # overflow rows: a fp32 running sum passes 2^128, E = +-2^127
    dense_extra[r0 + 7] = {200: -big, 201: -big, 202: big}
    for k in range(8):                                                # subnormal products: 2^-70 x 2^-70 ~ 2^-140
        dense_extra[r0 + 8 + k] = {300 + 3 * j: float(np.float32(2.0 ** -70 * (1 + j / 7))) for j in range(1 + 9 * k)}
    ip, ix, dv = list(m.indptr[: r0 + 1]), list(m.indices[: m.indptr[r0]]), list(m.data[: m.indptr[r0]])
    for r in range(r0, rows):
        for c, v in sorted(dense_extra.get(r, {}).items()):
            ix.append(c)
            dv.append(v)
        ip.append(len(ix))
    m = sp.csr_matrix((np.array(dv, dtype=np.float32), np.array(ix), np.array(ip)), shape=(rows, cols))
    assert m.nnz == len(dv)                                           # explicit zeros are kept
    for c, v in nonfinite.items():
        x[c] = v
    x[unused] = np.nan
    x[100:103] = 4.0
    x[200:203] = 4.0
    x[300:500] = np.float32(2.0 ** -70 * 1.25)
    v, o = host.default_banks(impl)
    _, cp = cases.formatted(m, impl, v, o, True)
    assert cp.num_cols > cols                                         # there ARE padded x words
    xp = np.full(cp.num_cols, np.nan, dtype=np.float32)               # padded x words beyond the real columns: NaN
    xp[:cols] = x
    ref = fc.Reference(m, xp, cp.num_rows)
    assert ref.nan[[r0 + 1, r0 + 2, r0 + 3, r0 + 5]].all() and ref.inf[r0] == 1 and ref.inf[r0 + 4] == -1
    assert np.isfinite(ref.E[r0 + 6]) and abs(ref.E[r0 + 6]) == 2.0 ** 127
    sub = np.arange(r0 + 8, r0 + 16)
    assert (np.abs(ref.E[sub]) < 2.0 ** -126).all() and (ref.E[sub] != 0).all()
    _EDGES[impl] = (m, xp, cp, ref, r0, kinds)
    return _EDGES[impl]


def _check_edges(y, ref, r0, kinds, L, S, d_class, what):
    check = np.ones(ref.num_rows, dtype=bool)
    if not d_class or S > 1:
        check[[r0 + 6, r0 + 7]] = False      # the finite answer past an fp32 running sum is promised by the one-slice D paths only
    bad = ref.violations(y, L=L, slices=S) & check
    assert not bad.any(), (what, np.nonzero(bad)[0][:8], y[bad][:8].view(np.float32))
    if d_class and S == 1:
        assert y[r0 + 6] == np.float32(ref.E[r0 + 6]).view(np.uint32), what       # fl32(E), finite
    assert (y[r0 + 8: r0 + 16] != 0).all(), what                                  # subnormal products are kept (vector ALU)
    assert (y[np.r_[kinds["empty"], r0 + 16: ref.num_rows]] == 0).all(), what     # empty rows: exactly +0.0


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("slices", [1, 3])
def test_non_finite_x_and_ieee_edges(impl, variant, slices, monkeypatch):
    m, xp, cp, ref, r0, kinds = _edge_case(impl)
    _force(monkeypatch, variant, slices)
    with device.SpmvEngine(impl, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        _assert_forced_plan(st, cp, impl, m.nnz)
        L = fc.chain(variant, m, eng.read_tiles())
        eng.load_vector(host.pack_vector(impl, xp))
        eng.run()
        y = eng.read_result()
    S = int(st["col_slices"])
    if variant.startswith("pairs") or variant.startswith("delta"):
        assert S == slices
    _check_edges(y, ref, r0, kinds, L, S, variant in D_VARIANTS, f"{variant} S={S}")


@pytest.mark.parametrize("impl", [1, 2])
def test_non_finite_x_through_spmm_and_spmspv(impl, monkeypatch):
    # the same edges through the fused BITMAP SpMM (4 columns), the four-vector SpMM over a SWEEP image and hs_spmspv (x as entries)
    m, xp, cp, ref, r0, kinds = _edge_case(impl)
    xw = host.pack_vector(impl, xp)
    fin = np.where(np.isfinite(xp), xp, np.float32(1.0)).astype(np.float32)
    ref_fin = fc.Reference(m, fin, cp.num_rows)
    X = np.stack([xw, host.pack_vector(impl, fin), xw, xw])
    refs = [ref, ref_fin, ref, ref]
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "bitmap")
    monkeypatch.setenv("HISPARSE_COL_SLICES", "1")
    monkeypatch.setenv("HISPARSE_SPMM_MFMA", "0")
    with device.SpmvEngine(impl, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "bitmap" and st["col_slices"] == 1
        Y = eng.spmm(X)
    for j in range(4):
        _check_edges(Y[j], refs[j], r0, kinds, 8, 1, False, f"fused bitmap column {j}")
    monkeypatch.setenv("HISPARSE_STREAM_FORMAT", "sweep")
    with device.SpmvEngine(impl, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank) as eng:
        eng.set_option("spmm_vectors", "4")
        eng.load_matrix(cp)
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "sweep" and st["col_slices"] == 1
        Y = eng.spmm(X)
    for j in range(4):
        _check_edges(Y[j], refs[j], r0, kinds, 1, 1, True, f"spmm_vectors=4 column {j}")
    indptr, ridx, words = host.csr_to_csc(host.CSRMatrix.from_scipy(m), impl)
    cols = m.shape[1]
    with device.SpmvEngine(impl) as eng:
        eng.load_matrix_csc(indptr, ridx, words, m.shape[0])
        y = eng.spmspv(np.arange(cols, dtype=np.uint32), xw[:cols])       # every column an entry, the non-finite ones included
    ref_s = fc.Reference(m, xp[:cols])
    _check_edges(y, ref_s, r0, kinds, 1, 1, True, "spmspv")


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("variant", ["pairs", "delta", "bitmap", "owner24", "sweep"])
def test_non_finite_matrix_values_through_load_csr(impl, variant, monkeypatch):
    m, x, kinds = fc.designed(300, 20000, 51 + impl, hubs=1, hub_len=12000)
    m = m.tocsr()
    data = m.data.copy()
    marks = {}
    for k, (r, val) in enumerate([(20, np.inf), (31, -np.inf), (42, np.nan), (53, np.inf)]):
        data[m.indptr[r]] = val
        marks[r] = val
    data[m.indptr[53] + 1] = -np.inf if m.indptr[54] - m.indptr[53] > 1 else data[m.indptr[53] + 1]
    m2 = sp.csr_matrix((data, m.indices, m.indptr), shape=m.shape)
    _force(monkeypatch, variant)
    with device.SpmvEngine(impl) as eng:
        eng.load_matrix_csr((m.shape[0], m.shape[1], m.indptr, m.indices, data))
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == variant and st["light_kernel"] == 0 and st["col_slices"] == 1
        L = fc.chain(variant, m2, eng.read_tiles())
        xp = np.zeros(eng.num_cols, dtype=np.float32)
        xp[: x.size] = x
        eng.load_vector(host.pack_vector(impl, xp))
        eng.run()
        y = eng.read_result()
        nrows = eng.num_rows
    ref = fc.Reference(m2, xp, nrows)
    assert not ref.finite[list(marks)].any()
    ref.check(y, L=L, what=f"{variant} load_csr")
