"""The fused attention step (include/hisparse_attention.h) on the device: the cases of tests/attention_cases.py against the HIP library,
what hsat_info reports, the stride loop over more than two trips of the grid at the widest group, long rows among short and empty
ones, and the call on one caller-owned stream with the chain hsw_sddmm_device -> hsr_softmax_device that recomputes P, which ties lse
to the existing objects.  The same cases on libhisparse_cpu.so: tests/test_attention_cpu.py."""
import math

import numpy as np
import pytest

from hisparse_amd import attention, device, rows, wide

import attention_cases as ac
import rows_cases as rc
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return ac.HipMemory()


@pytest.mark.parametrize("d", ac.DS)
def test_general(mem, d):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, pad 0 and 8, lse taken and NULL, the host form and the device form"""
    ac.general(mem, (d,))


def test_what_info_reports():
    indptr, indices = ac.random_pattern(ac.ROWS, ac.COLS, ac.NNZ, 1)
    for ip, ix, shape in ((indptr, indices, (ac.ROWS, ac.COLS)), (np.zeros(6, dtype=np.uint32), np.zeros(0, dtype=np.uint32), (5, 7))):
        with attention.PatternAttention((ip, ix, shape)) as pa:
            assert pa.info() == {"nnz": ix.size, "device_bytes": 4 * (shape[0] + 1) + 4 * max(ix.size, 1) + 4 * shape[0]}


def test_edges(mem):
    ac.edges(mem)


@pytest.mark.parametrize("d", [4, 64])
def test_score_order(mem, d):
    ac.score_order(mem, (d,))


def test_non_finite_scores(mem):
    ac.non_finite(mem)


def test_scale_zero(mem):
    ac.scale_zero(mem)


def test_heads_by_leading_dimension(mem):
    ac.heads(mem)


def test_a_call_leaves_nothing_for_the_next(mem):
    ac.nothing_carried_over(mem)


def test_refusals(mem):
    ac.refusals(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def _large(mem, shape, indptr, indices, d, seed, what):
    """the device form over one large pattern, every word inside its bound (float64 sums as the reference)"""
    Q, K, V = ac.operands(shape, d, seed)
    ref = ac.reference(indptr, indices, Q, K, V, 0.5, exact=False)
    with attention.PatternAttention((indptr, indices, shape)) as pa:
        ref.check(*ac.device_form(mem, pa, Q, K, V, 0.5, 4, True, what), what)
    return ref


def test_stride_loop_over_the_shortest_class_at_the_widest_group(mem):
    """rows of 1 ... 4 entries over 1000 columns at d = 256: one group of 64 lanes per row, four rows per workgroup, and more than two
    trips of the grid (20 000 rows, or as many as the device's CU count asks for by the same formula)"""
    n_cols, d = 1000, 256
    assert wide.team_lanes(1, d) == 64
    n_rows = max(20000, 2 * wide.rows_per_trip(_compute_units(), 1, d) + 1000)
    assert 2 * wide.rows_per_trip(_compute_units(), 1, d) < n_rows
    rng = np.random.default_rng(2100)
    lengths = rng.integers(1, 5, n_rows)
    indptr = rc.indptr_of(lengths)
    indices = rng.integers(0, n_cols, int(indptr[-1])).astype(np.uint32)
    _large(mem, (n_rows, n_cols), indptr, indices, d, 2110, f"{n_rows} short rows, d 256")


@pytest.mark.parametrize("d", [4, 64])
def test_long_rows_among_short_and_empty_rows(mem, d):
    """2001 rows x 4096 columns: rows of 513, 1025 and 3000 entries, 199 of 1 ... 39, the others (the first and the last among them) empty"""
    rng = np.random.default_rng(2200)
    n_rows, n_cols = 2001, 4096
    lengths = np.zeros(n_rows, dtype=np.int64)
    live = rng.choice(np.arange(1, n_rows - 1), 202, replace=False)
    lengths[live] = rng.integers(1, 40, live.size)
    lengths[live[:3]] = (513, 1025, 3000)
    assert lengths[0] == lengths[-1] == 0 and (lengths > wide.WIDE_LONG).sum() == 3 and (lengths > 0).sum() == 202
    indptr = rc.indptr_of(lengths)
    indices = np.concatenate([rng.choice(n_cols, int(n), replace=False) for n in lengths if n]).astype(np.uint32)
    ref = _large(mem, (n_rows, n_cols), indptr, indices, d, 2210 + d, f"long rows among short and empty ones, d {d}")
    assert ref.empty.sum() == n_rows - 202 and ref.finite.sum() == 202


def test_one_stream_with_the_chain_that_recomputes_p(mem):
    """2000 x 3000, 40 000 entries, d = 20 with ld = 24: hsat_forward_device on a caller-owned stream, then hsw_sddmm_device ->
    hsr_softmax_device on the same stream, no host synchronisation until the end.  For every non-empty row sum_e P[e] = 1 within hsr's
    bound (3 2^-23 P + 2^-125 per entry), and exp(scale S[e] - lse[r]) = P[e] within expm1(2 eta_r) + 3 2^-23 relative, with S and P
    as the chain wrote them and lse as the fused call wrote it."""
    import scipy.sparse as sp
    n_rows, n_cols, d, ld, scale = 2000, 3000, 20, 24, 0.5
    rng = np.random.default_rng(2300)
    flat = np.sort(rng.choice(n_rows * n_cols, 40000, replace=False))
    m = sp.csr_matrix((np.ones(flat.size, dtype=np.float32), (flat // n_cols, flat % n_cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    indptr, indices, shape = m.indptr.astype(np.uint32), m.indices.astype(np.uint32), (n_rows, n_cols)
    Q, K, V = ac.operands(shape, d, 2310)
    (dq, _), (dk, _), (dv, _) = (wc._features_in(mem, a, ld - wc.round_up4(d)) for a in (Q, K, V))
    dy = mem.alloc(np.full((n_rows, ld), ac.SENTINEL, dtype=np.uint32))
    dl = mem.alloc(np.full(n_rows, ac.SENTINEL, dtype=np.uint32))
    ds, dp = (mem.alloc(np.full(m.nnz, ac.SENTINEL, dtype=np.uint32)) for _ in range(2))
    st = mem.stream()
    with attention.PatternAttention(m) as pa, wide.WideProducts(m, transposed=False) as wp, rows.RowSoftmax(m) as rs:
        for obj in (pa, wp, rs):
            obj.set_stream(st.value)
        pa.forward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, d, scale, dy.ptr, ld, dl.ptr)
        wp.sddmm_device(dq.ptr, ld, dk.ptr, ld, d, ds.ptr)
        rs.softmax_device(ds.ptr, scale, dp.ptr)
        assert mem.rt.hipStreamSynchronize(st) == 0
        y = np.ascontiguousarray(mem.fetch(dy).reshape(n_rows, ld)[:, :d]).view(np.float32)
        lse, S, P = (mem.fetch(b).view(np.float32) for b in (dl, ds, dp))
        for obj in (pa, wp, rs):
            obj.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    ref = ac.reference(indptr, indices, Q, K, V, scale)
    ref.check(y, lse, "one stream with the chain")
    assert not ref.bad.any() and not ref.dead.any()
    wc.Reference("sddmm", shape, indptr, indices, Q, K).check(S, "one stream with the chain, S")
    rc.forward_check(m.indptr, S, scale, P, "one stream with the chain, P")
    of = ac.entry_rows(indptr)
    p64 = P.astype(np.float64).tolist()
    ip = indptr.tolist()
    worst_sum = worst_p = 0.0
    for r in np.nonzero(ref.finite)[0]:
        total = math.fsum(p64[ip[r]: ip[r + 1]])
        worst_sum = max(worst_sum, abs(total - 1.0) / (3.0 * 2.0 ** -23 * total + (ip[r + 1] - ip[r]) * 2.0 ** -125))
    t = (np.float32(scale) * S).astype(np.float64)                       # one fp32 multiply, as both kernels form it
    again = np.exp(t - lse.astype(np.float64)[of])
    rel = np.abs(again - P.astype(np.float64)) / P.astype(np.float64)
    worst_p = float((rel / (np.expm1(2.0 * ref.eta[of]) + 3.0 * 2.0 ** -23)).max())
    print(f"sum of P / bound = {worst_sum:.3f}; exp(scale S - lse) against P / bound = {worst_p:.3f}")
    assert (P > 0).all()
    assert worst_sum <= 1.0, worst_sum
    assert worst_p <= 1.0, worst_p
