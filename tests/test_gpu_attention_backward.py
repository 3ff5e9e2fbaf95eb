"""The fused attention backward step (include/hisparse_attention_backward.h) on the device: the cases of
tests/attention_backward_cases.py against the HIP library, what hsab_info reports, the stride loops of both kernels over more than two
trips of the grid at the widest group, long rows and long columns among short and empty ones, the training step hsat_forward_device ->
hsab_backward_device on one caller-owned stream (with gV against the recomputing chain's hsw_spmm_t_device), and the call captured into
a graph.  The same cases on libhisparse_cpu.so: tests/test_attention_backward_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from hisparse_amd import attention, attention_backward, device, rows, wide

import attention_backward_cases as bc
import attention_cases as ac
import rows_cases as rc
import wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return bc.HipMemory()


@pytest.mark.parametrize("d", bc.DS)
def test_general(mem, d):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, pad 0 and 8, the host form and the device form"""
    bc.general(mem, (d,))


def test_what_info_reports():
    indptr, indices = bc.random_pattern(bc.ROWS, bc.COLS, bc.NNZ, 1)
    for ip, ix, (r, c) in ((indptr, indices, (bc.ROWS, bc.COLS)), (np.zeros(6, dtype=np.uint32), np.zeros(0, dtype=np.uint32), (5, 7))):
        with attention_backward.PatternAttentionBackward((ip, ix, (r, c))) as pb:
            assert pb.info() == {"nnz": ix.size, "device_bytes": 4 * (r + 1) + 4 * max(ix.size, 1) + 4 * r + 4 * (c + 1) + 4 * max(ix.size, 1) + 4 * c + 8 * r}


def test_edges(mem):
    bc.edges(mem)


def test_special_rows(mem):
    bc.special_rows(mem)


def test_scale_zero(mem):
    bc.scale_zero(mem)


def test_heads_by_leading_dimension(mem):
    bc.heads(mem)


def test_a_call_leaves_nothing_for_the_next(mem):
    bc.nothing_carried_over(mem)


def test_refusals(mem):
    bc.refusals(mem)


def _compute_units():
    import scipy.sparse as sp
    m = sp.random(128, 64, density=0.03, format="csr", dtype=np.float32, random_state=1)
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr((128, 64, m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ones(m.nnz, dtype=np.float32)))
        return eng.stats()["num_compute_units"]


def _large(mem, shape, indptr, indices, d, seed, what):
    """the device form over one large pattern, every word inside its bound (float64 sums as the reference)"""
    Q, K, V, gY = bc.operands(shape, d, seed)
    scores = bc.scores_of(indptr, indices, Q, K, exact=False)
    lse = bc.forward_lse(scores, V, 0.5)
    ref = bc.Reference(scores, V, gY, lse, 0.5)
    with attention_backward.PatternAttentionBackward((indptr, indices, shape)) as pb:
        ref.check(*bc.device_form(mem, pb, Q, K, V, gY, lse, 0.5, 4, what), what)
    return ref


def _transposed(shape, indptr, indices):
    """the CSR arrays of the transposed pattern"""
    rows_, cols_ = shape
    cptr, trow, _ = wc.transposed_pattern(rows_, cols_, indptr, indices)
    return (cols_, rows_), np.asarray(cptr, dtype=np.uint32), np.asarray(trow, dtype=np.uint32)


def _short_rows(n_cols, d):
    """rows of 1 ... 4 entries over n_cols columns: more than two trips of the grid at class 1 (20 000 rows, or as many as the device's CU
    count asks for by the same formula)"""
    assert wide.team_lanes(1, d) == 64
    n_rows = max(20000, 2 * wide.rows_per_trip(_compute_units(), 1, d) + 1000)
    assert 2 * wide.rows_per_trip(_compute_units(), 1, d) < n_rows
    rng = np.random.default_rng(5100)
    indptr = rc.indptr_of(rng.integers(1, 5, n_rows))
    return (n_rows, n_cols), indptr, rng.integers(0, n_cols, int(indptr[-1])).astype(np.uint32)


def test_stride_loop_of_the_row_side_at_the_widest_group(mem):
    """rows of 1 ... 4 entries over 1000 columns at d = 256: one group of 64 lanes per row, four rows per workgroup, and more than two
    trips of the grid in the row kernel"""
    shape, indptr, indices = _short_rows(1000, 256)
    _large(mem, shape, indptr, indices, 256, 5110, f"{shape[0]} short rows, d 256")


def test_stride_loop_of_the_column_side_at_the_widest_group(mem):
    """the mirror image: that many columns of 1 ... 4 entries over 1000 rows, more than two trips of the grid in the column kernel"""
    shape, indptr, indices = _transposed(*_short_rows(1000, 256))
    lengths = np.bincount(indices, minlength=shape[1])
    assert shape[0] == 1000 and lengths.min() >= 1 and lengths.max() <= 4
    _large(mem, shape, indptr, indices, 256, 5120, f"{shape[1]} short columns, d 256")


def _long_rows():
    """2001 rows x 4096 columns: rows of 513, 1025 and 3000 entries, 199 of 1 ... 39, the others (the first and the last among them) empty"""
    rng = np.random.default_rng(5200)
    n_rows, n_cols = 2001, 4096
    lengths = np.zeros(n_rows, dtype=np.int64)
    live = rng.choice(np.arange(1, n_rows - 1), 202, replace=False)
    lengths[live] = rng.integers(1, 40, live.size)
    lengths[live[:3]] = (513, 1025, 3000)
    assert lengths[0] == lengths[-1] == 0 and (lengths > wide.WIDE_LONG).sum() == 3 and (lengths > 0).sum() == 202
    indptr = rc.indptr_of(lengths)
    indices = np.concatenate([rng.choice(n_cols, int(n), replace=False) for n in lengths if n]).astype(np.uint32)
    return (n_rows, n_cols), indptr, indices


@pytest.mark.parametrize("d", [4, 64])
def test_long_rows_among_short_and_empty_rows(mem, d):
    shape, indptr, indices = _long_rows()
    ref = _large(mem, shape, indptr, indices, d, 5210 + d, f"long rows among short and empty ones, d {d}")
    assert ref.empty_r.sum() == shape[0] - 202 and sorted(ref.n[ref.n > wide.WIDE_LONG]) == [513, 1025, 3000]


@pytest.mark.parametrize("d", [4, 64])
def test_long_columns_among_short_and_empty_columns(mem, d):
    """the transpose-shaped twin, 4096 x 2001: columns of 513, 1025 and 3000 entries among short and empty ones"""
    shape, indptr, indices = _transposed(*_long_rows())
    ref = _large(mem, shape, indptr, indices, d, 5220 + d, f"long columns among short and empty ones, d {d}")
    assert shape == (4096, 2001) and ref.empty_c.sum() == shape[1] - 202 and sorted(ref.m[ref.m > wide.WIDE_LONG]) == [513, 1025, 3000]


def _step_inputs():
    """2000 x 3000, 40 000 entries, d = 20 with ld = 24"""
    import scipy.sparse as sp
    n_rows, n_cols, d, ld = 2000, 3000, 20, 24
    rng = np.random.default_rng(5300)
    flat = np.sort(rng.choice(n_rows * n_cols, 40000, replace=False))
    m = sp.csr_matrix((np.ones(flat.size, dtype=np.float32), (flat // n_cols, flat % n_cols)), shape=(n_rows, n_cols))
    m.sort_indices()
    return m, bc.operands((n_rows, n_cols), d, 5310), d, ld


def _step_buffers(mem, m, ops, d, ld):
    ins = [wc._features_in(mem, a, ld - wc.round_up4(d))[0] for a in ops]
    outs = [mem.alloc(np.full((n, ld), bc.SENTINEL, dtype=np.uint32)) for n in (m.shape[0], m.shape[0], m.shape[1], m.shape[1])]      # y, gq, gk, gv
    return ins, outs, mem.alloc(np.full(m.shape[0], bc.SENTINEL, dtype=np.uint32))


def _features(mem, buf, d, ld):
    w = mem.fetch(buf).reshape(-1, ld)
    assert (w[:, d:] == bc.SENTINEL).all()
    return np.ascontiguousarray(w[:, :d]).view(np.float32)


def test_one_stream_forward_then_backward(mem):
    """hsat_forward_device then hsab_backward_device on a caller-owned stream, one synchronisation at the end: three launches.  gQ, gK and gV
    are inside the bounds computed from the lse words the device wrote.  Then the recomputing chain on the same stream, hsw_sddmm_device ->
    hsr_softmax_device -> hsw_spmm_t_device(P, gY): its gV and the fused one differ by at most the sum of the contracts' bounds --
    the fused call's around sum P' gY with P' = exp(scale S - lse), hsw_spmm_t's around the sum of the fp32 products of the chain's P and gY
    (each off by u |P gY| from the real product), and |P' - P| <= (expm1(2 eta_r) + 3 2^-23) P from lse's and hsr_softmax's contracts (as
    tests/test_gpu_attention.py asserts it)."""
    m, (Q, K, V, gY), d, ld = _step_inputs()
    indptr, indices, shape, scale = m.indptr.astype(np.uint32), m.indices.astype(np.uint32), m.shape, 0.5
    (dq, dk, dv, dg), (dy, oq, ok, ov), dl = _step_buffers(mem, m, (Q, K, V, gY), d, ld)
    ds, dp = (mem.alloc(np.full(m.nnz, bc.SENTINEL, dtype=np.uint32)) for _ in range(2))
    chain_v = mem.alloc(np.full((shape[1], ld), bc.SENTINEL, dtype=np.uint32))
    st = mem.stream()
    with attention.PatternAttention(m) as pa, attention_backward.PatternAttentionBackward(m) as pb, wide.WideProducts(m, transposed=True) as wp, rows.RowSoftmax(m) as rs:
        for obj in (pa, pb, wp, rs):
            obj.set_stream(st.value)
        pa.forward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, d, scale, dy.ptr, ld, dl.ptr)
        pb.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, d, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld)
        assert mem.rt.hipStreamSynchronize(st) == 0
        lse = mem.fetch(dl).view(np.float32)
        gq, gk, gv = (_features(mem, b, d, ld) for b in (oq, ok, ov))
        wp.sddmm_device(dq.ptr, ld, dk.ptr, ld, d, ds.ptr)
        rs.softmax_device(ds.ptr, scale, dp.ptr)
        wp.spmm_t_device(dp.ptr, dg.ptr, ld, d, chain_v.ptr, ld)
        assert mem.rt.hipStreamSynchronize(st) == 0
        P = mem.fetch(dp).view(np.float32)
        gv_chain = _features(mem, chain_v, d, ld)
        for obj in (pa, pb, wp, rs):
            obj.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    scores = bc.scores_of(indptr, indices, Q, K)
    fwd = ac.Reference(scores, V, scale)
    fwd.check(_features(mem, dy, d, ld), lse, "forward then backward, the forward")
    assert np.isfinite(lse).all()
    ref = bc.Reference(scores, V, gY, lse, scale)
    ref.check(gq, gk, gv, "forward then backward on one stream")
    chain = wc.Reference("spmm_t", shape, indptr, indices, P, gY)
    chain.check(gv_chain, "the chain's gV")
    of = scores.of
    kappa = np.expm1(2.0 * fwd.eta[of]) + 3.0 * 2.0 ** -23
    between = ac._seg_sum((((2.0 ** -24 + kappa) * P.astype(np.float64))[:, None] * np.abs(ref.G64))[ref.perm], ref.cptr)
    ratio = np.abs(gv.astype(np.float64) - gv_chain.astype(np.float64)) / (ref.bound["gv"] + chain.bound + between)
    print(f"gV fused against the chain: difference / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0, ratio.max()


def _graph_runtime(rt):
    vp = C.c_void_p
    rt.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    rt.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    rt.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, vp, vp, C.c_size_t]
    rt.hipGraphLaunch.argtypes = [vp, vp]
    rt.hipGraphGetNodes.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    rt.hipGraphGetRootNodes.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    rt.hipGraphGetEdges.argtypes = [vp, vp, vp, C.POINTER(C.c_size_t)]
    rt.hipGraphExecDestroy.argtypes = [vp]
    rt.hipGraphDestroy.argtypes = [vp]


def test_graph_capture(mem):
    """hsab_backward_device captured into a graph on a caller-owned stream and replayed once: the bits of the direct call, and the graph is
    one linear branch -- two kernel nodes, one root, one edge"""
    m, (Q, K, V, gY), d, ld = _step_inputs()
    scale, rt = 0.5, mem.rt
    _graph_runtime(rt)
    lse = bc.forward_lse(bc.scores_of(m.indptr.astype(np.uint32), m.indices.astype(np.uint32), Q, K), V, scale)
    (dq, dk, dv, dg), (_, oq, ok, ov), dl = _step_buffers(mem, m, (Q, K, V, gY), d, ld)
    assert rt.hipMemcpy(C.c_void_p(dl.ptr), lse.ctypes.data, lse.nbytes, 1) == 0
    (_, gq2, gk2, gv2) = _step_buffers(mem, m, (Q, K, V, gY), d, ld)[1]
    st = mem.stream()
    graph, run = C.c_void_p(), C.c_void_p()
    with attention_backward.PatternAttentionBackward(m) as pb:
        pb.set_stream(st.value)
        pb.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, d, scale, oq.ptr, ld, ok.ptr, ld, ov.ptr, ld)
        assert rt.hipStreamSynchronize(st) == 0
        direct = [_features(mem, b, d, ld) for b in (oq, ok, ov)]
        assert rt.hipStreamBeginCapture(st, 2) == 0                      # hipStreamCaptureModeRelaxed
        pb.backward_device(dq.ptr, ld, dk.ptr, ld, dv.ptr, ld, dg.ptr, ld, dl.ptr, d, scale, gq2.ptr, ld, gk2.ptr, ld, gv2.ptr, ld)
        assert rt.hipStreamEndCapture(st, C.byref(graph)) == 0 and graph.value
        assert (mem.fetch(gq2) == bc.SENTINEL).all(), "the captured call ran"
        nodes, roots, edges = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert rt.hipGraphGetNodes(graph, None, C.byref(nodes)) == 0 and rt.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0
        assert rt.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
        assert (nodes.value, roots.value, edges.value) == (2, 1, 1), (nodes.value, roots.value, edges.value)
        assert rt.hipGraphInstantiate(C.byref(run), graph, None, None, 0) == 0
        assert rt.hipGraphLaunch(run, st) == 0 and rt.hipStreamSynchronize(st) == 0
        replayed = [_features(mem, b, d, ld) for b in (gq2, gk2, gv2)]
        assert rt.hipGraphExecDestroy(run) == 0 and rt.hipGraphDestroy(graph) == 0
        pb.set_stream(None)
    rt.hipStreamDestroy(st)
    assert bc.same_words(direct, replayed)
