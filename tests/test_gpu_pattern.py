"""The sampled dense product (include/hisparse_pattern.h) on the device: the cases of tests/pattern_cases.py against the HIP library in all
three numeric modes, the grid-stride loop and the tail, row expansion at scale, independence from the staging of an earlier call, the
result consumed as it is by hs_update_values_device (forward and transposed context, one caller-owned stream), and stream order after
hs_run.  The same cases on libhisparse_cpu.so: tests/test_pattern_cpu.py."""
import numpy as np
import pytest

from hisparse_amd import device, host, pattern

import pattern_cases as pc

pytestmark = pytest.mark.gpu

IMPLS = (0, 1, 2)


@pytest.fixture(scope="module")
def mem():
    return pc.HipMemory()


def test_general_in_every_mode_and_both_float_modes_alike(mem):
    words = pc.general(mem, IMPLS)
    for k in pc.KS:
        assert np.array_equal(words[1][k], words[2][k]), k


def test_nan_reaches_exactly_its_entry(mem):
    pc.nan_reaches_its_entry(mem, (1, 2))


def test_pattern_edges(mem):
    pc.edges(mem, IMPLS)


def test_refusals(mem):
    pc.refusals(mem, IMPLS)


def test_info_reports_what_the_object_holds():
    indptr, indices = pc.random_pattern(300, 517, 4001, 3)
    with pattern.SampledProduct(0, (indptr, indices, (300, 517)), 1) as sp:
        assert sp.info() == {"nnz": 4001, "device_bytes": 2 * 4004 * 4}                    # rows and columns, whole 16-byte words; max_k = 1 stages nothing
    with pattern.SampledProduct(1, (indptr, indices, (300, 517)), 6) as sp:
        assert sp.info() == {"nnz": 4001, "device_bytes": 2 * 4004 * 4 + 2 * (300 + 517) * 16}


BIG_ROWS, BIG_COLS, BIG_NNZ = 70000, 90001, (1 << 22) + 3
_BIG = {}


def big_pattern():
    if not _BIG:
        _BIG["p"] = pc.random_pattern(BIG_ROWS, BIG_COLS, BIG_NNZ, 11)
    return _BIG["p"]


@pytest.mark.parametrize("impl", [0, 1])
def test_stride_loop_and_tail(mem, impl):
    """more entries than one trip of the grid covers, and nnz mod 4 = 3: every word against the numpy reference (float: the header's
    double sum in ascending j rounded once, which is inside its bound by construction -- math.fsum over 4 M entries would take the
    test's whole budget)"""
    with device.SpmvEngine(0) as eng:
        eng.load_matrix_csr(_csr(_matrix(128, 64, 200, 1), np.ones(200, dtype=np.float32)))
        cus = eng.stats()["num_compute_units"]
    assert pattern.entries_per_pass(cus) <= 1 << 22 < BIG_NNZ and BIG_NNZ % pattern.SDDMM_ENTRIES_PER_LANE == 3
    indptr, indices = big_pattern()
    with pattern.SampledProduct(impl, (indptr, indices, (BIG_ROWS, BIG_COLS)), 5) as sp:
        assert sp.nnz == BIG_NNZ
        for k in (1, 5):
            U, V = pc.vectors(impl, k, BIG_ROWS, 100 + k), pc.vectors(impl, k, BIG_COLS, 200 + k)
            got, out = pc.device_form(mem, sp, U, V)
            if impl == 0:
                want = pc.fixed_ref(indptr, indices, U, V)
                assert np.array_equal(got, want), (k, np.nonzero(got != want)[0][:5])
                again, _ = pc.device_form(mem, sp, U, V, accumulate_into=got, out=out)
                assert np.array_equal(again, pc.fixed_ref(indptr, indices, U, V, old=got)), k
            else:
                assert pc.same_floats(got, pc.float_exact(pc.float_products(indptr, indices, U, V))), k


def test_row_expansion_at_scale(mem):
    """200 000 rows, nine in ten empty, one row of 300 000 entries, the rest short: k = 1 in fixed point, bit exact"""
    rng = np.random.default_rng(12)
    rows, cols = 200000, 250000
    counts = np.zeros(rows, dtype=np.int64)
    live = rng.choice(rows, rows // 10, replace=False)
    counts[live] = rng.integers(1, 6, live.size)
    counts[live[0]] = 300000
    counts[0] = counts[rows - 1] = 0
    assert (counts == 0).mean() >= 0.9
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    indices = rng.integers(0, cols, int(indptr[-1])).astype(np.uint32)
    U, V = pc.vectors(0, 1, rows, 13), pc.vectors(0, 1, cols, 14)
    with pattern.SampledProduct(0, (indptr, indices, (rows, cols)), 1) as sp:
        got, _ = pc.device_form(mem, sp, U, V)
    assert np.array_equal(got, pc.fixed_ref(indptr, indices, U, V))


@pytest.mark.parametrize("impl", IMPLS)
def test_a_call_leaves_nothing_for_the_next(impl):
    """16 vectors, then 3 on the same object: the words of a fresh object (stale staging words of the wider call must not reach the padding)"""
    indptr, indices = pc.random_pattern(pc.ROWS, pc.COLS, pc.NNZ, 4)
    shape = (indptr, indices, (pc.ROWS, pc.COLS))
    U16, V16 = pc.vectors(impl, 16, pc.ROWS, 15, 4.0), pc.vectors(impl, 16, pc.COLS, 16, 4.0)
    U3, V3 = pc.vectors(impl, 3, pc.ROWS, 17), pc.vectors(impl, 3, pc.COLS, 18)
    with pattern.SampledProduct(impl, shape, 16) as sp, pattern.SampledProduct(impl, shape, 16) as fresh:
        pc.check(impl, sp.sddmm(U16, V16), indptr, indices, U16, V16, "16 vectors")
        second = sp.sddmm(U3, V3)
        assert np.array_equal(second, fresh.sddmm(U3, V3))
        pc.check(impl, second, indptr, indices, U3, V3, "3 vectors after 16")


def _matrix(rows, cols, nnz, seed):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(rows * cols, nnz, replace=False))
    m = sp.csr_matrix((rng.normal(size=nnz).astype(np.float32), (flat // cols, flat % cols)), shape=(rows, cols))
    m.sort_indices()
    return m


def _csr(m, values):
    return (m.shape[0], m.shape[1], m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ascontiguousarray(values, dtype=np.float32))


@pytest.mark.parametrize("transpose", [False, True])
def test_result_is_consumed_as_it_is_by_update_values_device(mem, transpose):
    """The point of the feature, in float mode: SDDMM into a device buffer, hs_update_values_device with that buffer, hs_run -- on ONE
    caller-owned stream for both objects -- gives, bit for bit, the y of a fresh load of the same arrays with the values READ BACK from the
    buffer.  Order and layout, not the arithmetic a second time."""
    impl, k = 1, 4
    m = _matrix(2000, 3000, 40000, 21)
    st = mem.stream()
    U, V = pc.vectors(impl, k, 2000, 22), pc.vectors(impl, k, 3000, 23)
    du, dv, out = mem.alloc(U), mem.alloc(V), mem.alloc(np.zeros(m.nnz, dtype=np.uint32))
    with device.SpmvEngine(impl) as eng, pattern.SampledProduct(impl, m, k) as sp:
        eng.set_option("value_map", "1")
        eng.load_matrix_csr(_csr(m, m.data), transpose=transpose)
        x = host.pack_vector(impl, np.random.default_rng(24).normal(size=eng.num_cols).astype(np.float32))
        eng.load_vector(x)
        eng.set_stream(st.value)
        sp.set_stream(st.value)
        eng.run()
        sp.sddmm_device(du.ptr, 2000, dv.ptr, 3000, k, out.ptr)
        eng.update_values_device(out.ptr, m.nnz)
        eng.run()
        y = eng.read_result()
        assert mem.rt.hipStreamSynchronize(st) == 0
        values = mem.fetch(out).view(np.float32)
        eng.set_stream(None)
        sp.set_stream(None)
    mem.rt.hipStreamDestroy(st)
    pc.float_check(values.view(np.uint32), pc.float_products(m.indptr, m.indices, U, V), 1, "the buffer")
    assert np.isfinite(values).all() and np.count_nonzero(values) > 0.99 * m.nnz
    with device.SpmvEngine(impl) as fresh:
        fresh.load_matrix_csr(_csr(m, values), transpose=transpose)
        fresh.load_vector(x)
        fresh.run()
        want = fresh.read_result()
    assert want.any() and np.array_equal(y, want)


@pytest.mark.parametrize("impl", [0, 1])
def test_stream_order_after_hs_run(mem, impl):
    """hs_run into a bound y, then SDDMM with that y as U, on one caller-owned stream and with no host synchronisation in between: the
    words of the synchronised computation"""
    m = _matrix(2000, 3000, 40000, 31)
    if impl == 0:
        m.data[:] = np.random.default_rng(32).uniform(0.0, 0.2, m.nnz).astype(np.float32)
    st = mem.stream()
    V = pc.vectors(impl, 1, 3000, 33)
    dv, out = mem.alloc(V), mem.alloc(np.zeros(m.nnz, dtype=np.uint32))
    with device.SpmvEngine(impl) as eng, pattern.SampledProduct(impl, m, 1) as sp:
        eng.load_matrix_csr(_csr(m, m.data))
        yb = mem.alloc(np.zeros(eng.num_rows, dtype=np.uint32))
        eng.load_vector(pc.vectors(impl, 1, eng.num_cols, 34)[0])
        eng.bind_device_result(yb.ptr)
        eng.set_stream(st.value)
        sp.set_stream(st.value)
        eng.run()
        sp.sddmm_device(yb.ptr, eng.num_rows, dv.ptr, 3000, 1, out.ptr)      # ldu = padded_rows of the context
        assert mem.rt.hipStreamSynchronize(st) == 0
        got, y = mem.fetch(out), mem.fetch(yb)
        eng.set_stream(None)
        sp.set_stream(None)
        eng.bind_device_result(None)
    mem.rt.hipStreamDestroy(st)
    assert y[:2000].any()
    pc.check(impl, got, m.indptr, m.indices, y[None, :2000], V, f"SDDMM over the y of hs_run, impl {impl}")
    if impl:
        assert pc.same_floats(got, pc.float_exact(pc.float_products(m.indptr, m.indices, y[None, :2000], V)))
