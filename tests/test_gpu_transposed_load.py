"""hs_load_matrix_csr_transposed: A^T from A's CSR arrays, with the value map in A's order.

"The reference load" is load_matrix_csr of scipy's m.T.tocsr() on a second engine; `perm` takes A's value order to that of m.T.tocsr().
The contract is byte identity with the reference load: stats (apart from load_seconds), image, Block[], Unit[] and the matrix-engine
image, for every plan and numeric mode; the segment edges of the 16-element cursor; a symmetric matrix gives the plain load's bytes from
the same arrays; update_values takes A's order (the bytes of a fresh transposed load of b, and of the reference load of b[perm]); a
forward and a backward engine refreshed from ONE device buffer; the host fallbacks; the refusals; device memory comes back; a seeded fuzz.
Shapes are non-square so that a swapped dimension cannot cancel out, banks are small so that small matrices span several row and column
partitions."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from hisparse_amd import device, host
from oracle import oracle as orc

import cases

pytestmark = pytest.mark.gpu

PLANS = {
    "pairs": {"stream_format": "pairs", "light": "0"},
    "pairs24": {"stream_format": "pairs", "light": "0", "aux_bits": "24"},
    "delta": {"stream_format": "delta"},
    "owner": {"stream_format": "owner"},
    "owner24": {"stream_format": "owner24"},
    "sweep": {"stream_format": "sweep"},
    "bitmap": {"stream_format": "bitmap"},
    "light": {"stream_format": "pairs", "light": "1"},
    "slices2": {"col_slices": "2", "light": "0"},
    "spmm4": {"spmm_vectors": "4"},
    "autotune": {"autotune": "1"},
    "planner": {},
}
ENV = ("HISPARSE_STREAM_FORMAT", "HISPARSE_LIGHT", "HISPARSE_COL_SLICES", "HISPARSE_AUX_BITS", "HISPARSE_SPMM_VECTORS", "HISPARSE_AUTOTUNE",
       "HISPARSE_VALUE_MAP", "HISPARSE_BITMAP_BUILD", "HISPARSE_RETILE", "HISPARSE_MAX_ROWS", "HISPARSE_SWEEP", "HISPARSE_CARRY_COMBINE")
VB = 16


def _ob(impl):
    return 8 if impl == 2 else 2


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _engine(impl, opts, value_map=False):
    eng = device.SpmvEngine(impl, ob_bank=_ob(impl), vb_bank=VB)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_option("value_map", "1" if value_map else "0")
    return eng


def _snapshot(eng):
    st = {k: v for k, v in eng.stats().items() if k != "load_seconds"}
    t = eng.read_tiles()
    return st, t["image"].tobytes(), t["blocks"].tobytes(), t["units"].tobytes(), eng.read_mfma_image().tobytes()


def _arrays(m, values=None):
    return (m.shape[0], m.shape[1], m.indptr.astype(np.uint32), m.indices.astype(np.uint32),
            np.ascontiguousarray(m.data if values is None else values, dtype=np.float32))


def _transposed(m):
    """(m.T.tocsr(), perm): the host-transposed matrix and the permutation from m's value order into its own"""
    tag = sp.csr_matrix((np.arange(m.nnz, dtype=np.float64), m.indices, m.indptr), shape=m.shape).T.tocsr()
    perm = tag.data.astype(np.int64)
    mt = sp.csr_matrix((m.data[perm], tag.indices, tag.indptr), shape=tag.shape)
    return mt, perm


def _oracle(m, impl, xw, values=None):
    cp = host.format_matrix(host.CSRMatrix.from_arrays(*_arrays(m, values)), impl, vb_bank=VB, ob_bank=_ob(impl), skip_empty_rows=True)
    return orc.spmv(impl, [cp.channel_ptr(c)[0] for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                    cp.ob_bank, cp.vb_bank)


def _same_y(impl, got, want):
    return np.array_equal(got, want) if impl == 0 else cases.float_close(got, want)


def _y(eng, xw):
    eng.load_vector(xw)
    eng.run()
    return eng.read_result()


def _names(a, b):
    return [n for n, x, y in zip(("stats", "image", "Block[]", "Unit[]", "matrix-engine image"), a, b) if x != y]


def _check_identity(m, impl, opts, what, oracle=True):
    """transposed load of m against the reference load; returns the transposed engine's stats"""
    mt, _ = _transposed(m)
    with _engine(impl, opts) as t, _engine(impl, opts) as ref:
        t.load_matrix_csr(_arrays(m), transpose=True)
        ref.load_matrix_csr(_arrays(mt))
        divisor = 128 * (8 if impl == 2 else 1)
        assert (t.num_rows, t.num_cols) == (-(-m.shape[1] // divisor) * divisor, -(-m.shape[0] // 8) * 8) == (ref.num_rows, ref.num_cols), what
        a, b = _snapshot(t), _snapshot(ref)
        assert a == b, f"{what}: {_names(a, b)} differ from the reference load"
        if oracle:
            xw = host.pack_vector(impl, cases.random_x(t.num_cols, 3, impl))
            assert _same_y(impl, _y(t, xw), _oracle(mt, impl, xw)), f"{what}: y differs from the oracle of the host-transposed matrix"
        return a[0]


# ---- 1. byte identity ------------------------------------------------------------------------------------------------------------------
def _shapes(plan):
    if plan == "bitmap":
        return [(600, 5000, 0.2), (5000, 600, 0.2)]
    if plan == "light":
        return [(1500, 1200, 0.01)]
    return [(2500, 700, 0.02), (700, 2500, 0.02)]


IDENTITY_PLANS = ["pairs", "pairs24", "delta", "owner", "owner24", "sweep", "bitmap", "light", "slices2", "spmm4", "planner"]


@pytest.mark.parametrize("impl", [0, 1, 2])
@pytest.mark.parametrize("plan,shape", [(p, s) for p in IDENTITY_PLANS for s in _shapes(p)])
def test_same_bytes_as_the_host_transposed_load(plan, shape, impl):
    rows, cols, density = shape
    m = cases.random_csr(rows, cols, density, 13, impl)
    st = _check_identity(m, impl, PLANS[plan], f"{plan}/{impl}/{rows}x{cols}")
    assert st["nnz"] == m.nnz and st["retiled_on_gpu"] == 1
    if plan == "slices2":
        assert st["col_slices"] == 2
    if plan == "bitmap":
        assert device.STREAM_FORMATS[st["stream_format"]] == "bitmap"
    if plan == "light":
        assert st["light_kernel"] == 1


# ---- 2. segment edges of the 16-element cursor ---------------------------------------------------------------------------------------------
def _edge_matrices(impl):
    rng = np.random.default_rng(7)

    def values(n):
        return (rng.uniform(0.1, 2.0, n) if impl == 0 else rng.normal(0.0, 1.0, n)).astype(np.float32)

    def from_coo(rows, cols, r, c):
        m = sp.csr_matrix((values(len(r)), (np.asarray(r), np.asarray(c))), shape=(rows, cols), dtype=np.float32)
        m.sort_indices()
        return m

    out = {}
    for n in (1, 15, 16, 17):                                       # one thread's segment: under, exactly, one over
        cells = rng.choice(37 * 53, n, replace=False)
        out[f"nnz{n}"] = from_coo(37, 53, cells // 53, cells % 53)
    out["1xN"] = from_coo(1, 300, np.zeros(120, int), rng.choice(300, 120, replace=False))
    out["Nx1"] = from_coo(300, 1, rng.choice(300, 120, replace=False), np.zeros(120, int))
    # rows of A empty at the start, in the middle and at the end; the others hold 0-2 entries, so a segment crosses several empty rows
    live = np.array([i for i in range(10, 190) if not 50 <= i < 85])
    r = np.repeat(live, rng.integers(0, 3, live.size))
    out["empty_rows"] = from_coo(200, 90, r, rng.integers(0, 90, r.size))      # (a cell drawn twice is summed into one entry)
    # empty columns of A (empty rows of A^T), the last ones before the padding among them
    live = np.array([c for c in range(260) if not 40 <= c < 70 and c < 250])
    cells = rng.choice(150 * live.size, 700, replace=False)
    out["empty_cols"] = from_coo(150, 260, cells // live.size, live[cells % live.size])
    cells = rng.choice(131 * 77 - 1, 300, replace=False)
    out["last_corner"] = from_coo(131, 77, np.append(cells // 77, 130), np.append(cells % 77, 76))
    return out


@pytest.mark.parametrize("impl", [0, 2])
def test_segment_edges(impl):
    mats = _edge_matrices(impl)
    assert mats["empty_rows"].nnz > 64 and mats["last_corner"][130, 76] != 0
    for name, m in mats.items():
        _check_identity(m, impl, {}, f"{name}/{impl}")


@pytest.mark.parametrize("impl", [0, 2])
def test_unsorted_columns_explicit_zeros_and_negative_values(impl):
    rng = np.random.default_rng(5)
    m = cases.random_csr(1300, 900, 0.01, 6, impl)
    ip, ix, dv = m.indptr.copy(), m.indices.copy(), m.data.copy()
    for r in range(m.shape[0]):
        a, b = ip[r], ip[r + 1]
        p = rng.permutation(b - a)
        ix[a:b], dv[a:b] = ix[a:b][p], dv[a:b][p]
    dv[::17] = 0.0
    dv[5::23] = -1.0             # negative: 0 in Q8.24, still a stored element
    shuffled = sp.csr_matrix((dv, ix, ip), shape=m.shape)
    assert not shuffled.has_sorted_indices and shuffled.nnz == m.nnz
    _check_identity(shuffled, impl, {}, f"unsorted/{impl}")


# ---- 3. symmetric pin: no scipy transposition involved -------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 2])
@pytest.mark.parametrize("plan", ["planner", "delta", "sweep", "bitmap"])
def test_symmetric_matrix_gives_the_plain_loads_bytes(plan, impl):
    r = cases.random_csr(1300, 1300, 0.2 if plan == "bitmap" else 0.01, 17, impl)
    m = (r + r.T).tocsr().astype(np.float32)
    m.sort_indices()
    assert (m != m.T).nnz == 0
    with _engine(impl, PLANS[plan]) as t, _engine(impl, PLANS[plan]) as plain:
        t.load_matrix_csr(_arrays(m), transpose=True)
        plain.load_matrix_csr(_arrays(m))
        a, b = _snapshot(t), _snapshot(plain)
        assert a == b, f"{_names(a, b)} differ between the transposed and the plain load of the same symmetric arrays"


# ---- 4. value map in A's order --------------------------------------------------------------------------------------------------------------
def _hard_values(n, impl, seed):
    """negative values, zeros, NaN, +-inf, values above 256 (saturation), exact Q8.24 half-ulp ties"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0.0, 2.0, n) if impl == 0 else rng.normal(0.0, 1.0, n)).astype(np.float32)
    v[0::11] = -rng.uniform(0.1, 5.0, v[0::11].size)
    v[1::13] = 0.0
    v[2::17] = np.nan
    v[3::19] = np.inf
    v[4::23] = -np.inf
    v[5::29] = rng.uniform(256.0, 1e6, v[5::29].size)
    v[6::31] = (rng.integers(0, 1 << 20, v[6::31].size) + 0.5) / 16777216.0      # (k + 1/2) ulps: exactly representable, a rounding tie
    return v


def _finite_values(n, impl, seed):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0.0, 3.0, n) if impl == 0 else rng.normal(0.0, 1.5, n)).astype(np.float32)
    v[::9] = 0.0
    if impl == 0:
        v[1::7] = -1.0
    return v


def _fresh(impl, opts, load, kept):
    """snapshots of fresh value_map = 0 loads done by load(engine).  autotune times plans: its pick may differ between two loads, so the
    reference is then also taken with the kept format forced (what autotune's final load does) -- the one whose plan matches counts."""
    refs = [opts]
    if "autotune" in opts:
        refs += [{"stream_format": device.STREAM_FORMATS[kept["stream_format"]], "light": "0"}, {}]
    snaps = []
    for o in refs:
        with _engine(impl, o) as eng:
            load(eng)
            snaps.append(_snapshot(eng))
    return snaps


def _assert_same(snap, refs, what):
    plan = [r for r in refs if r[0] == snap[0] and r[2] == snap[2] and r[3] == snap[3]]
    assert plan, f"{what}: no reference load has the same plan (stats / Block[] / Unit[])"
    assert snap[1] == plan[0][1], f"{what}: image bytes differ"
    assert snap[4] == plan[0][4], f"{what}: matrix-engine image differs"


@pytest.mark.parametrize("plan,impl", [(p, i) for p in ("delta", "owner24", "sweep", "bitmap", "light", "slices2", "autotune") for i in (0, 1, 2)
                                       if not (p == "bitmap" and i == 0)])
def test_update_takes_the_order_of_the_arrays_passed_in(plan, impl):
    rows, cols, density = _shapes(plan)[0]
    m = cases.random_csr(rows, cols, density, 23, impl)
    mt, perm = _transposed(m)
    a, b = m.data.astype(np.float32), _hard_values(m.nnz, impl, 100 + impl)
    with _engine(impl, PLANS[plan], True) as eng:
        eng.load_matrix_csr(_arrays(m, a), transpose=True)
        assert eng.csr_nnz == m.nnz
        first = _snapshot(eng)
        if plan == "bitmap":
            assert first[4], "a float BITMAP matrix keeps the matrix-engine image (and the second map)"
        eng.update_values(b)
        after = _snapshot(eng)
        _assert_same(after, _fresh(impl, PLANS[plan], lambda e: e.load_matrix_csr(_arrays(m, b), transpose=True), first[0]), f"{plan}/{impl}: fresh transposed load of b")
        _assert_same(after, _fresh(impl, PLANS[plan], lambda e: e.load_matrix_csr(_arrays(mt, b[perm])), first[0]), f"{plan}/{impl}: reference load of b[perm]")
        eng.update_values(a)
        assert _snapshot(eng) == first, f"{plan}/{impl}: updating back to a does not restore the first load's bytes"


# ---- 5. forward and backward engine, one device value buffer ----------------------------------------------------------------------------------
class _Hip:
    """device buffers through the HIP runtime libhisparse_hip.so itself uses (ctypes), freed together by close()"""

    def __init__(self):
        device.lib()
        self.rt = C.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def zeros(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), max(int(nbytes), 16)) == 0
        assert self.rt.hipMemset(p, 0, max(int(nbytes), 16)) == 0
        self.bufs.append(p)
        return p.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.zeros(a.nbytes)
        assert self.rt.hipMemcpy(C.c_void_p(p), a.ctypes.data, a.nbytes, 1) == 0
        return p

    def get(self, ptr, n, dtype=np.uint32):
        a = np.empty(n, dtype=dtype)
        assert self.rt.hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) == 0
        return a

    def close(self):
        assert self.rt.hipDeviceSynchronize() == 0
        for p in self.bufs:
            self.rt.hipFree(p)
        self.bufs = []


@pytest.mark.parametrize("impl", [0, 2])
def test_forward_and_backward_engines_share_one_device_value_buffer(impl):
    m = cases.random_csr(2500, 700, 0.02, 41, impl)
    mt, perm = _transposed(m)
    first, second = _finite_values(m.nnz, impl, 9), _finite_values(m.nnz, impl, 10)
    hip = _Hip()
    with _engine(impl, {}, True) as fwd, _engine(impl, {}, True) as bwd:
        fwd.load_matrix_csr(_arrays(m))
        bwd.load_matrix_csr(_arrays(m), transpose=True)
        assert (fwd.num_cols, bwd.num_cols) == (704, 2504) and 700 <= bwd.num_rows < fwd.num_rows
        x = host.pack_vector(impl, cases.random_x(fwd.num_cols, 6, impl))        # y = W x
        g = host.pack_vector(impl, cases.random_x(bwd.num_cols, 7, impl))        # g_x = W^T g_y
        fwd.load_vector(x)
        bwd.load_vector(g)
        bufs = [hip.put(first), hip.put(second)]
        outs = [(hip.zeros(fwd.num_rows * 4), hip.zeros(bwd.num_rows * 4)) for _ in bufs]
        for values_dev, (out_f, out_b) in zip(bufs, outs):                        # no synchronisation in between: stream order
            fwd.update_values_device(values_dev, m.nnz)
            bwd.update_values_device(values_dev, m.nnz)                           # the same pointer, no permutation
            fwd.run(); fwd.push_result([out_f], fwd.num_rows)
            bwd.run(); bwd.push_result([out_b], bwd.num_rows)
        fwd.sync()
        bwd.sync()
        got = [(hip.get(f, fwd.num_rows), hip.get(b, bwd.num_rows)) for f, b in outs]
    hip.close()
    for (yf, yb), values in zip(got, (first, second)):
        assert _same_y(impl, yf, _oracle(m, impl, x, values)), "forward y"
        assert _same_y(impl, yb, _oracle(mt, impl, g, values[perm])), "backward y"
    assert not np.array_equal(got[0][1], got[1][1])


# ---- 6. host fallbacks ----------------------------------------------------------------------------------------------------------------------
def _rc_update(eng, n):
    v = np.ones(n, dtype=np.float32)
    return device.lib().hs_update_values(eng._h, v.ctypes.data, n)


@pytest.mark.parametrize("impl", [0, 1])
def test_duplicate_entries_are_formatted_on_the_host_and_add_up(impl):
    ip = np.array([0, 2, 2, 3], dtype=np.uint32)            # A is 3 x 10 with (0, 4) twice: A^T holds (4, 0) twice
    dup = (3, 10, ip, np.array([4, 4, 1], dtype=np.uint32), np.array([1.0, 2.0, 4.0], dtype=np.float32))
    with _engine(impl, {}, True) as eng:
        eng.load_matrix_csr(dup, transpose=True)
        assert eng.stats()["retiled_on_gpu"] == 0 and eng.stats()["nnz"] == 3
        assert eng.num_cols == 8 and eng.num_rows % 128 == 0
        xs = np.array([1.0, 2.0, 3.0, 0, 0, 0, 0, 0], dtype=np.float32)
        y = orc.unpack_result(impl, _y(eng, host.pack_vector(impl, xs)))
        assert y[:10].tolist() == [0.0, 12.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0] and not y[10:].any(), "both products of the duplicate entry are added"
        assert _rc_update(eng, 3) == -6 and b"host builder" in device.lib().hs_last_error(eng._h)
        m = cases.random_csr(700, 300, 0.02, 3, impl)       # the context is usable: a good load, and its update
        eng.load_matrix_csr(_arrays(m), transpose=True)
        assert eng.stats()["retiled_on_gpu"] == 1
        xw = host.pack_vector(impl, cases.random_x(eng.num_cols, 4, impl))
        assert _same_y(impl, _y(eng, xw), _oracle(_transposed(m)[0], impl, xw))
        eng.update_values(m.data)


@pytest.mark.parametrize("impl", [0, 1])
def test_bitmap_built_on_the_host_gives_the_device_builds_image(impl):
    m = cases.random_csr(600, 5000, 0.2, 52, impl)
    with _engine(impl, {"stream_format": "bitmap", "bitmap_build": "host"}, True) as on_host, _engine(impl, {"stream_format": "bitmap"}, True) as on_dev:
        on_host.load_matrix_csr(_arrays(m), transpose=True)
        on_dev.load_matrix_csr(_arrays(m), transpose=True)
        a, b = _snapshot(on_host), _snapshot(on_dev)
        assert a[0].pop("retiled_on_gpu") == 0 and b[0].pop("retiled_on_gpu") == 1
        assert a == b, f"{_names(a, b)} differ between the host and the device build"
        assert _rc_update(on_host, m.nnz) == -6 and b"host builder" in device.lib().hs_last_error(on_host._h)
        assert _rc_update(on_dev, m.nnz) == 0
        xw = host.pack_vector(impl, cases.random_x(on_host.num_cols, 4, impl))
        assert _same_y(impl, _y(on_host, xw), _oracle(_transposed(m)[0], impl, xw))


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------
def test_refused_loads_leave_the_context_usable():
    impl = 0
    m = cases.random_csr(300, 90, 0.05, 8, impl)
    mt, _ = _transposed(m)
    rows, cols, ip, ix, dv = _arrays(m)
    bad_ix = ix.copy(); bad_ix[m.nnz // 2] = cols             # an index equal to num_cols (a legal ROW of A: it is not one)
    assert cols < rows
    down = ip.copy(); down[7] = down[8] + 1
    off = ip.copy(); off[0] = 1
    lib = device.lib()
    with _engine(impl, {}) as eng:
        xw = None
        for what, args in (("column", (ip, bad_ix)), ("indptr", (down, ix)), ("indptr", (off, ix)), (None, None)):
            if what:
                with pytest.raises(device.DeviceError, match=what) as err:
                    eng.load_matrix_csr((rows, cols, args[0], args[1], dv), transpose=True)
                assert err.value.code == -4
            else:
                assert lib.hs_load_matrix_csr_transposed(eng._h, rows, cols, None, ix.ctypes.data, dv.ctypes.data, None, None) == -1      # a null indptr
            eng.load_matrix_csr(_arrays(m), transpose=True)   # usable for a following good load
            xw = host.pack_vector(impl, cases.random_x(eng.num_cols, 4, impl)) if xw is None else xw
            assert _same_y(impl, _y(eng, xw), _oracle(mt, impl, xw))
        # an empty matrix of the right shape is fine
        eng.load_matrix_csr((3, 10, np.zeros(4, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)), transpose=True)
        assert eng.num_cols == 8 and not _y(eng, np.zeros(eng.num_cols, dtype=np.uint32)).any()


# ---- 8. memory --------------------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    device.lib()
    rt = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert rt.hipDeviceSynchronize() == 0
    assert rt.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_load_update_reload_cycles_give_memory_back():
    # (hipMemGetInfo counts the whole device, which other processes share: the allowance of tests/test_gpu_value_update.py)
    m = cases.random_csr(20000, 30000, 0.004, 62, 1)
    b = _finite_values(m.nnz, 1, 13)
    before = _free_bytes()
    for _ in range(4):
        with _engine(1, {}, True) as eng:
            eng.load_matrix_csr(_arrays(m), transpose=True)
            eng.update_values(b)
            eng.load_matrix_csr(_arrays(m, b))
            eng.update_values(m.data)
            eng.set_option("stream_format", "bitmap")
            eng.load_matrix_csr(_arrays(m), transpose=True)
            eng.update_values(b)
    assert before - _free_bytes() <= (64 << 20)


# ---- 9. seeded fuzz -----------------------------------------------------------------------------------------------------------------------------
FUZZ_PLANS = ["pairs", "pairs24", "delta", "owner", "owner24", "sweep", "bitmap", "light", "slices2", "planner"]
FUZZ_SEED, FUZZ_CASES = 20261017, 40


def fuzz_cases():
    """(case, impl, plan, matrix) of the seeded fuzz; nnz == 0 cases included (the test skips those, and only those)"""
    rng = np.random.default_rng(FUZZ_SEED)
    for case in range(FUZZ_CASES):
        impl = int(rng.integers(0, 3))
        plan = FUZZ_PLANS[int(rng.integers(0, len(FUZZ_PLANS)))]
        rows, cols = int(rng.integers(64, 6001)), int(rng.integers(8, 30001))
        density = float(min(0.3, 10 ** rng.uniform(-3.5, -0.7)))
        density = min(density, 2e5 / (rows * cols))              # at most ~200 K non-zeros a case
        yield case, impl, plan, cases.random_csr(rows, cols, density, 3000 + case, impl)


def test_seeded_fuzz_byte_identity():
    failures, empty = [], 0
    for case, impl, plan, m in fuzz_cases():
        if m.nnz == 0:
            empty += 1
            continue
        mt, perm = _transposed(m)
        b = _hard_values(m.nnz, impl, case)
        with _engine(impl, PLANS[plan], True) as t, _engine(impl, PLANS[plan], False) as ref:
            t.load_matrix_csr(_arrays(m), transpose=True)
            ref.load_matrix_csr(_arrays(mt))
            if _snapshot(t) != _snapshot(ref):
                failures.append((case, impl, plan, m.shape, m.nnz, "load"))
                continue
            t.update_values(b)
            ref.load_matrix_csr(_arrays(mt, b[perm]))
            if _snapshot(t) != _snapshot(ref):
                failures.append((case, impl, plan, m.shape, m.nnz, "update"))
    assert empty <= 2, f"{empty} of the seeded cases have no non-zero"
    assert not failures, failures[:10]
