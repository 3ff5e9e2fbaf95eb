"""hs_update_values / hs_update_values_device (option value_map): a loaded CSR matrix gets new values in place.

The contract is byte identity: after an update the image, Block[], Unit[] and the matrix-engine image are what a fresh value_map = 0 load
of the same pattern with the new values leaves -- every format, the LIGHT and sliced plans, the four-vector SWEEP image, autotune and the
planner's own choice, in all three numeric modes; the option by itself changes nothing; results match the oracle of the new values through
every entry point; the update keeps stream order (also against a carried combine pass); refusals leave the context usable; the map costs
4 (8) bytes per non-zero and is given back; a seeded fuzz; the ogbl-ppa stand-in at full size; and the update is far cheaper than a reload.
"""
import ctypes as C
import time

import numpy as np
import pytest

from hisparse_amd import datasets, device, host
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
    "slices4": {"col_slices": "4", "light": "0"},
    "spmm4": {"spmm_vectors": "4"},
    "autotune": {"autotune": "1"},
    "planner": {},
}
ENV = ("HISPARSE_STREAM_FORMAT", "HISPARSE_LIGHT", "HISPARSE_COL_SLICES", "HISPARSE_AUX_BITS", "HISPARSE_SPMM_VECTORS", "HISPARSE_AUTOTUNE",
       "HISPARSE_VALUE_MAP", "HISPARSE_BITMAP_BUILD", "HISPARSE_RETILE", "HISPARSE_MAX_ROWS", "HISPARSE_SWEEP", "HISPARSE_CARRY_COMBINE")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _engine(impl, opts, value_map):
    eng = device.SpmvEngine(impl)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_option("value_map", "1" if value_map else "0")
    return eng


def _snapshot(eng):
    st = {k: v for k, v in eng.stats().items() if k != "load_seconds"}
    t = eng.read_tiles()
    return st, t["image"].tobytes(), t["blocks"].tobytes(), t["units"].tobytes(), eng.read_mfma_image().tobytes()


def _csr(m, values):
    return (m.shape[0], m.shape[1], m.indptr.astype(np.uint32), m.indices.astype(np.uint32), np.ascontiguousarray(values, dtype=np.float32))


def _fresh(impl, opts, m, values, kept=None):
    """snapshot of a fresh value_map = 0 load of (pattern of m, values).  autotune times plans: its pick may differ between two loads, so
    the reference is then also taken with the kept format forced (what autotune's final load does) -- the one whose plan matches counts."""
    refs = [opts]
    if "autotune" in opts and kept is not None:
        refs.append({"stream_format": device.STREAM_FORMATS[kept["stream_format"]], "light": "0"})
        refs.append({})
    snaps = []
    for o in refs:
        with _engine(impl, o, False) as eng:
            eng.load_matrix_csr(_csr(m, values))
            snaps.append(_snapshot(eng))
    return snaps


def _assert_same(snap, refs, what):
    plan = [r for r in refs if r[0] == snap[0] and r[2] == snap[2] and r[3] == snap[3]]
    assert plan, f"{what}: no reference load has the same plan (stats / Block[] / Unit[])"
    r = plan[0]
    assert snap[1] == r[1], f"{what}: image bytes differ"
    assert snap[4] == r[4], f"{what}: matrix-engine image differs"


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


def _oracle(m, values, impl, xw):
    cp = host.format_matrix(host.CSRMatrix.from_arrays(*_csr(m, values)), impl, skip_empty_rows=True)
    return orc.spmv(impl, [cp.channel_ptr(c)[0] for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                    cp.ob_bank, cp.vb_bank)


def _same_y(impl, got, want):
    return np.array_equal(got, want) if impl == 0 else cases.float_close(got, want)


def _matrix(plan, impl, seed=3):
    if plan == "light":
        return cases.random_csr(1500, 1200, 0.01, seed, impl)
    if plan == "bitmap":
        return cases.random_csr(600, 5000, 0.2, seed, impl)
    return cases.random_csr(3000, 24000, 0.003, seed, impl)


# ---- (a) byte identity with a fresh load, and back -------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1, 2])
@pytest.mark.parametrize("plan", list(PLANS))
def test_update_gives_the_bytes_of_a_fresh_load(plan, impl):
    m = _matrix(plan, impl)
    a = m.data.astype(np.float32)
    b = _hard_values(m.nnz, impl, 100 + impl)
    with _engine(impl, PLANS[plan], True) as eng:
        eng.load_matrix_csr(_csr(m, a))
        first = _snapshot(eng)
        st = first[0]
        if plan == "light":
            assert st["light_kernel"] == 1
        if plan.startswith("slices"):
            assert st["col_slices"] == int(plan[-1])
        if plan == "spmm4":
            assert device.STREAM_FORMATS[st["stream_format"]] == "sweep"
        if plan == "bitmap" and impl:
            assert first[4], "a float BITMAP matrix keeps the matrix-engine image"
        eng.update_values(b)
        _assert_same(_snapshot(eng), _fresh(impl, PLANS[plan], m, b, st), f"{plan}/{impl} -> B")
        eng.update_values(a)
        assert _snapshot(eng) == first, f"{plan}/{impl}: updating back to A does not give the first load's bytes"


# ---- (b) the option by itself changes nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1, 2])
@pytest.mark.parametrize("plan", list(PLANS))
def test_value_map_option_changes_nothing_by_itself(plan, impl):
    m = _matrix(plan, impl, seed=9)
    with _engine(impl, PLANS[plan], True) as eng:
        eng.load_matrix_csr(_csr(m, m.data))
        snap = _snapshot(eng)
    _assert_same(snap, _fresh(impl, PLANS[plan], m, m.data, snap[0]), f"{plan}/{impl}")


# ---- (c) results through every entry point ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1, 2])
@pytest.mark.parametrize("plan", ["planner", "slices2", "delta", "owner24", "sweep", "bitmap", "light"])
def test_results_after_update_match_the_oracle(plan, impl):
    m = _matrix(plan, impl, seed=21)
    b = _finite_values(m.nnz, impl, 7)
    with _engine(impl, PLANS[plan], True) as eng:
        eng.load_matrix_csr(_csr(m, m.data))
        xw = host.pack_vector(impl, cases.random_x(eng.num_cols, 5, impl))
        eng.load_vector(xw)
        eng.run()
        want_a, want_b = _oracle(m, m.data, impl, xw), _oracle(m, b, impl, xw)
        assert _same_y(impl, eng.read_result(), want_a)
        eng.update_values(b)
        eng.run()
        assert _same_y(impl, eng.read_result(), want_b), "hs_run"
        eng.load_vector(np.zeros_like(xw)); eng.run(); eng.load_vector(xw)
        eng.run_batch(3)
        assert _same_y(impl, eng.read_result(), want_b), "hs_run_batch"
        one = host.pack_vector(impl, np.ones(8, dtype=np.float32))[0]
        eng.iterate(1, int(one), 0)
        assert _same_y(impl, eng.read_result(), want_b), "hs_iterate"
        eng.load_vector(xw)


@pytest.mark.parametrize("impl", [0, 1, 2])
@pytest.mark.parametrize("path", ["bitmap_fused", "bitmap_mfma", "sweep4"])
def test_spmm_after_update_matches_the_oracle(path, impl):
    if path == "bitmap_mfma" and impl == 0:
        pytest.skip("the matrix-engine image exists for float matrices only")
    plan = "spmm4" if path == "sweep4" else "bitmap"
    m = _matrix(plan, impl, seed=31)
    b = _finite_values(m.nnz, impl, 8)
    with _engine(impl, PLANS[plan], True) as eng:
        if path == "bitmap_fused":
            eng.set_option("spmm_mfma", "0")
        eng.load_matrix_csr(_csr(m, m.data))
        if path == "bitmap_mfma":
            assert eng.read_mfma_image().size
        k = 4
        xs = np.stack([host.pack_vector(impl, cases.random_x(eng.num_cols, 40 + j, impl)) for j in range(k)])
        eng.spmm(xs)
        eng.update_values(b)
        got = eng.spmm(xs)
    for j in range(k):
        assert _same_y(impl, got[j], _oracle(m, b, impl, xs[j])), f"{path}: column {j}"


# ---- (d) stream order -------------------------------------------------------------------------------------------------------------------
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
def test_updates_keep_stream_order(impl):
    m = _matrix("planner", impl, seed=41)
    a, b = m.data.astype(np.float32), _finite_values(m.nnz, impl, 9)
    hip = _Hip()
    with _engine(impl, {}, True) as eng:
        eng.load_matrix_csr(_csr(m, a))
        xw = host.pack_vector(impl, cases.random_x(eng.num_cols, 6, impl))
        eng.load_vector(xw)
        da, db = hip.put(a), hip.put(b)
        outs = [hip.zeros(eng.num_rows * 4) for _ in range(3)]
        eng.run(); eng.push_result([outs[0]], eng.num_rows)
        eng.update_values_device(db, m.nnz)
        eng.run(); eng.push_result([outs[1]], eng.num_rows)
        eng.update_values_device(da, m.nnz)
        eng.run(); eng.push_result([outs[2]], eng.num_rows)
        eng.sync()
        ys = [hip.get(o, eng.num_rows) for o in outs]
    hip.close()
    want_a, want_b = _oracle(m, a, impl, xw), _oracle(m, b, impl, xw)
    assert _same_y(impl, ys[0], want_a) and _same_y(impl, ys[1], want_b) and _same_y(impl, ys[2], want_a)


@pytest.mark.parametrize("impl", [0, 1])
def test_update_between_carried_steps(impl):
    """run, run (its combine pass is owed), update, run, run on a sliced plan with the carried combine: every y of its own values"""
    m = cases.random_csr(3000, 40000, 0.004, 43, impl)
    a, b = m.data.astype(np.float32), _finite_values(m.nnz, impl, 10)
    hip = _Hip()
    with _engine(impl, {"col_slices": "2", "light": "0", "carry_combine": "1"}, True) as eng:
        eng.load_matrix_csr(_csr(m, a))
        st = eng.stats()
        assert st["col_slices"] == 2 and st["stream_bytes"] < (160 << 20)
        xw = host.pack_vector(impl, cases.random_x(eng.num_cols, 7, impl))
        eng.load_vector(xw)
        db = hip.put(b)
        outs = [hip.zeros(eng.num_rows * 4) for _ in range(3)]
        eng.run(); eng.push_result([outs[0]], eng.num_rows)
        eng.run()                                              # owed: its combine pass
        eng.update_values_device(db, m.nnz)
        eng.push_result([outs[1]], eng.num_rows)               # the second step's y: old values
        eng.run(); eng.run()
        eng.push_result([outs[2]], eng.num_rows)
        eng.sync()
        ys = [hip.get(o, eng.num_rows) for o in outs]
    hip.close()
    want_a, want_b = _oracle(m, a, impl, xw), _oracle(m, b, impl, xw)
    assert _same_y(impl, ys[0], want_a) and _same_y(impl, ys[1], want_a) and _same_y(impl, ys[2], want_b)


# ---- (e) refusals -------------------------------------------------------------------------------------------------------------------
def _usable(eng, m, values, impl):
    xw = host.pack_vector(impl, cases.random_x(eng.num_cols, 11, impl))
    eng.load_vector(xw)
    eng.run()
    assert _same_y(impl, eng.read_result(), _oracle(m, values, impl, xw))


def _rc(eng, values, nnz=None, device_ptr=None):
    lib = device.lib()
    if device_ptr is not None:
        return lib.hs_update_values_device(eng._h, C.c_void_p(device_ptr or None), nnz)
    values = np.ascontiguousarray(values, dtype=np.float32)
    return lib.hs_update_values(eng._h, values.ctypes.data, values.size if nnz is None else nnz)


@pytest.mark.parametrize("impl", [0, 1])
def test_refusals_leave_the_context_usable(impl):
    m = cases.random_csr(2000, 3000, 0.01, 51, impl)
    a, b = m.data.astype(np.float32), _finite_values(m.nnz, impl, 12)
    with _engine(impl, {}, False) as eng:
        assert _rc(eng, b) == -5                                             # before any load
        eng.load_matrix_csr(_csr(m, a))
        assert _rc(eng, b) == -6 and b"option" in device.lib().hs_last_error(eng._h)      # option off
        _usable(eng, m, a, impl)
    with _engine(impl, {}, True) as eng:                                    # CPSR load
        cp = host.format_matrix(host.CSRMatrix.from_arrays(*_csr(m, a)), impl, skip_empty_rows=True)
        eng.load_matrix(cp)
        assert _rc(eng, b) == -6 and b"CPSR" in device.lib().hs_last_error(eng._h)
        _usable(eng, m, a, impl)
    ip = np.array([0, 3] + [4] * 127, dtype=np.uint32)                      # (0, 5) twice: formatted on the host
    dup = (128, 16, ip, np.array([5, 5, 1, 2], dtype=np.uint32), np.array([1.0, 2.0, 0.5, 0.25], dtype=np.float32))
    with _engine(impl, {}, True) as eng:
        eng.load_matrix_csr(dup)
        assert not eng.stats()["retiled_on_gpu"]
        assert _rc(eng, np.ones(4, np.float32)) == -6 and b"host builder" in device.lib().hs_last_error(eng._h)
    with _engine(impl, {"stream_format": "bitmap", "bitmap_build": "host"}, True) as eng:
        mb = _matrix("bitmap", impl, seed=52)
        eng.load_matrix_csr(_csr(mb, mb.data))
        assert _rc(eng, mb.data) == -6
        _usable(eng, mb, mb.data, impl)
    with _engine(impl, {}, True) as eng:
        eng.load_matrix_csr(_csr(m, a))
        assert _rc(eng, b, nnz=m.nnz - 1) == -1 and _rc(eng, b, nnz=m.nnz + 1) == -1         # wrong count
        assert device.lib().hs_update_values(eng._h, None, m.nnz) == -1                      # null
        hip = _Hip()
        db = hip.put(np.concatenate([[0.0], b]).astype(np.float32))
        assert _rc(eng, None, nnz=m.nnz, device_ptr=0) == -1                                 # null device pointer
        assert _rc(eng, None, nnz=m.nnz, device_ptr=db + 2) == -1                            # misaligned
        _usable(eng, m, a, impl)
        assert _rc(eng, None, nnz=m.nnz, device_ptr=db + 4) == 0                             # 4-byte aligned: the one-value-per-lane kernel
        _usable(eng, m, b, impl)
        hip.close()
        eng.set_option("value_map", "0")
        eng.load_matrix_csr(_csr(m, a))                                                      # a reload with the option off drops the map
        assert _rc(eng, b) == -6
        _usable(eng, m, a, impl)


# ---- (f) memory ---------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    device.lib()
    rt = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert rt.hipDeviceSynchronize() == 0
    assert rt.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _load_cost(impl, opts, m, value_map):
    eng = _engine(impl, opts, value_map)
    before = _free_bytes()
    eng.load_matrix_csr(_csr(m, m.data))
    cost = before - _free_bytes()
    mfma = eng.read_mfma_image().size > 0
    eng.close()
    return cost, mfma


@pytest.mark.parametrize("impl,plan", [(0, "planner"), (1, "bitmap"), (0, "sweep")])
def test_map_costs_four_bytes_per_non_zero(impl, plan):
    # hipMemGetInfo counts the whole device, which other processes share: the median of five alternating pairs of loads
    m = cases.random_csr(800, 40000, 0.12, 61, impl) if plan == "bitmap" else cases.random_csr(20000, 30000, 0.004, 61, impl)
    diffs, mfma = [], False
    for _ in range(5):
        off, _ = _load_cost(impl, PLANS[plan], m, False)
        on, mfma = _load_cost(impl, PLANS[plan], m, True)
        diffs.append(on - off)
    want = (8 if mfma else 4) * m.nnz
    assert plan != "bitmap" or mfma
    got = sorted(diffs)[2]
    tol = (2 << 20) * (2 if mfma else 1)          # the device allocates in 2 MiB pages: +- 2 MiB per map
    assert abs(got - want) <= tol, f"map cost {got} bytes (pairs: {diffs}), expected {want} (+- {tol >> 20} MiB)"


def test_load_update_reload_cycles_give_memory_back():
    m = cases.random_csr(20000, 30000, 0.004, 62, 1)
    b = _finite_values(m.nnz, 1, 13)
    hip = _Hip()
    db = hip.put(b)
    before = _free_bytes()
    for _ in range(4):
        with _engine(1, {}, True) as eng:
            eng.load_matrix_csr(_csr(m, m.data))
            eng.update_values(b)
            eng.update_values_device(db, m.nnz)
            eng.sync()
            eng.load_matrix_csr(_csr(m, b))
            eng.update_values(m.data)
            eng.set_option("stream_format", "bitmap")
            eng.load_matrix_csr(_csr(m, m.data))
            eng.update_values(b)
    assert before - _free_bytes() <= (64 << 20)
    hip.close()


# ---- (g) seeded fuzz -----------------------------------------------------------------------------------------------------------------
FUZZ_PLANS = ["pairs", "pairs24", "delta", "owner", "owner24", "sweep", "bitmap", "light", "slices2", "planner"]


def test_seeded_fuzz_byte_identity():
    rng = np.random.default_rng(20261015)
    failures = []
    hip = _Hip()
    for case in range(150):
        impl = int(rng.integers(0, 3))
        plan = FUZZ_PLANS[int(rng.integers(0, len(FUZZ_PLANS)))]
        rows, cols = int(rng.integers(64, 6000)), int(rng.integers(8, 30000))
        density = float(min(0.3, 10 ** rng.uniform(-3.5, -0.7)))
        if plan == "bitmap":
            rows, density = min(rows, 2000), max(density, 0.02)
        density = min(density, 4e5 / (rows * cols))             # at most ~400 K non-zeros a case
        m = cases.random_csr(rows, cols, density, 1000 + case, impl)
        if m.nnz == 0:
            continue
        with _engine(impl, PLANS[plan], True) as eng, _engine(impl, PLANS[plan], False) as ref:
            eng.load_matrix_csr(_csr(m, m.data))
            for u in range(3):
                vals = _hard_values(m.nnz, impl, case * 10 + u)
                if u % 2 == 0:
                    eng.update_values(vals)
                else:
                    eng.update_values_device(hip.put(vals), m.nnz)
                    eng.sync()
                ref.load_matrix_csr(_csr(m, vals))
                if _snapshot(eng) != _snapshot(ref):
                    failures.append((case, impl, plan, rows, cols, density, u))
        hip.close()
    assert not failures, failures[:10]


# ---- (h) full size ---------------------------------------------------------------------------------------------------------------------
def test_ogbl_ppa_full_size_update_is_bit_exact():
    cfg, csr = datasets.load("ogbl_ppa")
    impl = host.impl_id(cfg.impl)
    ip, ix, dv = csr.arrays()
    new = np.random.default_rng(77).uniform(0.0, 2.0, dv.size).astype(np.float32)
    with _engine(impl, {}, True) as eng:
        eng.load_matrix_csr(csr)
        eng.update_values(new)
        xw = host.pack_vector(impl, np.random.default_rng(78).uniform(0.0, 2.0, eng.num_cols).astype(np.float32))
        eng.load_vector(xw)
        eng.run()
        got = eng.read_result()
    cp = host.format_matrix(host.CSRMatrix.from_arrays(csr.num_rows, csr.num_cols, ip, ix, new), impl, skip_empty_rows=cfg.skip_empty_rows)
    want = orc.spmv(impl, [cp.channel_ptr(c)[0] for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                    cp.ob_bank, cp.vb_bank)
    assert np.array_equal(got, want)


# ---- (i) speed sanity -------------------------------------------------------------------------------------------------------------------
def test_device_update_is_a_small_fraction_of_a_reload():
    cfg, csr = datasets.load("ogbl_ppa", scale=0.25)
    ip, ix, dv = csr.arrays()
    assert 5e6 < dv.size < 2e7
    with _engine(0, {}, True) as eng:
        eng.load_matrix_csr(csr)
        eng.load_matrix_csr(csr)                                  # the reload: the second load in the process
        reload_s = eng.stats()["load_seconds"]
        hip = _Hip()
        dvals = hip.put(dv)
        for _ in range(3):
            eng.update_values_device(dvals, dv.size)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(20):
            eng.update_values_device(dvals, dv.size)
        eng.sync()
        update_s = (time.perf_counter() - t0) / 20
        hip.close()
    assert update_s < reload_s / 10, f"update {update_s * 1e3:.3f} ms against a reload of {reload_s * 1e3:.1f} ms"
