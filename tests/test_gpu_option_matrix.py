"""Every plan-time option of hs_set_option on the device: the table of tests/option_variants.py (its host-side counterpart is
tests/test_option_matrix_cpu.py), set per context with hs_set_option -- the device loads of this file run with no HISPARSE_ variable in the
environment (one test sets one on purpose: the refusal of a value that arrives that way).

Per variant and numeric mode: the image the device builds (from CPSR packets and from CSR arrays) is the host builder's, byte for byte, and
the stats show the option at work; hs_run (twice, and in a burst with the carried combine), hs_run_batch and the hs_run_partition loop give
the oracle's y -- bit for bit in fixed point, within 1e-4 and within the float64 bound of the path's rounding class (float_contract.py) in
the float modes, there also on a designed matrix of the same shape family whose data can tell a wrong summation; the accumulator border in
fixed point; hs_spmm over the matrix engine's image at every mfma_chunk, without that image, over skewed BITMAP runs and over a SWEEP image
of short blocks; hs_update_values through the value maps of these layouts; and four host threads loading under different options at once.
"""
import threading

import numpy as np
import pytest

from hisparse_amd import device, host
from oracle import oracle as orc

import cases
import float_contract as fc
import option_variants as ov
from test_gpu_float_contract import _teeth
from test_gpu_saturation import _setup as _saturation_setup
from test_gpu_value_update import _csr, _hard_values, _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for k in ov.option_keys():
        monkeypatch.delenv("HISPARSE_" + k, raising=False)


def _engine(impl, cp, options, **more):
    eng = device.SpmvEngine(impl, ob_bank=cp.ob_bank, vb_bank=cp.vb_bank)
    for k, val in {**options, **more}.items():
        eng.set_option(k, val)
    return eng


def _oracle(cp, impl, xw):
    return orc.spmv(impl, [cp.channel(c) for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                    cp.ob_bank, cp.vb_bank)


def _assert_options_took_effect(v, st, want):
    assert device.STREAM_FORMATS[st["stream_format"]] == want["format"]
    if "stream_format" in v.options:
        assert want["format"] == v.options["stream_format"]
    assert st["col_slices"] == want["col_slices"] and st["num_blocks"] == want["blocks"].size and st["num_units"] == want["units"].size
    assert st["num_workgroups"] == want["num_workgroups"] and st["stream_bytes"] == want["image"].size
    assert st["stream_elements"] == want["elements"] and st["nnz"] == want["nnz"]
    assert st["light_kernel"] == (1 if v.options.get("light") == "1" else 0)
    if "col_slices" in v.options:
        assert st["col_slices"] == int(v.options["col_slices"])
    if "light_wgs" in v.options:
        assert st["num_blocks"] <= st["num_compute_units"] * int(v.options["light_wgs"])


# ---- the image the device builds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,impl", ov.params())
def test_device_image_is_the_host_builders(name, impl):
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp = c.cp
    want = None
    for loader in ("hs_load_matrix", "hs_load_matrix_csr"):
        with _engine(impl, cp, v.options) as eng:
            if loader == "hs_load_matrix":
                eng.load_matrix(cp)
            else:
                eng.load_matrix_csr(_csr(c.m, c.m.data))
                assert (eng.num_rows, eng.num_cols) == (cp.num_rows, cp.num_cols)
            st = eng.stats()
            got = eng.read_tiles()
            got_mfma = eng.read_mfma_image()
        if want is None:
            want = ov.build(v.options, v.matrix, impl, st["num_compute_units"])
            base = ov.build(v.base, v.matrix, impl, st["num_compute_units"])
            assert not ov.same_tiles(want, base), "the option changes nothing at this device's workgroup count"
        assert st["retiled_on_gpu"] == 1, loader      # (no variant of the table is one the builder hands to the host code)
        _assert_options_took_effect(v, st, want)
        assert got["blocks"].tobytes() == want["blocks"].tobytes(), f"{loader}: Block[] differs"
        assert got["units"].tobytes() == want["units"].tobytes(), f"{loader}: Unit[] differs"
        if not np.array_equal(got["image"], want["image"]):
            bad = np.nonzero(got["image"] != want["image"])[0]
            raise AssertionError(f"{loader}: image differs at {bad.size} of {want['image'].size} bytes, first at {bad[:8]}")
        assert got_mfma.tobytes() == want["mfma"].tobytes(), f"{loader}: matrix-engine image differs"


# ---- the kernels over it -----------------------------------------------------------------------------------------------------------------
def _entry_points(eng, cp, xw, sliced, reverse):
    """y through every SpMV entry point of a loaded context: {what: packed y}"""
    outs = {}
    eng.load_vector(xw)
    eng.run()
    outs["run"] = eng.read_result()
    eng.run()
    outs["run again"] = eng.read_result()
    if sliced:
        for _ in range(3):      # back to back: the combine of each step but the last is carried into the next step's kernel
            eng.run()
        outs["burst of three"] = eng.read_result()
    eng.run_batch(3)
    outs["batch"] = eng.read_result()
    orders = [("partitions", range(cp.num_row_partitions))]
    if reverse:
        orders.append(("partitions in reverse", reversed(range(cp.num_row_partitions))))
    for what, order in orders:
        eng.load_matrix(cp)      # (y zeroed) the reference's launch loop, one row partition at a time
        eng.load_vector(xw)
        for j in order:
            eng.run_partition(j, cp.part_len(j))
        outs[what] = eng.read_result()
    return outs


# designed matrices (float_contract.designed) per shape family: rows, columns, hub rows, their length
DESIGNED = {
    "graph": (1100, 20000, 3, 12000), "graph-parts": (1100, 20000, 3, 12000), "graph-tall": (1100, 20000, 3, 12000),
    "dense-300": (300, 5000, 2, 3000), "thin-300": (300, 5000, 2, 3000), "dense-5": (22, 5000, 2, 3000),
    "mfma-300": (300, 9000, 2, 6000), "mfma-17": (66, 3000, 2, 2000),
}
_DESIGNED = {}


def _designed(matrix, impl):
    """(m, cp, xw, kinds, ref, the oracle's y) of the family's designed matrix, with the family's banks; made once"""
    key = (matrix, impl)
    if key not in _DESIGNED:
        rows, cols, hubs, hub_len = DESIGNED[matrix]
        m, x, kinds = fc.designed(rows, cols, 70 + impl + rows, hubs=hubs, hub_len=hub_len)
        base = ov.case(matrix, impl).cp
        _, cp = cases.formatted(m, impl, base.vb_bank, base.ob_bank, True)
        xp = np.zeros(cp.num_cols, dtype=np.float32)
        xp[: x.size] = x
        xw = host.pack_vector(impl, xp)
        _DESIGNED[key] = (m, cp, xw, kinds, fc.Reference(m, xp, cp.num_rows), _oracle(cp, impl, xw))
    return _DESIGNED[key]


@pytest.mark.parametrize("name,impl", ov.params())
def test_kernels_give_the_oracles_y(name, impl):
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp = c.cp
    reverse = v.options.get("cross_partitions") == "0"
    with _engine(impl, cp, v.options, carry_combine="1") as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        tiles = eng.read_tiles()
        outs = _entry_points(eng, cp, c.xw, st["col_slices"] > 1, reverse)
    assert device.STREAM_FORMATS[st["stream_format"]] == v.options.get("stream_format", device.STREAM_FORMATS[st["stream_format"]])
    assert st["light_kernel"] == (1 if v.options.get("light") == "1" else 0)
    if reverse:
        assert cp.num_row_partitions > 1 and (tiles["blocks"]["last_part"] == tiles["blocks"]["row_part"]).all()
    S = int(st["col_slices"])
    for what, y in outs.items():
        if impl == 0:
            assert np.array_equal(y, c.want), (name, what, np.nonzero(y != c.want)[0][:8], y[y != c.want][:8])
        else:
            assert cases.float_close(y, c.want), (name, what)
            ov.reference(v.matrix, impl).check(y, L=fc.chain(v.chain, c.m, tiles), slices=S, what=f"{name} {what}")
    if impl == 0 or v.matrix not in DESIGNED:
        return
    # float: a designed matrix of the same shape family -- twelve binades, cancelling rows, hub rows -- under the same options
    m, dcp, xw, kinds, ref, want = _designed(v.matrix, impl)
    _teeth(ref, kinds, want)
    with _engine(impl, dcp, v.options, carry_combine="1") as eng:
        eng.load_matrix(dcp)
        st = eng.stats()
        tiles = eng.read_tiles()
        outs = _entry_points(eng, dcp, xw, st["col_slices"] > 1, reverse)
    assert device.STREAM_FORMATS[st["stream_format"]] == v.options["stream_format"]
    L, S = fc.chain(v.chain, m, tiles), int(st["col_slices"])
    for what, y in outs.items():      # (not against the oracle: its fp32 running sum is what _teeth shows to break the bound here)
        ref.check(y, L=L, slices=S, what=f"{name} designed S={S} {what}")
        assert (y[kinds["empty"]] == 0).all() and (y[m.shape[0]:] == 0).all(), what      # empty and padded rows: exactly +0.0


def _distinct(prefixes):
    """one variant per distinct option set among the variants whose names begin with one of `prefixes` (fixed point is one of its modes)"""
    seen, out = set(), []
    for v in ov.VARIANTS:
        key = tuple(sorted(v.options.items()))
        if v.name.startswith(prefixes) and 0 in v.impls and key not in seen:
            seen.add(key)
            out.append(v.name)
    return out


_BORDER = {}


def _border_case(tall):
    """(cp, xw, expected y) of the matrix of tests/test_gpu_saturation.py.  tall: the same 700 rows on top of 11000 bulk rows (1.1 M more
    non-zeros, values exact in Q8.24) -- the 56 K non-zeros of the matrix alone are 54 LIGHT blocks whatever light_wgs says, so the
    light-wgs variants would lay it out like the default plan and show nothing; the border rows and their expected words are the same."""
    if tall not in _BORDER:
        m, cp, x, xw, want = _saturation_setup()
        if tall:
            import scipy.sparse as sp
            rng = np.random.default_rng(10)
            ip, ix, _ = host.CSRMatrix.generate("powerlaw", 11000, m.shape[1], a=1.15e6, b=0.2, c=1.0, seed=10).arrays()
            dv = (np.round(rng.uniform(0.0, 2.0, ix.size) * 2 ** 20) / 2 ** 20).astype(np.float32)
            bulk = sp.csr_matrix((dv, ix.astype(np.int64), ip.astype(np.int64)), shape=(11000, m.shape[1]))
            tall_m = sp.vstack([m, bulk]).tocsr()
            _, tcp = cases.formatted(tall_m, 0, cp.vb_bank, cp.ob_bank, True)
            assert tcp.num_cols == cp.num_cols
            twant = _oracle(tcp, 0, xw)
            assert np.array_equal(twant[: m.shape[0]], want[: m.shape[0]])      # the border rows: the Python-integer words of _setup
            cp, want = tcp, twant
        want.setflags(write=False)
        _BORDER[tall] = (cp, xw, want)
    return _BORDER[tall]


@pytest.mark.parametrize("name", _distinct(("delta-deal-wave", "bitmap-skew", "light-wgs")))
def test_accumulator_border_does_not_depend_on_who_sums_the_row(name):
    """Fixed point over the matrix of tests/test_gpu_saturation.py: rows that end at 0xFFFFFFFE, at 0xFFFFFFFF, one product past it, and
    whose slices stay below 2^32 while their total passes it -- whichever lane, wavefront or run the layout gives their elements to."""
    v = ov.BY_NAME[name]
    cp, xw, want = _border_case("light_wgs" in v.options)
    assert cp.num_row_partitions > 1
    with _engine(0, cp, v.options, carry_combine="1") as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        tiles = eng.read_tiles()
        assert device.STREAM_FORMATS[st["stream_format"]] == v.options["stream_format"]
        assert st["light_kernel"] == (1 if v.options.get("light") == "1" else 0)
        outs = _entry_points(eng, cp, xw, st["col_slices"] > 1, False)
    # the option lays THIS matrix out differently too: the same load without it
    with _engine(0, cp, v.base) as eng:
        eng.load_matrix(cp)
        base = eng.read_tiles()
    assert any(tiles[k].tobytes() != base[k].tobytes() for k in ("image", "blocks", "units")), "the option changes nothing on this matrix"
    for what, y in outs.items():
        assert np.array_equal(y, want), (name, st["col_slices"], what, np.nonzero(y != want)[0][:8], y[y != want][:8])


# ---- SpMM --------------------------------------------------------------------------------------------------------------------------------
_X = {}


def _activations(matrix, impl, k):
    """(k, num_cols) float32 activations (N(0, 1), as tests/test_spmm.py takes them) and their packed words, per case; made once"""
    key = (matrix, impl, k)
    if key not in _X:
        cp = ov.case(matrix, impl).cp
        Xf = np.stack([cases.random_x(cp.num_cols, 300 + j, impl) for j in range(k)])
        _X[key] = (Xf, np.stack([host.pack_vector(impl, Xf[j]) for j in range(k)]))
    return _X[key]


@pytest.mark.parametrize("name,impl", [(v.name, i) for v in ov.VARIANTS if "mfma_chunk" in v.options for i in v.impls])
def test_spmm_on_the_matrix_engine_at_every_chunk(name, impl):
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp, m = c.cp, c.m
    Xf, X = _activations(v.matrix, impl, 21)
    n = np.maximum(np.diff(m.indptr), 1)
    Xbad_f = Xf[:16].copy()
    Xbad_f[3, 70] = np.inf                              # reaches exactly the rows that hold the column: the exact fallback of spmm_finish_kernel,
    Xbad_f[5, 130] = np.nan                             # which walks the image unit by unit
    Xbad = np.stack([host.pack_vector(impl, Xbad_f[j]) for j in range(16)])
    with _engine(impl, cp, v.options) as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "bitmap" and eng.read_mfma_image().size > 0
        Y16 = eng.spmm(X[:16])
        Y21 = eng.spmm(X)
        Ybad = eng.spmm(Xbad)
        eng.set_option("spmm_mfma", "0")
        Y0 = eng.spmm(X)
    S = int(st["col_slices"])
    for j in range(21):
        if j < 16:      # the matrix engine: n FMAs of unrounded products from a zero accumulator, L = n + 1
            exact = fc.Reference(m, Xf[j], cp.num_rows, exact_products=True)
            exact.check(Y16[j], L=n + 1, what=f"{name} 16 columns, column {j}")
            exact.check(Y21[j], L=n + 1, what=f"{name} 21 columns, column {j}")
            assert cases.float_close(Y16[j], Y0[j], rtol=1e-5, atol=1e-5), f"{name}: column {j} of 16 against the vector-ALU path"
        else:           # the rest of the 21: four columns through the fused BITMAP kernel, one through the SpMV kernel -- batches of 8
            fc.Reference(m, Xf[j], cp.num_rows).check(Y21[j], L=8, slices=S, what=f"{name} 21 columns, column {j}")
        assert cases.float_close(Y21[j], _oracle(cp, impl, X[j])), (name, j)
        assert cases.float_close(Y21[j], Y0[j], rtol=1e-5, atol=1e-5), f"{name}: column {j} against the vector-ALU path"
    # a call with a non-finite word takes the exact path as a whole: every column is fp32 products summed in double (class D, written by
    # the finish kernel itself: no slices); inf and NaN reach exactly the rows that hold their column
    for j in range(16):
        ref = fc.Reference(m, Xbad_f[j], cp.num_rows)
        assert ref.finite.any() and ref.finite.all() == (j not in (3, 5))
        ref.check(Ybad[j], L=1, what=f"{name} non-finite call, column {j}")


@pytest.mark.parametrize("impl", [1, 2])
def test_spmm_with_a_chunk_beyond_the_row(impl):
    """mfma_chunk beyond the groups of a row, at its cap: the image of chunk = groups and, bit for bit, its answers"""
    c = ov.case("mfma-17", impl)
    cp, m = c.cp, c.m
    groups = (cp.num_cols + 63) // 64
    Xf, X = _activations("mfma-17", impl, 16)
    n = np.maximum(np.diff(m.indptr), 1)
    images, Y = {}, {}
    for chunk in (groups, 65536):
        with _engine(impl, cp, {"stream_format": "bitmap", "mfma_chunk": str(chunk)}) as eng:
            eng.load_matrix(cp)
            assert eng.stats()["retiled_on_gpu"] == 1
            images[chunk] = eng.read_mfma_image().tobytes()
            assert images[chunk] == images[groups] and len(images[chunk]) > 0      # (before any kernel runs over it)
            Y[chunk] = eng.spmm(X)
    for j in range(16):
        fc.Reference(m, Xf[j], cp.num_rows, exact_products=True).check(Y[65536][j], L=n + 1, what=f"column {j}")
        assert np.array_equal(Y[65536][j], Y[groups][j])


def test_a_chunk_the_kernel_cannot_take_is_refused(monkeypatch):
    """hs_set_option refuses what the matrix engine's kernel cannot take (tests/test_option_matrix_cpu.py says why) with HS_ERR_BAD_ARG and
    leaves the context as it was; the same value from the environment is refused by the load; fixed point never reads the switch."""
    c = ov.case("mfma-17", 1)
    cp = c.cp
    with _engine(1, cp, {"stream_format": "bitmap", "mfma_chunk": "7"}) as eng:
        for value in ("0", "-3", "65537", "1431655766", "2147483648", "99999999999999999999", "12x", "abc", " 5", "4.0"):
            with pytest.raises(device.DeviceError) as e:
                eng.set_option("mfma_chunk", value)
            assert e.value.code == -1 and "MFMA_CHUNK" in str(e.value), value
        eng.load_matrix(cp)                                   # the option it had stays in force
        want = ov.build({"stream_format": "bitmap", "mfma_chunk": "7"}, "mfma-17", 1, eng.stats()["num_compute_units"])
        assert eng.read_mfma_image().tobytes() == want["mfma"].tobytes() and want["mfma_chunk"] == 7
        eng.set_option("mfma_chunk", None)
        monkeypatch.setenv("HISPARSE_MFMA_CHUNK", "1431655766")
        with pytest.raises(device.DeviceError) as e:
            eng.load_matrix(cp)
        assert e.value.code == -1 and "MFMA_CHUNK" in str(e.value)
        with pytest.raises(device.DeviceError):
            eng.run()                                         # nothing is loaded after a refused load
        monkeypatch.delenv("HISPARSE_MFMA_CHUNK")
        eng.load_matrix(cp)
        eng.load_vector(c.xw)
        eng.run()
        assert cases.float_close(eng.read_result(), c.want)
    monkeypatch.setenv("HISPARSE_MFMA_CHUNK", "1431655766")
    c0 = ov.case("dense-5", 0)
    with _engine(0, c0.cp, {"stream_format": "bitmap"}) as eng:
        eng.load_matrix(c0.cp)
        eng.load_vector(c0.xw)
        eng.run()
        assert np.array_equal(eng.read_result(), c0.want)


@pytest.mark.parametrize("name,impl", [(v.name, i) for v in ov.VARIANTS if "no_mfma_image" in v.options for i in v.impls])
def test_spmm_without_the_matrix_engine_image(name, impl):
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp, m = c.cp, c.m
    Xf, X = _activations(v.matrix, impl, 16)
    with _engine(impl, cp, v.options) as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        assert device.STREAM_FORMATS[st["stream_format"]] == "bitmap"
        assert eng.read_mfma_image().size == 0
        Y = eng.spmm(X)
    with _engine(impl, cp, v.base) as eng:
        eng.load_matrix(cp)
        assert eng.read_mfma_image().size > 0
        eng.set_option("spmm_mfma", "0")
        Y0 = eng.spmm(X)
    for j in range(16):
        # the fused kernel's bound, not the matrix engine's
        fc.Reference(m, Xf[j], cp.num_rows).check(Y[j], L=8, slices=int(st["col_slices"]), what=f"{name} column {j}")
        assert np.array_equal(Y[j], Y0[j]), f"{name}: column {j} is not the fused kernel's answer"


@pytest.mark.parametrize("name,impl", [(v.name, i) for v in ov.VARIANTS if "bitmap_skew" in v.options for i in v.impls])
def test_spmm_over_skewed_bitmap_runs(name, impl):
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp = c.cp
    X = np.stack([host.pack_vector(impl, cases.random_x(cp.num_cols, 200 + j, impl)) for j in range(7)])      # 4 + 2 + 1
    with _engine(impl, cp, v.options) as eng:
        eng.load_matrix(cp)
        assert device.STREAM_FORMATS[eng.stats()["stream_format"]] == "bitmap"
        Y = eng.spmm(X)
        singles = []
        for j in range(7):
            eng.load_vector(X[j])
            eng.run()
            singles.append(eng.read_result())
    for j in range(7):
        want = _oracle(cp, impl, X[j])
        if impl == 0:
            assert np.array_equal(Y[j], singles[j]) and np.array_equal(Y[j], want), (name, j)
        else:
            assert cases.float_close(Y[j], singles[j], rtol=1e-5, atol=1e-5) and cases.float_close(Y[j], want), (name, j)


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_spmm_four_vectors_over_a_sweep_image_of_short_blocks(impl):
    v = ov.BY_NAME["max-rows-100-sweep"]
    c = ov.case(v.matrix, impl)
    cp = c.cp
    Xf = np.stack([cases.random_x(cp.num_cols, 400 + j, impl) for j in range(7)])
    X = np.stack([host.pack_vector(impl, Xf[j]) for j in range(7)])
    with _engine(impl, cp, v.options, spmm_vectors="4") as eng:
        eng.load_matrix(cp)
        st = eng.stats()
        tiles = eng.read_tiles()
        Y = eng.spmm(X)
    assert device.STREAM_FORMATS[st["stream_format"]] == "sweep" and tiles["blocks"]["nrows"].max() <= 100
    for j in range(7):
        want = _oracle(cp, impl, X[j])
        if impl == 0:
            assert np.array_equal(Y[j], want), (j, np.nonzero(Y[j] != want)[0][:8])
        else:
            assert cases.float_close(Y[j], want), j
            fc.Reference(c.m, Xf[j], cp.num_rows).check(Y[j], L=1, slices=int(st["col_slices"]), what=f"spmm_vectors=4 column {j}")


# ---- the value map -----------------------------------------------------------------------------------------------------------------------
VALUE_MAP_VARIANTS = ["delta-deal-wave", "delta-deal-wave-3-slices", "bitmap-skew-1-9999-1-1-300-rows", "bitmap-skew-1-1-1-9999-5-rows",
                      "mfma-chunk-47-300-rows", "light-wgs-6"]


@pytest.mark.parametrize("name,impl", [(n, i) for n in VALUE_MAP_VARIANTS for i in ov.BY_NAME[n].impls])
def test_update_values_gives_the_bytes_of_a_fresh_load(name, impl):
    """hs_update_values through the value map of each layout (float BITMAP: both maps -- the snapshot holds the matrix engine's image too)"""
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp, m = c.cp, c.m
    a = m.data.astype(np.float32)
    b = _hard_values(m.nnz, impl, 300 + impl)
    with _engine(impl, cp, v.options, value_map="1") as eng:
        eng.load_matrix_csr(_csr(m, a))
        first = _snapshot(eng)
        assert device.STREAM_FORMATS[first[0]["stream_format"]] == v.options["stream_format"] and first[0]["retiled_on_gpu"] == 1
        if impl and v.options["stream_format"] == "bitmap":
            assert first[4], "a float BITMAP matrix keeps the matrix-engine image"
        eng.update_values(b)
        updated = _snapshot(eng)
        eng.update_values(a)
        back = _snapshot(eng)
    with _engine(impl, cp, v.options, value_map="0") as eng:
        eng.load_matrix_csr(_csr(m, b))
        fresh = _snapshot(eng)
    for k, what in enumerate(("stats", "image", "Block[]", "Unit[]", "matrix-engine image")):
        assert updated[k] == fresh[k], f"{name}: {what} after the update differs from a fresh load of the new values"
    assert back == first, f"{name}: updating back does not give the first load's bytes"
    assert updated[1] != first[1]


# ---- options are per context, also from several host threads at once -----------------------------------------------------------------------
def test_contexts_of_four_threads_keep_their_own_options():
    """tiles_common.h: a context's options rule its own load, on whichever thread; loads of different contexts neither wait for each other
    nor see each other's options.  Four threads, four plans of the same matrix, three rounds at the same time: every context's stats and
    image are those of the same load done alone, every y the oracle's."""
    plans = {
        "pairs": {"stream_format": "pairs", "light": "0"},
        "delta+wave": {"stream_format": "delta", "light": "0", "delta_deal": "wave"},
        "bitmap+skew": {"stream_format": "bitmap", "bitmap_skew": "1/9999/1/1"},
        "sweep": {"stream_format": "sweep", "max_rows": "100"},
    }
    c = ov.case("graph", 0)
    cp = c.cp

    def load(options):
        with _engine(0, cp, options) as eng:
            eng.load_matrix(cp)
            snap = _snapshot(eng)
            eng.load_vector(c.xw)
            eng.run()
            return snap, eng.read_result()

    alone = {k: load(o) for k, o in plans.items()}
    images = [s[1] for s, _ in alone.values()]
    assert len(set(images)) == len(images)                               # four different layouts
    for k, (snap, y) in alone.items():
        assert device.STREAM_FORMATS[snap[0]["stream_format"]] == plans[k]["stream_format"]
        assert np.array_equal(y, c.want), k
    rounds = 3
    gate = threading.Barrier(len(plans))
    results, errors = {}, []

    def worker(k):
        try:
            for r in range(rounds):
                gate.wait(timeout=60)
                results[(k, r)] = load(plans[k])
        except BaseException as e:      # noqa: BLE001 -- reported by the main thread
            errors.append((k, e))
            gate.abort()

    threads = [threading.Thread(target=worker, args=(k,)) for k in plans]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads) and not errors, errors
    for k in plans:
        for r in range(rounds):
            snap, y = results[(k, r)]
            assert snap == alone[k][0], f"{k}, round {r}: not the stats and bytes of the same load done alone"
            assert np.array_equal(y, c.want), (k, r)
