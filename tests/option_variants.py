"""The plan-time options of hs_set_option as one table of named variants (a test helper, like cases.py): what to set, what to compare
the resulting image with, in which numeric modes, on which matrix, and which rounding class of tests/float_contract.py bounds it.

tests/test_option_matrix_cpu.py builds every variant with the host builder and walks it with the emulated kernel;
tests/test_gpu_option_matrix.py loads it on the device.  A key of kOptionKeys (hs_api.cpp) that is not in this table must be named in
COVERED_ELSEWHERE, with the test file that exercises it: the ratchet of the CPU file checks both.  tools/tiles_ab.py lists many of the
same switches for its byte comparison of two host builds: keep the two lists in step.

The shapes are the smallest at which each layout was seen to change at 256 workgroups (the CPU file asserts that it does).
"""
import contextlib
import os
from collections import namedtuple

import numpy as np

from hisparse_amd import device, host
from oracle import oracle as orc

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKGROUPS = 256          # the compute units of the device the table is sized for

# options / base: {key: value} as hs_set_option takes them (lower case, no prefix); impls: numeric modes; matrix: a key of MATRICES;
# chain: the float_contract.chain variant name.  (No variant's image is built by the host code on the device path: that happens for
# duplicate entries, bitmap_build = host, retile = host and SWEEP chunks wider than 65535 columns -- tests/test_gpu_retile.py.)
Variant = namedtuple("Variant", "name options base impls matrix chain")

ALL, FLOAT = (0, 1, 2), (1, 2)


def _v(name, options, base, matrix, chain, impls=ALL):
    return Variant(name, dict(options), dict(base), tuple(impls), matrix, chain)


def _with(base, **more):
    d = dict(base)
    d.update({k: str(v) for k, v in more.items()})
    return d


SKEWS = ("100/100/100/100", "9999/1/1/1", "1/9999/1/1", "1/1/1/9999")


def _table():
    t = []
    # ---- the graph matrix: 3000 x 20000 at 1 %, three x sub-tiles, default banks --------------------------------------------------
    delta = {"stream_format": "delta", "light": "0"}
    for tag, more, chain in (("", {"col_slices": 1}, "delta"), ("-row-runs-1", {"col_slices": 1, "row_runs": 1}, "delta-lane-sums"),
                             ("-row-runs-0", {"col_slices": 1, "row_runs": 0}, "delta-no-lane-sums"), ("-3-slices", {"col_slices": 3}, "delta")):
        base = _with(delta, **more)
        t.append(_v("delta-deal-wave" + tag, _with(base, delta_deal="wave"), base, "graph", chain))
    for fmt in ("pairs", "delta"):
        base = {"stream_format": fmt, "light": "0", "col_slices": "4"}
        t.append(_v(f"xcd-affinity-{fmt}", _with(base, xcd_affinity=1), base, "graph", fmt))
    # (3000 rows over 256 workgroups are blocks of a few dozen rows, which max_rows = 100 does not cut, and 600 K non-zeros are fewer LIGHT blocks
    # than four per workgroup: these run on the taller matrix -- 156 rows per workgroup, 1.3 M non-zeros)
    for fmt in ("pairs", "delta", "sweep"):
        base = {"stream_format": fmt, "light": "0", "col_slices": "1"}
        t.append(_v(f"max-rows-100-{fmt}", _with(base, max_rows=100), base, "graph-tall", fmt))
    light = {"stream_format": "pairs", "light": "1"}
    for n, matrix in ((1, "graph"), (2, "graph"), (6, "graph-tall")):
        t.append(_v(f"light-wgs-{n}", _with(light, light_wgs=n), light, matrix, "light"))
    # ... with small output banks: several row partitions
    for fmt in ("pairs", "delta", "owner24", "sweep"):
        base = {"stream_format": fmt, "light": "0"}
        t.append(_v(f"cross-partitions-0-{fmt}", _with(base, cross_partitions=0), base, "graph-parts", fmt))
    # ---- dense rows: forced BITMAP, the share of a block each wavefront gets --------------------------------------------------------
    bitmap = {"stream_format": "bitmap"}
    # (300 dense rows over 256 workgroups are blocks of one or two rows, every row cut into pieces; the thin matrix -- 0.6 % -- has so few
    # non-zeros that a block holds some forty rows and its wavefronts get whole rows)
    for matrix, tag, more in (("dense-300", "300-rows", {}), ("dense-5", "5-rows", {}), ("dense-300", "300-rows-2-slices", {"col_slices": 2}),
                              ("dense-300", "300-rows-max-rows-3", {"max_rows": 3}), ("thin-300", "300-thin-rows", {})):
        base = _with(bitmap, **more)
        for skew in SKEWS:
            t.append(_v(f"bitmap-skew-{skew.replace('/', '-')}-{tag}", _with(base, bitmap_skew=skew), base, matrix, "bitmap"))
    t.append(_v("max-rows-3-bitmap", _with(bitmap, max_rows=3), bitmap, "dense-300", "bitmap"))
    # ---- the matrix engine's image (float modes) -------------------------------------------------------------------------------------
    for matrix, tag in (("mfma-300", "300-rows"), ("mfma-17", "17-rows")):
        for n in (1, 47, 1000):
            t.append(_v(f"mfma-chunk-{n}-{tag}", _with(bitmap, mfma_chunk=n), bitmap, matrix, "bitmap", FLOAT))
        t.append(_v(f"no-mfma-image-{tag}", _with(bitmap, no_mfma_image=1), bitmap, matrix, "bitmap", FLOAT))
    # ---- slice rules -------------------------------------------------------------------------------------------------------------------
    # (These two only choose a slice COUNT; the sliced float kernels run under the 3- and 4-slice variants above.  Fixed point and float_pob:
    # float_stall plans from the same rules, and the 4 M non-zero banded matrix is the largest of the table.)
    for fmt in ("pairs", "delta"):
        base = {"stream_format": fmt, "light": "0"}
        t.append(_v(f"pow2-slices-{fmt}", _with(base, pow2_slices=1), base, "powerlaw-wide", fmt, (0, 1)))
    t.append(_v("plan-census-0", {"plan_census": "0"}, {}, "banded", "delta", (0, 1)))
    return t


VARIANTS = _table()
BY_NAME = {v.name: v for v in VARIANTS}
assert len(BY_NAME) == len(VARIANTS)

# every other key of kOptionKeys: the test file that sets it (the CPU ratchet checks that the file mentions the key)
COVERED_ELSEWHERE = {
    "STREAM_FORMAT": "tests/test_gpu_parity.py",
    "COL_SLICES": "tests/test_gpu_parity.py",
    "SPMM_VECTORS": "tests/test_gpu_float_contract.py",
    "ROW_RUNS": "tests/test_gpu_parity.py",
    "AUX_BITS": "tests/test_gpu_parity.py",
    "STREAM_RESIDENT": "tests/test_gpu_options.py",
    "RETILE": "tests/test_gpu_retile.py",
    "PLAN_DEBUG": "tests/test_tiles_cpu.py",
    "BITMAP_X_LDS": "tests/test_gpu_bitmap.py",
    "BITMAP_BUILD": "tests/test_gpu_retile.py",
    "WALK_LANES": "tests/test_tiles_cpu.py",
    "LIGHT": "tests/test_gpu_parity.py",
    "SWEEP": "tests/test_gpu_sweep.py",
    "SPMM_FUSED": "tests/test_gpu_float_contract.py",
    "SPMM_MFMA": "tests/test_gpu_float_contract.py",
    "SPMSPV": "tests/test_spmspv.py",
    "SPMSPV_CROSSOVER": "tests/test_spmspv.py",
    "ITERATE_GRAPH": "tests/test_gpu_parity.py",
    "BATCH_GRAPH": "tests/test_gpu_options.py",
    "CARRY_COMBINE": "tests/test_gpu_carry.py",
    "AUTOTUNE": "tests/test_gpu_planner.py",
    "VALUE_MAP": "tests/test_gpu_value_update.py",
}


def table_keys():
    """the option keys (upper case) some variant sets beyond its base"""
    return {k.upper() for v in VARIANTS for k in v.options if v.options.get(k) != v.base.get(k)}


def option_keys():
    """the string literals of kOptionKeys in hs_api.cpp"""
    import re
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "hs_api.cpp")).read()
    body = re.search(r"kOptionKeys\[\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    return re.findall(r'"([A-Z0-9_]+)"', body)


@contextlib.contextmanager
def environment(options):
    """HISPARSE_<KEY> for the host builder (hs_tiles_build has no context: it reads the environment); every key of kOptionKeys is cleared first
    and the environment restored afterwards"""
    keys = ["HISPARSE_" + k for k in option_keys()]
    saved = {k: os.environ.pop(k) for k in keys if k in os.environ}
    try:
        for k, val in options.items():
            os.environ["HISPARSE_" + k.upper()] = str(val)
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(saved)


# ---- matrices: (scipy CSR, vb_bank, ob_bank) per numeric mode ----------------------------------------------------------------------------

def _banks(impl):
    return host.default_banks(impl)


_GRAPH = {}


def _graph(impl):
    if impl not in _GRAPH:      # (scipy.sparse.random takes seconds at this shape: once per mode, for both bank settings)
        _GRAPH[impl] = cases.random_csr(3000, 20000, 0.01, 61, impl)
    v, o = _banks(impl)
    return _GRAPH[impl], v, o


def _graph_parts(impl):
    v, _ = _banks(impl)
    return _graph(impl)[0], v, 8 if impl == 2 else 2


def _graph_tall(impl):
    v, o = _banks(impl)
    return _scipy(host.CSRMatrix.generate("powerlaw", 40000, 20000, a=1.3e6, b=0.3, seed=66), impl), v, o


def _dense(rows, cols, density, seed):
    def make(impl):
        m = cases.random_csr(rows, cols, density, seed, impl)
        if impl != 0:
            m.data *= np.float32(0.05)      # pruned-NN weights, as tests/test_gpu_parity.py test_dense_rows_pick_bitmap scales them
        v, o = _banks(impl)
        return m, v, o
    return make


def _scipy(csr, impl):
    import scipy.sparse as sp
    ip, ix, dv = csr.arrays()
    if impl != 0:
        dv = (dv - np.float32(1.0)).astype(np.float32)
    return sp.csr_matrix((dv, ix.astype(np.int64), ip.astype(np.int64)), shape=(csr.num_rows, csr.num_cols))


def _powerlaw_wide(impl):
    v, o = _banks(impl)
    return _scipy(host.CSRMatrix.generate("powerlaw", 20000, 140000, a=1.2e6, b=0.4, seed=19), impl), v, o


_TOOLS = {}


def _planner_check():
    """tools/planner_check.py, loaded once by its path (nothing is added to sys.path for it)"""
    if "pc" not in _TOOLS:
        import importlib.util
        spec = importlib.util.spec_from_file_location("planner_check", os.path.join(ROOT, "tools", "planner_check.py"))
        _TOOLS["pc"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_TOOLS["pc"])
    return _TOOLS["pc"]


def _banded(impl):
    # the matrix of tests/test_planner_cpu.py test_banded_and_block_diagonal_matrices_are_not_sliced: one slice with the census, several
    # without (a uniform matrix gets the same plan either way)
    v, o = _banks(impl)
    return _planner_check().banded(200_000, 20, 1_000, 1, impl), v, o


MATRICES = {
    "graph": _graph, "graph-parts": _graph_parts, "graph-tall": _graph_tall,
    "dense-300": _dense(300, 5000, 0.3, 62), "dense-5": _dense(5, 5000, 0.5, 63),
    "thin-300": _dense(300, 5000, 0.006, 67), "mfma-300": _dense(300, 9000, 0.2, 64), "mfma-17": _dense(17, 3000, 0.5, 65),
    "powerlaw-wide": _powerlaw_wide, "banded": _banded,
}

Case = namedtuple("Case", "m cp x xw want")
_CASES = {}


def case(matrix, impl):
    """(scipy matrix, formatted packets, x, packed x, the oracle's y), made once per (matrix, mode) and shared: treat as read-only"""
    key = (matrix, impl)
    if key not in _CASES:
        m, vb, ob = MATRICES[matrix](impl)
        _, cp = cases.formatted(m, impl, vb, ob, True)
        x = cases.random_x(cp.num_cols, 60, impl)
        xw = host.pack_vector(impl, x)
        want = orc.spmv(impl, [cp.channel(c) for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                        cp.ob_bank, cp.vb_bank)
        for a in (x, xw, want):
            a.setflags(write=False)
        _CASES[key] = Case(m, cp, x, xw, want)
    return _CASES[key]


_REFERENCES = {}


def reference(matrix, impl):
    """float_contract.Reference of a float case (float64 facts per row), made once"""
    import float_contract as fc
    key = (matrix, impl)
    if key not in _REFERENCES:
        c = case(matrix, impl)
        _REFERENCES[key] = fc.Reference(c.m, c.x, c.cp.num_rows)
    return _REFERENCES[key]


_BUILDS = {}


def build(options, matrix, impl, workgroups=WORKGROUPS):
    """the host builder's tiles of a matrix of the table under `options` (cached: the base of one variant is the base of others)"""
    key = (tuple(sorted(options.items())), matrix, impl, workgroups)
    if key not in _BUILDS:
        cp = case(matrix, impl).cp
        with environment(options):
            _BUILDS[key] = device.build_tiles(cp, impl, cp.ob_bank, cp.vb_bank, cp.num_rows, cp.num_cols, cp.num_row_partitions,
                                              cp.num_col_partitions, workgroups)
    return _BUILDS[key]


def same_tiles(a, b):
    """image, Block[], Unit[] and the matrix engine's image of two builds, byte for byte"""
    return (a["image"].tobytes() == b["image"].tobytes() and a["blocks"].tobytes() == b["blocks"].tobytes()
            and a["units"].tobytes() == b["units"].tobytes() and a["mfma"].tobytes() == b["mfma"].tobytes())


def params():
    """(variant name, impl) of every case, for pytest.mark.parametrize"""
    return [(v.name, impl) for v in VARIANTS for impl in v.impls]
