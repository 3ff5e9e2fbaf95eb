"""hs_update_values without a GPU: the CPU backend refreshes a CSR-loaded matrix's values in place (checked against the oracle of the
new values), both symbols are exported by both libraries and by device.EXPORTS, the HIP library's argument checks answer without a device,
the update kernel in the shipped gfx950 code object is a plain streaming kernel (no scratch, no LDS, no memory-side atomics, no MFMA), and
the value-word conversion has exactly one device definition, shared by the load and the update."""
import ctypes
import os
import re
import subprocess
import sys


from hisparse_amd import device
from test_isa_invariants import shipped  # noqa: F401  (module fixture: the shipped code object's metadata + disassembly)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "hisparse_amd", "lib", "libhisparse_cpu.so")

CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from hisparse_amd import device, host
from oracle import oracle as orc
import cases

def oracle_y(cp, impl, xw):
    return orc.spmv(impl, [cp.channel(c) for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, cp.ob_bank, cp.vb_bank)

checked = 0
for impl in (0, 1, 2):
    for rows, cols, density in [(1000, 1000, 0.01), (700, 3000, 0.02)]:
        m = cases.random_csr(rows, cols, density, 11 + rows, impl)
        rng = np.random.default_rng(rows + impl)
        b = (rng.uniform(0.0, 300.0, m.nnz) if impl == 0 else rng.normal(0.0, 2.0, m.nnz)).astype(np.float32)
        b[::7] = 0.0
        if impl == 0:
            b[1::11] = -1.5                                   # negative: 0 in fixed point
            b[2::13] = np.float32(3.0 / 16777216.0)           # an exact Q8.24 half-ulp tie (1.5 ulp): rounds half up
        csr_a = host.CSRMatrix.from_scipy(m)
        csr_b = host.CSRMatrix.from_arrays(m.shape[0], m.shape[1], m.indptr, m.indices, b)
        cp_a = host.format_matrix(csr_a, impl, skip_empty_rows=True)
        cp_b = host.format_matrix(csr_b, impl, skip_empty_rows=True)
        xw = host.pack_vector(impl, cases.random_x(cp_a.num_cols, rows, impl))
        want_a, want_b = oracle_y(cp_a, impl, xw), oracle_y(cp_b, impl, xw)
        assert not np.array_equal(want_a, want_b)
        same = (lambda a, w: np.array_equal(a, w)) if impl == 0 else (lambda a, w: cases.float_close(a, w))
        with device.SpmvEngine(impl) as eng:
            eng.load_matrix_csr(csr_a)
            eng.load_vector(xw)
            eng.run()
            assert same(eng.read_result(), want_a)
            eng.update_values(b)
            eng.run()
            assert same(eng.read_result(), want_b), "y after the update is not the oracle's for the new values"
            eng.update_values(m.data)
            eng.run()
            assert same(eng.read_result(), want_a)
            lib = device.lib()
            assert lib.hs_update_values(eng._h, b.ctypes.data, m.nnz + 1) == -1          # wrong count
            assert lib.hs_update_values(eng._h, None, m.nnz) == -1                       # null values
            assert lib.hs_update_values_device(eng._h, b.ctypes.data, m.nnz) == -6       # no device memory here
            eng.run()
            assert same(eng.read_result(), want_a), "a refused update changed the matrix"
        with device.SpmvEngine(impl) as eng:                                             # CPSR: no value order to follow
            eng.load_matrix(cp_a)
            assert device.lib().hs_update_values(eng._h, b.ctypes.data, m.nnz) == -6
            eng.load_vector(xw); eng.run()
            assert same(eng.read_result(), want_a)
        with device.SpmvEngine(impl) as eng:                                             # nothing loaded
            assert device.lib().hs_update_values(eng._h, b.ctypes.data, m.nnz) == -5
        checked += 1
print("cpu value update ok", checked)
"""


def test_cpu_backend_updates_csr_values_to_the_oracle_of_the_new_values():
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    env.pop("HISPARSE_STREAM_FORMAT", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "cpu value update ok 6" in r.stdout, r.stdout + r.stderr


def test_both_libraries_and_exports_carry_the_update_entry_points():
    for name in ("hs_update_values", "hs_update_values_device"):
        assert name in device.EXPORTS
        assert hasattr(device.lib(), name)
        assert hasattr(ctypes.CDLL(CPU_LIB), name)
    lib = device.lib()
    assert lib.hs_update_values(None, None, 0) == -1
    assert lib.hs_update_values_device(None, None, 0) == -1


def test_update_kernel_is_a_plain_streaming_kernel(shipped):  # noqa: F811
    meta, code = shipped
    names = [n for n in meta if "value_update_kernel" in n]
    assert len(names) == 8, names                   # fixed / float x 16-byte / 4-byte loads x one image / two
    for n in names:
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        assert meta[n].get("group_segment_fixed_size", 0) == 0, f"{n} uses LDS"
        body = code[n]
        assert not [i for i in body if re.match(r"(global|flat|buffer)_atomic", i)], f"{n}: memory-side atomics"
        assert not [i for i in body if i.startswith("v_mfma")], f"{n}: MFMA"
        assert not [i for i in body if i.startswith("scratch_")], f"{n}: scratch access"
        assert [i for i in body if i.startswith("global_store_dword ")], f"{n}: no 4-byte scatter store"
    vec = [n for n in names if re.search(r"value_update_kernelILb[01]ELb1E", n)]
    assert vec and all(any(i.startswith("global_load_dwordx4") for i in code[n]) for n in vec), "the 16-byte streaming loads are missing"


def test_one_device_definition_of_the_value_conversion():
    csrc = os.path.join(ROOT, "hisparse_amd", "csrc")
    defs = []
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".cpp")):
            text = open(os.path.join(csrc, f)).read()
            defs += [f] * len(re.findall(r"uint32_t\s+value_word\s*\(\s*float", text))
    assert defs == ["value_word.h"], defs
    for f in ("gpu_tiles.hip", "value_update.hip"):
        assert '#include "value_word.h"' in open(os.path.join(csrc, f)).read()
