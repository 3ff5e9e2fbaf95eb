"""hs_load_matrix_csr_transposed without a GPU: the CPU backend loads A^T from A's CSR arrays.  y equals y of the reference load
(load_matrix_csr of scipy's m.T.tocsr() on a second engine) in all three numeric modes, the padded dimensions are those of A^T,
update_values takes A's value order (it equals a reference load of b[perm]), and the error cases are refused with the context still
usable.  Non-square shapes throughout, so that a swapped dimension cannot cancel out."""
import ctypes
import os
import subprocess
import sys

from hisparse_amd import device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "hisparse_amd", "lib", "libhisparse_cpu.so")

CHILD = r"""
import ctypes
import sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from hisparse_amd import device, host
import cases

def u32(a): return np.asarray(a, dtype=np.uint32)

checked = 0
for impl in (0, 1, 2):
    divisor = 128 * (8 if impl == 2 else 1)
    for rows, cols, density in [(1000, 300, 0.02), (300, 3000, 0.02)]:
        m = cases.random_csr(rows, cols, density, 21 + rows, impl)
        nnz = m.nnz
        mt = m.T.tocsr()                                          # the reference: the host-transposed matrix
        perm = sp.csr_matrix((np.arange(nnz, dtype=np.float64), m.indices, m.indptr), shape=m.shape).T.tocsr().data.astype(np.int64)
        assert np.array_equal(mt.data, m.data[perm])
        rng = np.random.default_rng(rows + impl)
        b = (rng.uniform(0.0, 300.0, nnz) if impl == 0 else rng.normal(0.0, 2.0, nnz)).astype(np.float32)
        b[::7] = 0.0
        if impl == 0:
            b[1::11] = -1.5                                       # negative: 0 in fixed point
            b[2::13] = np.float32(3.0 / 16777216.0)               # an exact Q8.24 half-ulp tie: rounds half up
        same = (lambda a, w: np.array_equal(a, w)) if impl == 0 else (lambda a, w: cases.float_close(a, w))
        arrays = lambda mat, data: (mat.shape[0], mat.shape[1], u32(mat.indptr), u32(mat.indices), np.asarray(data, dtype=np.float32))
        with device.SpmvEngine(impl) as t, device.SpmvEngine(impl) as ref:
            t.load_matrix_csr(arrays(m, m.data), transpose=True)
            ref.load_matrix_csr(arrays(mt, mt.data))
            assert (t.num_rows, t.num_cols) == (ref.num_rows, ref.num_cols) == (-(-cols // divisor) * divisor, -(-rows // 8) * 8), (t.num_rows, t.num_cols)
            assert t.csr_nnz == nnz and t.stats()["nnz"] == nnz
            xw = host.pack_vector(impl, cases.random_x(t.num_cols, rows, impl))
            def y_of(eng):
                eng.load_vector(xw); eng.run()
                return eng.read_result()
            ya = y_of(ref)
            assert ya.any() and same(y_of(t), ya), "y of the transposed load differs from the reference load"
            t.update_values(b)                                    # A's order ...
            ref.load_matrix_csr(arrays(mt, b[perm]))              # ... is the reference's order through perm
            yb = y_of(ref)
            assert not np.array_equal(ya, yb)
            assert same(y_of(t), yb), "y after update_values(b) differs from a reference load of b[perm]"
            t.update_values(m.data)
            assert same(y_of(t), ya)
            lib = device.lib()
            assert lib.hs_update_values(t._h, b.ctypes.data, nnz + 1) == -1
            # the refused loads: BAD_MATRIX (-4), and the context still holds its matrix
            ip, ix = u32(m.indptr), u32(m.indices)
            bad_ix = ix.copy(); bad_ix[nnz // 2] = cols             # an index equal to num_cols
            down = ip.copy(); down[5] = down[6] + 1                 # a decreasing indptr
            off = ip.copy(); off[0] = 1                             # does not start at 0
            pr, pc = ctypes.c_uint32(), ctypes.c_uint32()
            for bad_ip, bad_indices in ((ip, bad_ix), (down, ix), (off, ix)):
                rc = lib.hs_load_matrix_csr_transposed(t._h, rows, cols, bad_ip.ctypes.data, bad_indices.ctypes.data, m.data.ctypes.data, ctypes.byref(pr), ctypes.byref(pc))
                assert rc == -4, rc
            assert lib.hs_load_matrix_csr_transposed(t._h, rows, cols, None, ix.ctypes.data, m.data.ctypes.data, None, None) == -1
            assert lib.hs_load_matrix_csr_transposed(t._h, 0, cols, ip.ctypes.data, ix.ctypes.data, m.data.ctypes.data, None, None) == -1
            t.load_matrix_csr(arrays(m, m.data), transpose=True)   # a good load after the refused ones
            assert same(y_of(t), ya)
            t.load_matrix_csr(arrays(m, m.data))                   # and a plain one: "replaces any previously loaded matrix"
            assert (t.num_rows, t.num_cols) == (-(-rows // divisor) * divisor, -(-cols // 8) * 8)
            t.update_values(b)                                     # (the plain load's own order again)
        checked += 1
# CSC arrays of a matrix are the CSR arrays of its transpose: the same entry point loads the matrix itself from CSC
m = cases.random_csr(500, 1300, 0.02, 5, 0)
csc = m.tocsc()
with device.SpmvEngine(0) as t, device.SpmvEngine(0) as ref:
    t.load_matrix_csr((csc.shape[1], csc.shape[0], u32(csc.indptr), u32(csc.indices), csc.data), transpose=True)
    ref.load_matrix_csr((m.shape[0], m.shape[1], u32(m.indptr), u32(m.indices), m.data))
    assert (t.num_rows, t.num_cols) == (ref.num_rows, ref.num_cols)
    xw = host.pack_vector(0, cases.random_x(t.num_cols, 9, 0))
    ys = []
    for eng in (t, ref):
        eng.load_vector(xw); eng.run(); ys.append(eng.read_result())
    assert ys[0].any() and np.array_equal(ys[0], ys[1])
print("cpu transposed load ok", checked)
"""


def test_cpu_backend_loads_the_transpose_and_keeps_the_callers_value_order():
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    env.pop("HISPARSE_STREAM_FORMAT", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "cpu transposed load ok 6" in r.stdout, r.stdout + r.stderr


def test_both_libraries_and_exports_carry_the_transposed_load():
    name = "hs_load_matrix_csr_transposed"
    assert name in device.EXPORTS
    assert hasattr(device.lib(), name)
    assert hasattr(ctypes.CDLL(CPU_LIB), name)
    assert device.lib().hs_load_matrix_csr_transposed(None, 1, 1, None, None, None, None, None) == -1
