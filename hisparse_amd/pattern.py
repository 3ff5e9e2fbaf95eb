"""hisparse_amd.pattern — ctypes binding of include/hisparse_pattern.h: the sampled dense product (SDDMM) over a CSR pattern.

    out[e] = sum_{j < k} U_j[row(e)] (x) V_j[col(e)]          for every entry e, in CSR order

`SampledProduct` holds the pattern on the device; its result is in the order `SpmvEngine.update_values_device` takes.  The symbols are
bound on the handle `device.lib()` returns, so HISPARSE_HIP_LIB selects libhisparse_cpu.so here as elsewhere (a second implementation
on host threads, where "device" pointers are host pointers) -- there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import device, host
from .device import DeviceError

EXPORTS = ["hsp_create", "hsp_destroy", "hsp_last_error", "hsp_info", "hsp_set_stream", "hsp_sync", "hsp_sddmm_device", "hsp_sddmm"]

MAX_K = 64
# launch geometry of the product kernel (hisparse_amd/csrc/sddmm.h): at most compute_units * SDDMM_BLOCKS_PER_CU workgroups of
# SDDMM_THREADS lanes, SDDMM_ENTRIES_PER_LANE entries per lane and trip -- a larger pattern goes round the grid-stride loop
SDDMM_THREADS = 256
SDDMM_BLOCKS_PER_CU = 8
SDDMM_ENTRIES_PER_LANE = 4

_bound = None


def entries_per_pass(compute_units):
    """the most entries one trip of the product kernel's grid covers on a device of `compute_units` CUs"""
    return compute_units * SDDMM_BLOCKS_PER_CU * SDDMM_THREADS * SDDMM_ENTRIES_PER_LANE


def lib():
    """device.lib() with the hsp_* prototypes set."""
    global _bound
    l = device.lib()
    if _bound is not l:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        l.hsp_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, u32, u32, vp, vp, u32]
        l.hsp_destroy.argtypes = [vp]
        l.hsp_last_error.restype = C.c_char_p
        l.hsp_last_error.argtypes = [vp]
        l.hsp_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        l.hsp_set_stream.argtypes = [vp, vp]
        l.hsp_sync.argtypes = [vp]
        l.hsp_sddmm_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, C.c_int]
        l.hsp_sddmm.argtypes = [vp, vp, vp, u32, vp]
        _bound = l
    return l


def _pattern_arrays(csr):
    """(num_rows, num_cols, indptr, indices) of a host.CSRMatrix, a scipy CSR matrix or an (indptr, indices, (rows, cols)) tuple."""
    if isinstance(csr, host.CSRMatrix):
        indptr, indices, _ = csr.arrays()
        return csr.num_rows, csr.num_cols, indptr, indices
    if hasattr(csr, "indptr") and hasattr(csr, "indices") and hasattr(csr, "shape"):
        return csr.shape[0], csr.shape[1], csr.indptr, csr.indices
    indptr, indices, shape = csr
    return shape[0], shape[1], indptr, indices


class SampledProduct:
    def __init__(self, impl, csr, max_k, device_id=0):
        self._h = C.c_void_p()
        self.impl = host.impl_id(impl)
        rows, cols, indptr, indices = _pattern_arrays(csr)
        indptr = np.ascontiguousarray(indptr, dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if indptr.size != rows + 1:
            raise DeviceError(-1, f"indptr holds {indptr.size} words for {rows} rows")
        if indptr.size and indices.size < int(indptr.max()):      # (keeps short arrays from being over-read; the library checks the rest)
            raise DeviceError(-4, f"indices holds {indices.size} entries, indptr reaches {int(indptr.max())}")
        rc = lib().hsp_create(C.byref(self._h), device_id, self.impl, rows, cols, indptr.ctypes.data, indices.ctypes.data if indices.size else None, max_k)
        if rc != 0:
            raise DeviceError(rc, lib().hsp_last_error(None).decode())
        self.num_rows, self.num_cols, self.max_k = int(rows), int(cols), int(max_k)
        self.ldu, self.ldv = -(-self.num_rows // 4) * 4, -(-self.num_cols // 4) * 4      # the host form's strides
        self.nnz = self.info()["nnz"]

    def _check(self, rc):
        if rc != 0:
            raise DeviceError(rc, lib().hsp_last_error(self._h).decode() or device.lib().hs_strerror(rc).decode())

    def close(self):
        if self._h:
            lib().hsp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def info(self):
        nnz, nbytes = C.c_uint64(), C.c_uint64()
        self._check(lib().hsp_info(self._h, C.byref(nnz), C.byref(nbytes)))
        return {"nnz": nnz.value, "device_bytes": nbytes.value}

    def set_stream(self, hip_stream):
        self._check(lib().hsp_set_stream(self._h, C.c_void_p(hip_stream or None)))

    def sync(self):
        self._check(lib().hsp_sync(self._h))

    def _padded(self, words, n, ld, what):
        words = np.asarray(words)
        if words.ndim == 1:
            words = words[None, :]
        if words.ndim != 2 or words.shape[1] != n or words.dtype.itemsize != 4:
            raise DeviceError(-1, f"sddmm: {what} must be (k, {n}) 32-bit value words")
        out = np.zeros((words.shape[0], ld), dtype=np.uint32)
        out[:, :n] = words.view(np.uint32)
        return out

    def sddmm(self, u_words, v_words):
        """hsp_sddmm, the host form: u_words (k, num_rows) and v_words (k, num_cols) value words (host.pack_vector's; a float32 array is
        taken as its words); returns the nnz result words as uint32 (fp32 bits in the float modes, Q8.24 in fixed point)."""
        u = self._padded(u_words, self.num_rows, self.ldu, "u_words")
        v = self._padded(v_words, self.num_cols, self.ldv, "v_words")
        if u.shape[0] != v.shape[0]:
            raise DeviceError(-1, f"sddmm: {u.shape[0]} vectors in u_words, {v.shape[0]} in v_words")
        out = np.zeros(max(self.nnz, 1), dtype=np.uint32)
        self._check(lib().hsp_sddmm(self._h, u.ctypes.data, v.ctypes.data, u.shape[0], out.ctypes.data))
        return out[:self.nnz]

    def sddmm_device(self, u_ptr, ldu, v_ptr, ldv, k, out_ptr, accumulate=False):
        """hsp_sddmm_device: pointers (int) into device memory, 16-byte aligned; asynchronous on the object's stream."""
        self._check(lib().hsp_sddmm_device(self._h, C.c_void_p(u_ptr or None), int(ldu), C.c_void_p(v_ptr or None), int(ldv), int(k),
                                           C.c_void_p(out_ptr or None), 1 if accumulate else 0))
