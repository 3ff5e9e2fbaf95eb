"""hisparse_amd.rows — ctypes binding of include/hisparse_rows.h: the row softmax over a CSR pattern, forward and backward.

    forward    p[e] = exp(scale s[e] - m_row) / sum_row exp(scale s[e'] - m_row)
    backward   gs[e] = scale p[e] (gp[e] - sum_row p[e'] gp[e'])

`RowSoftmax` holds indptr and its schedule on the device; scores, probabilities and gradients are fp32 arrays in CSR order, the order
`SampledProduct.sddmm_device` writes and `SpmvEngine.update_values_device` takes.  The symbols are bound on the handle `device.lib()`
returns, so HISPARSE_HIP_LIB selects libhisparse_cpu.so here as elsewhere (a second implementation on the host, where "device"
pointers are host pointers) -- there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import device, host
from .device import DeviceError

EXPORTS = ["hsr_create", "hsr_destroy", "hsr_last_error", "hsr_info", "hsr_set_stream", "hsr_sync", "hsr_softmax_device",
           "hsr_softmax_backward_device", "hsr_softmax", "hsr_softmax_backward"]

# launch geometry of the kernels (hisparse_amd/csrc/row_softmax.h): at most compute_units * ROWS_BLOCKS_PER_CU workgroups of ROWS_THREADS
# lanes; a lane of a group class holds ROWS_PER_LANE scores, a row of more than ROWS_LONG entries takes a workgroup of its own -- a
# schedule of more virtual workgroups goes round the stride loop
ROWS_THREADS = 256
ROWS_BLOCKS_PER_CU = 8
ROWS_PER_LANE = 4
ROWS_LONG = 256

_bound = None


def rows_per_trip(compute_units, lanes_per_row):
    """the most rows of a group class of `lanes_per_row` lanes one trip of the grid covers on a device of `compute_units` CUs"""
    return compute_units * ROWS_BLOCKS_PER_CU * (ROWS_THREADS // lanes_per_row)


def lib():
    """device.lib() with the hsr_* prototypes set."""
    global _bound
    l = device.lib()
    if _bound is not l:
        vp, u64, f = C.c_void_p, C.c_uint64, C.c_float
        l.hsr_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, vp]
        l.hsr_destroy.argtypes = [vp]
        l.hsr_last_error.restype = C.c_char_p
        l.hsr_last_error.argtypes = [vp]
        l.hsr_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        l.hsr_set_stream.argtypes = [vp, vp]
        l.hsr_sync.argtypes = [vp]
        l.hsr_softmax_device.argtypes = [vp, vp, f, vp]
        l.hsr_softmax_backward_device.argtypes = [vp, vp, vp, f, vp]
        l.hsr_softmax.argtypes = [vp, vp, f, vp]
        l.hsr_softmax_backward.argtypes = [vp, vp, vp, f, vp]
        _bound = l
    return l


def _indptr_of(indptr_or_csr):
    """indptr of a host.CSRMatrix, of a scipy CSR matrix, or the array itself"""
    if isinstance(indptr_or_csr, host.CSRMatrix):
        return indptr_or_csr.arrays()[0]
    if hasattr(indptr_or_csr, "indptr"):
        return indptr_or_csr.indptr
    return indptr_or_csr


class RowSoftmax:
    def __init__(self, indptr_or_csr, device_id=0):
        self._h = C.c_void_p()
        indptr = np.ascontiguousarray(_indptr_of(indptr_or_csr), dtype=np.uint32).ravel()
        if indptr.size < 1:
            raise DeviceError(-1, "indptr is empty")
        rc = lib().hsr_create(C.byref(self._h), device_id, indptr.size - 1, indptr.ctypes.data)
        if rc != 0:
            raise DeviceError(rc, lib().hsr_last_error(None).decode())
        self.num_rows = int(indptr.size - 1)
        self.nnz = self.info()["nnz"]

    def _check(self, rc):
        if rc != 0:
            raise DeviceError(rc, lib().hsr_last_error(self._h).decode() or device.lib().hs_strerror(rc).decode())

    def close(self):
        if self._h:
            lib().hsr_destroy(self._h)
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
        self._check(lib().hsr_info(self._h, C.byref(nnz), C.byref(nbytes)))
        return {"nnz": nnz.value, "device_bytes": nbytes.value}

    def set_stream(self, hip_stream):
        self._check(lib().hsr_set_stream(self._h, C.c_void_p(hip_stream or None)))

    def sync(self):
        self._check(lib().hsr_sync(self._h))

    def _floats(self, a, what):
        a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        if a.size != self.nnz:
            raise DeviceError(-1, f"{what} holds {a.size} values, the pattern {self.nnz} entries")
        return a if a.size else np.zeros(1, dtype=np.float32)

    def softmax(self, scores, scale=1.0):
        """hsr_softmax, the host form: nnz fp32 scores in CSR order; returns the nnz probabilities (float32)."""
        s = self._floats(scores, "scores")
        p = np.empty_like(s)
        self._check(lib().hsr_softmax(self._h, s.ctypes.data, float(scale), p.ctypes.data))
        return p[:self.nnz]

    def softmax_backward(self, probs, grad_probs, scale=1.0):
        """hsr_softmax_backward, the host form: the forward's probabilities and the gradient with respect to them; returns the gradient
        with respect to the scores (float32)."""
        p, gp = self._floats(probs, "probs"), self._floats(grad_probs, "grad_probs")
        gs = np.empty_like(p)
        self._check(lib().hsr_softmax_backward(self._h, p.ctypes.data, gp.ctypes.data, float(scale), gs.ctypes.data))
        return gs[:self.nnz]

    def softmax_device(self, s_ptr, scale, p_ptr):
        """hsr_softmax_device: pointers (int) into device memory, nnz fp32 words each; p_ptr == s_ptr is in place; asynchronous on the
        object's stream."""
        self._check(lib().hsr_softmax_device(self._h, C.c_void_p(s_ptr or None), float(scale), C.c_void_p(p_ptr or None)))

    def softmax_backward_device(self, p_ptr, gp_ptr, scale, gs_ptr):
        """hsr_softmax_backward_device: gs_ptr == gp_ptr is in place; asynchronous on the object's stream."""
        self._check(lib().hsr_softmax_backward_device(self._h, C.c_void_p(p_ptr or None), C.c_void_p(gp_ptr or None), float(scale), C.c_void_p(gs_ptr or None)))
