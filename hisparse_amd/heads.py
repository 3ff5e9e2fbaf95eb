"""hisparse_amd.heads — ctypes binding of include/hisparse_heads.h: multi-head attention over a CSR pattern, forward (one kernel launch)
and backward (two), all heads of a call in one pass, with ROW-MAJOR dense operands stored [index][head][feature] (fp32, d in
{4, 8, ..., 256}, heads * d <= 256) and no per-entry array.

    forward    per head h, on words h d ... h d + d - 1: t[e] = scale * Q[row(e)] . K[col(e)], P = the row softmax of t,
               Y[r] = sum_{e in r} P[e] V[col(e)], lse[r][h] = the row's log-sum-exp of t
    backward   per head h: P[e] = exp(t[e] - lse[row(e)][h]), GP[e] = gY[row(e)] . V[col(e)], D[r] = sum_{e in r} P[e] GP[e],
               GS[e] = scale P[e] (GP[e] - D[row(e)]), gQ[r] = sum_{e in r} GS[e] K[col(e)], gK[c] = sum_{col(e) = c} GS[e] Q[row(e)],
               gV[c] = sum_{col(e) = c} P[e] gY[row(e)]

`MultiHeadAttention` holds the pattern (and, with backward=True, its transpose and the D words) on the device.  The symbols are bound
on the handle `device.lib()` returns, so HISPARSE_HIP_LIB selects libhisparse_cpu.so here as elsewhere (a second implementation on the
host, where "device" pointers are host pointers) -- there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import device
from .device import DeviceError
from .pattern import _pattern_arrays

EXPORTS = ["hsmh_create", "hsmh_destroy", "hsmh_last_error", "hsmh_info", "hsmh_set_stream", "hsmh_sync", "hsmh_forward_device", "hsmh_forward", "hsmh_backward_device",
           "hsmh_backward"]

BACKWARD = 1      # HSMH_BACKWARD
MAX_HEADS = 64
MAX_WIDTH = 256   # heads * d
DS = (4, 8, 16, 32, 64, 128, 256)

_bound = None


def lib():
    """device.lib() with the hsmh_* prototypes set."""
    global _bound
    l = device.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsmh_create.argtypes = [C.POINTER(vp), C.c_int, u32, u32, vp, vp, u32, u32]
        l.hsmh_destroy.argtypes = [vp]
        l.hsmh_last_error.restype = C.c_char_p
        l.hsmh_last_error.argtypes = [vp]
        l.hsmh_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        l.hsmh_set_stream.argtypes = [vp, vp]
        l.hsmh_sync.argtypes = [vp]
        l.hsmh_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64]
        l.hsmh_forward.argtypes = [vp, vp, vp, vp, u32, u32, f32, vp, vp]
        l.hsmh_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64, vp, u64]
        l.hsmh_backward.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, f32, vp, vp, vp]
        _bound = l
    return l


class MultiHeadAttention:
    def __init__(self, csr_or_arrays, max_heads, backward=True, device_id=0):
        """csr_or_arrays: a host.CSRMatrix, a scipy CSR matrix or an (indptr, indices, (rows, cols)) tuple; max_heads: the most heads a
        call will pass (1 ... 64); backward=True sets HSMH_BACKWARD"""
        self._h = C.c_void_p()
        rows, cols, indptr, indices = _pattern_arrays(csr_or_arrays)
        indptr = np.ascontiguousarray(indptr, dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if indptr.size != rows + 1:
            raise DeviceError(-1, f"indptr holds {indptr.size} words for {rows} rows")
        if indptr.size and indices.size < int(indptr.max()):      # (keeps short arrays from being over-read; the library checks the rest)
            raise DeviceError(-4, f"indices holds {indices.size} entries, indptr reaches {int(indptr.max())}")
        if not 0 <= int(max_heads) < 2 ** 32:
            raise DeviceError(-1, f"max_heads must be 1 ... {MAX_HEADS}, not {max_heads}")
        rc = self._create()(C.byref(self._h), device_id, rows, cols, indptr.ctypes.data, indices.ctypes.data if indices.size else None, int(max_heads),
                            BACKWARD if backward else 0)
        if rc != 0:
            raise DeviceError(rc, lib().hsmh_last_error(None).decode())
        self.num_rows, self.num_cols, self.max_heads = int(rows), int(cols), int(max_heads)
        self.nnz = self.info()["nnz"]

    def _create(self):
        """the create call of the object (heads_bias.BiasedMultiHeadAttention asks for hsmhb_create, same arguments)"""
        return lib().hsmh_create

    def _check(self, rc):
        if rc != 0:
            raise DeviceError(rc, lib().hsmh_last_error(self._h).decode() or device.lib().hs_strerror(rc).decode())

    def close(self):
        if self._h:
            lib().hsmh_destroy(self._h)
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
        self._check(lib().hsmh_info(self._h, C.byref(nnz), C.byref(nbytes)))
        return {"nnz": nnz.value, "device_bytes": nbytes.value}

    def set_stream(self, hip_stream):
        self._check(lib().hsmh_set_stream(self._h, C.c_void_p(hip_stream or None)))

    def sync(self):
        self._check(lib().hsmh_sync(self._h))

    def _features(self, a, n, heads, what):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] != n or heads < 1 or a.shape[1] % heads:
            raise DeviceError(-1, f"{what} must be ({n}, heads * d) float32 with heads = {heads}, not {a.shape}")
        return a

    def forward(self, Q, K, V, heads, scale, want_lse=True):
        """hsmh_forward, the host form: Q (num_rows, heads * d), K and V (num_cols, heads * d); returns (Y (num_rows, heads * d),
        lse (num_rows, heads)) float32, or Y alone with want_lse=False (the call then passes NULL for lse)."""
        heads = int(heads)
        Q, K, V = self._features(Q, self.num_rows, heads, "Q"), self._features(K, self.num_cols, heads, "K"), self._features(V, self.num_cols, heads, "V")
        if not Q.shape[1] == K.shape[1] == V.shape[1]:
            raise DeviceError(-1, f"forward: Q has {Q.shape[1]} words per row, K {K.shape[1]}, V {V.shape[1]}")
        Y = np.zeros((self.num_rows, Q.shape[1]), dtype=np.float32)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsmh_forward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, heads, Q.shape[1] // heads, float(scale), Y.ctypes.data,
                                       lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, Q, K, V, gY, lse, heads, scale):
        """hsmh_backward, the host form: Q and gY (num_rows, heads * d), K and V (num_cols, heads * d), lse (num_rows, heads); returns
        (gQ (num_rows, heads * d), gK (num_cols, heads * d), gV (num_cols, heads * d)) float32."""
        heads = int(heads)
        Q, gY = self._features(Q, self.num_rows, heads, "Q"), self._features(gY, self.num_rows, heads, "gY")
        K, V = self._features(K, self.num_cols, heads, "K"), self._features(V, self.num_cols, heads, "V")
        w = Q.shape[1]
        if not w == K.shape[1] == V.shape[1] == gY.shape[1]:
            raise DeviceError(-1, f"backward: Q has {w} words per row, K {K.shape[1]}, V {V.shape[1]}, gY {gY.shape[1]}")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows, heads):
            raise DeviceError(-1, f"lse must be ({self.num_rows}, {heads}) float32, not {lse.shape}")
        gQ = np.zeros((self.num_rows, w), dtype=np.float32)
        gK, gV = (np.zeros((self.num_cols, w), dtype=np.float32) for _ in range(2))
        self._check(lib().hsmh_backward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, heads, w // heads, float(scale), gQ.ctypes.data,
                                        gK.ctypes.data, gV.ctypes.data))
        return gQ, gK, gV

    def forward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, heads, d, scale, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsmh_forward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, lse_ptr may be None (rows of ldl
        words otherwise); one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsmh_forward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), int(heads), int(d), float(scale),
                                              vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, ldl, heads, d, scale, gq_ptr, ldgq, gk_ptr, ldgk, gv_ptr, ldgv):
        """hsmh_backward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, lse in rows of ldl words; two
        kernel launches, asynchronous on the object's stream; one call in flight per object."""
        vp = C.c_void_p
        self._check(lib().hsmh_backward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                               vp(lse_ptr or None), int(ldl), int(heads), int(d), float(scale), vp(gq_ptr or None), int(ldgq), vp(gk_ptr or None), int(ldgk),
                                               vp(gv_ptr or None), int(ldgv)))
