"""hisparse_amd.heads_bias — ctypes binding of include/hisparse_heads_bias.h: the multi-head attention object of hisparse_amd.heads with a
per-entry, per-head additive bias on the score, t[e][h] = scale * Q[row(e)] . K[col(e)] + bias[e][h] (edge encodings, relative-position
and distance biases, soft masks, hard masks as -inf), and the bias's gradient gB[e][h] = P[e][h] (GP[e][h] - D[row(e)][h]) out of the
backward.  bias and gbias are float32 (nnz, heads) in the order of the pattern's `indices`.

`BiasedMultiHeadAttention` IS a `heads.MultiHeadAttention`: one object, one pattern on the device, made by hsmhb_create, which with
backward=True also keeps the entry map the backward with a bias needs (4 * max(nnz, 1) bytes more in info()["device_bytes"]).
entry_map=False makes the object with plain hsmh_create: its forward with a bias works, its backward with a bias is refused.  The calls
without a bias stay reachable through the base class (`heads.MultiHeadAttention.forward(obj, ...)`), with their results unchanged, and
the forward with a bias runs on any such object (`BiasedMultiHeadAttention.forward(obj, ...)`).  As everywhere in this package there is
no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import heads
from .device import DeviceError

EXPORTS = ["hsmhb_create", "hsmhb_forward_device", "hsmhb_forward", "hsmhb_backward_device", "hsmhb_backward"]

_bound = None


def lib():
    """heads.lib() with the hsmhb_* prototypes set as well."""
    global _bound
    l = heads.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsmhb_create.argtypes = [C.POINTER(vp), C.c_int, u32, u32, vp, vp, u32, u32]
        l.hsmhb_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64]
        l.hsmhb_forward.argtypes = [vp, vp, vp, vp, vp, u32, u32, f32, vp, vp]
        l.hsmhb_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64, vp, u64, vp, u64]
        l.hsmhb_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, f32, vp, vp, vp, vp]
        _bound = l
    return l


def _entries(nnz, a, heads_, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (nnz, heads_):
        raise DeviceError(-1, f"{what} must be ({nnz}, {heads_}) float32, one row per entry in the order of indices, not {a.shape}")
    return a


class BiasedMultiHeadAttention(heads.MultiHeadAttention):
    def __init__(self, csr_or_arrays, max_heads, backward=True, device_id=0, entry_map=True):
        """as heads.MultiHeadAttention; entry_map=False creates the object with hsmh_create instead of hsmhb_create"""
        self.entry_map = bool(entry_map)
        super().__init__(csr_or_arrays, max_heads, backward, device_id)

    def _create(self):
        return lib().hsmhb_create if self.entry_map else heads.lib().hsmh_create

    def forward(self, Q, K, V, bias, heads, scale, want_lse=True):
        """hsmhb_forward, the host form: Q (num_rows, heads * d), K and V (num_cols, heads * d), bias (nnz, heads); returns (Y (num_rows,
        heads * d), lse (num_rows, heads)) float32, or Y alone with want_lse=False (the call then passes NULL for lse)."""
        heads = int(heads)
        Q, K, V = self._features(Q, self.num_rows, heads, "Q"), self._features(K, self.num_cols, heads, "K"), self._features(V, self.num_cols, heads, "V")
        if not Q.shape[1] == K.shape[1] == V.shape[1]:
            raise DeviceError(-1, f"forward: Q has {Q.shape[1]} words per row, K {K.shape[1]}, V {V.shape[1]}")
        bias = _entries(self.nnz, bias, heads, "bias")
        Y = np.zeros((self.num_rows, Q.shape[1]), dtype=np.float32)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsmhb_forward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, bias.ctypes.data, heads, Q.shape[1] // heads, float(scale), Y.ctypes.data,
                                        lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, Q, K, V, gY, lse, bias, heads, scale, want_gbias=True):
        """hsmhb_backward, the host form: Q and gY (num_rows, heads * d), K and V (num_cols, heads * d), lse (num_rows, heads), bias (nnz,
        heads); returns (gQ, gK, gV, gbias (nnz, heads)) float32, gbias None with want_gbias=False (the call then passes NULL for it)."""
        heads = int(heads)
        Q, gY = self._features(Q, self.num_rows, heads, "Q"), self._features(gY, self.num_rows, heads, "gY")
        K, V = self._features(K, self.num_cols, heads, "K"), self._features(V, self.num_cols, heads, "V")
        w = Q.shape[1]
        if not w == K.shape[1] == V.shape[1] == gY.shape[1]:
            raise DeviceError(-1, f"backward: Q has {w} words per row, K {K.shape[1]}, V {V.shape[1]}, gY {gY.shape[1]}")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows, heads):
            raise DeviceError(-1, f"lse must be ({self.num_rows}, {heads}) float32, not {lse.shape}")
        bias = _entries(self.nnz, bias, heads, "bias")
        gQ = np.zeros((self.num_rows, w), dtype=np.float32)
        gK, gV = (np.zeros((self.num_cols, w), dtype=np.float32) for _ in range(2))
        gB = np.zeros((self.nnz, heads), dtype=np.float32) if want_gbias else None
        self._check(lib().hsmhb_backward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, bias.ctypes.data, heads, w // heads, float(scale),
                                         gQ.ctypes.data, gK.ctypes.data, gV.ctypes.data, gB.ctypes.data if want_gbias else None))
        return gQ, gK, gV, gB

    def forward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, bias_ptr, ldb, heads, d, scale, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsmhb_forward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, bias in rows of ldb words per
        entry, lse_ptr may be None (rows of ldl words otherwise); one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsmhb_forward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(bias_ptr or None), int(ldb),
                                               int(heads), int(d), float(scale), vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, ldl, bias_ptr, ldb, heads, d, scale, gq_ptr, ldgq, gk_ptr, ldgk, gv_ptr, ldgv,
                        gbias_ptr=None, ldgb=0):
        """hsmhb_backward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, lse in rows of ldl words, bias
        and gbias in rows of ldb and ldgb words per entry, gbias_ptr may be None; two kernel launches, asynchronous on the object's
        stream; one backward call in flight per object."""
        vp = C.c_void_p
        self._check(lib().hsmhb_backward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                                vp(lse_ptr or None), int(ldl), vp(bias_ptr or None), int(ldb), int(heads), int(d), float(scale), vp(gq_ptr or None), int(ldgq),
                                                vp(gk_ptr or None), int(ldgk), vp(gv_ptr or None), int(ldgv), vp(gbias_ptr or None), int(ldgb)))
