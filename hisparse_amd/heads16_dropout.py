"""hisparse_amd.heads16_dropout — ctypes binding of include/hisparse_heads_dropout_bf16.h: the multi-head attention object of
hisparse_amd.heads_dropout with bf16 feature operands.  Q, K, V, gY, Y, gQ, gK and gV are bf16 bit patterns in uint16 arrays stored
[index][head][feature] (d in {8, 16, ..., 256}, heads * d <= 512); bias and gbias stay float32 (nnz, heads), bias may be None; lse stays
float32 (rows, heads), so a forward in one precision may be followed by a backward in the other with the same (drop_p, seed, offset).
The keep decision is heads_dropout's: `heads_dropout.keep_mask` gives the mask of a call of this module.

`DropoutMultiHeadAttentionBF16` IS a `heads_dropout.DropoutMultiHeadAttention`: one object, one pattern on the device, nothing new
allocated; its four compute methods call hsmhd16_* where the base class calls hsmhd_*.  The fp32 methods of the same object stay reachable
through the base class (`heads_dropout.DropoutMultiHeadAttention.forward(obj, ...)`), and the bf16 calls without bias and dropout through
`heads16.lib()`.  As everywhere in this package there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import heads16, heads_dropout
from .device import DeviceError
from .heads16 import from_bf16, to_bf16  # noqa: F401  (re-exported: the arrays of this module are made with them)
from .heads_bias import _entries

EXPORTS = ["hsmhd16_forward_device", "hsmhd16_forward", "hsmhd16_backward_device", "hsmhd16_backward"]

MAX_WIDTH = heads16.MAX_WIDTH   # heads * d
DS = heads16.DS

_bound = None


def lib():
    """heads_dropout.lib() with the hsmh16_* and hsmhd16_* prototypes set as well."""
    global _bound
    l = heads_dropout.lib()
    if _bound is not l:
        heads16.lib()
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsmhd16_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, f32, u64, u64, vp, u64, vp, u64]
        l.hsmhd16_forward.argtypes = [vp, vp, vp, vp, vp, u32, u32, f32, f32, u64, u64, vp, vp]
        l.hsmhd16_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, f32, u64, u64, vp, u64, vp, u64, vp, u64, vp, u64]
        l.hsmhd16_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, f32, f32, u64, u64, vp, vp, vp, vp]
        _bound = l
    return l


_features16 = heads16.MultiHeadAttentionBF16._features16      # called as a function: the methods below also run on other objects of the family


class DropoutMultiHeadAttentionBF16(heads_dropout.DropoutMultiHeadAttention):
    _features16 = _features16      # so that heads16.MultiHeadAttentionBF16.forward(obj, ...), the hsmh16_* calls, run on this object too

    def forward(self, Q, K, V, bias, heads, scale, drop_p, seed, offset, want_lse=True):
        """hsmhd16_forward, the host form: Q (num_rows, heads * d), K and V (num_cols, heads * d) uint16, bias (nnz, heads) float32 or None;
        returns (Y (num_rows, heads * d) uint16, lse (num_rows, heads) float32), or Y alone with want_lse=False (the call then passes NULL)."""
        heads = int(heads)
        Q, K, V = _features16(self, Q, self.num_rows, heads, "Q"), _features16(self, K, self.num_cols, heads, "K"), _features16(self, V, self.num_cols, heads, "V")
        if not Q.shape[1] == K.shape[1] == V.shape[1]:
            raise DeviceError(-1, f"forward: Q has {Q.shape[1]} elements per row, K {K.shape[1]}, V {V.shape[1]}")
        if bias is not None:
            bias = _entries(self.nnz, bias, heads, "bias")
        Y = np.zeros((self.num_rows, Q.shape[1]), dtype=np.uint16)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsmhd16_forward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, None if bias is None else bias.ctypes.data, heads, Q.shape[1] // heads, float(scale),
                                          float(drop_p), int(seed), int(offset), Y.ctypes.data, lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, Q, K, V, gY, lse, bias, heads, scale, drop_p, seed, offset, want_gbias=True):
        """hsmhd16_backward, the host form: Q and gY (num_rows, heads * d), K and V (num_cols, heads * d) uint16, lse (num_rows, heads)
        float32, bias (nnz, heads) float32 or None; returns (gQ, gK, gV uint16, gbias (nnz, heads) float32), gbias None with
        want_gbias=False (the call then passes NULL)."""
        heads = int(heads)
        Q, gY = _features16(self, Q, self.num_rows, heads, "Q"), _features16(self, gY, self.num_rows, heads, "gY")
        K, V = _features16(self, K, self.num_cols, heads, "K"), _features16(self, V, self.num_cols, heads, "V")
        w = Q.shape[1]
        if not w == K.shape[1] == V.shape[1] == gY.shape[1]:
            raise DeviceError(-1, f"backward: Q has {w} elements per row, K {K.shape[1]}, V {V.shape[1]}, gY {gY.shape[1]}")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows, heads):
            raise DeviceError(-1, f"lse must be ({self.num_rows}, {heads}) float32, not {lse.shape}")
        if bias is not None:
            bias = _entries(self.nnz, bias, heads, "bias")
        gQ = np.zeros((self.num_rows, w), dtype=np.uint16)
        gK, gV = (np.zeros((self.num_cols, w), dtype=np.uint16) for _ in range(2))
        gB = np.zeros((self.nnz, heads), dtype=np.float32) if want_gbias else None
        self._check(lib().hsmhd16_backward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, None if bias is None else bias.ctypes.data, heads,
                                           w // heads, float(scale), float(drop_p), int(seed), int(offset), gQ.ctypes.data, gK.ctypes.data, gV.ctypes.data,
                                           gB.ctypes.data if want_gbias else None))
        return gQ, gK, gV, gB

    def forward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, bias_ptr, ldb, heads, d, scale, drop_p, seed, offset, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsmhd16_forward_device: pointers (int) into device memory, features bf16, 16-byte aligned, ld in ELEMENTS (multiples of 8),
        bias_ptr may be None (rows of ldb float32 words per entry otherwise), lse_ptr may be None; one kernel launch, asynchronous on the
        object's stream."""
        vp = C.c_void_p
        self._check(lib().hsmhd16_forward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(bias_ptr or None), int(ldb),
                                                 int(heads), int(d), float(scale), float(drop_p), int(seed), int(offset), vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, ldl, bias_ptr, ldb, heads, d, scale, drop_p, seed, offset, gq_ptr, ldgq, gk_ptr, ldgk,
                        gv_ptr, ldgv, gbias_ptr=None, ldgb=0):
        """hsmhd16_backward_device: pointers (int) into device memory, features bf16, 16-byte aligned, ld in ELEMENTS, lse in rows of ldl
        float32 words, bias (may be None) and gbias (may be None) in rows of ldb and ldgb float32 words per entry; two kernel launches,
        asynchronous on the object's stream; one backward call in flight per object, whichever precision."""
        vp = C.c_void_p
        self._check(lib().hsmhd16_backward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                                  vp(lse_ptr or None), int(ldl), vp(bias_ptr or None), int(ldb), int(heads), int(d), float(scale), float(drop_p), int(seed),
                                                  int(offset), vp(gq_ptr or None), int(ldgq), vp(gk_ptr or None), int(ldgk), vp(gv_ptr or None), int(ldgv), vp(gbias_ptr or None),
                                                  int(ldgb)))
