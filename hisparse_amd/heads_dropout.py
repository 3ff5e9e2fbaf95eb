"""hisparse_amd.heads_dropout — ctypes binding of include/hisparse_heads_dropout.h: the multi-head attention object of hisparse_amd.heads_bias
with dropout on the attention weights, P'[e][h] = keep(e, h) P[e][h] / (1 - drop_p), after the softmax, with or without the per-entry,
per-head bias (bias=None).  No mask is stored: forward and backward recompute keep(e, h) from Philox4x32-10 keyed by (seed, offset, the
entry's index in the order of `indices`, the head), so the backward must be given the drop_p, seed and offset of its forward, and a
caller advances `offset` per step and layer.  `keep_mask` returns the mask itself, computed on the host.

`DropoutMultiHeadAttention` IS a `heads_bias.BiasedMultiHeadAttention`: one object, one pattern on the device, nothing new allocated.  Its
forward runs on any object of the family; its backward needs the entry map (entry_map=True, the default, and backward=True).  The calls
without dropout stay reachable through the base classes, with their results unchanged.  As everywhere in this package there is no Python
compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import heads, heads_bias
from .device import DeviceError
from .heads_bias import _entries

EXPORTS = ["hsmhd_forward_device", "hsmhd_forward", "hsmhd_backward_device", "hsmhd_backward", "hsmhd_keep_mask"]

_bound = None


def lib():
    """heads_bias.lib() with the hsmhd_* prototypes set as well."""
    global _bound
    l = heads_bias.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsmhd_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, f32, u64, u64, vp, u64, vp, u64]
        l.hsmhd_forward.argtypes = [vp, vp, vp, vp, vp, u32, u32, f32, f32, u64, u64, vp, vp]
        l.hsmhd_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, f32, u64, u64, vp, u64, vp, u64, vp, u64, vp, u64]
        l.hsmhd_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, f32, f32, u64, u64, vp, vp, vp, vp]
        l.hsmhd_keep_mask.argtypes = [u64, u32, f32, u64, u64, vp]
        _bound = l
    return l


def keep_mask(nnz, heads, drop_p, seed, offset):
    """hsmhd_keep_mask: (nnz, heads) uint8, 1 = kept; a pure host function of the library, no object and no device"""
    keep = np.zeros((int(nnz), int(heads)), dtype=np.uint8)
    rc = lib().hsmhd_keep_mask(int(nnz), int(heads), float(drop_p), int(seed), int(offset), keep.ctypes.data)
    if rc != 0:
        raise DeviceError(rc, f"hsmhd_keep_mask({nnz}, {heads}, {drop_p}, ...) was refused: drop_p must be finite and in [0, 1), heads 1 ... 64")
    return keep


class DropoutMultiHeadAttention(heads_bias.BiasedMultiHeadAttention):
    def keep_mask(self, heads, drop_p, seed, offset):
        """the mask of a call on this object: (nnz, heads) uint8 in the order of indices"""
        return keep_mask(self.nnz, heads, drop_p, seed, offset)

    def forward(self, Q, K, V, bias, heads, scale, drop_p, seed, offset, want_lse=True):
        """hsmhd_forward, the host form: Q (num_rows, heads * d), K and V (num_cols, heads * d), bias (nnz, heads) or None; returns (Y
        (num_rows, heads * d), lse (num_rows, heads)) float32, or Y alone with want_lse=False (the call then passes NULL for lse)."""
        heads = int(heads)
        Q, K, V = self._features(Q, self.num_rows, heads, "Q"), self._features(K, self.num_cols, heads, "K"), self._features(V, self.num_cols, heads, "V")
        if not Q.shape[1] == K.shape[1] == V.shape[1]:
            raise DeviceError(-1, f"forward: Q has {Q.shape[1]} words per row, K {K.shape[1]}, V {V.shape[1]}")
        if bias is not None:
            bias = _entries(self.nnz, bias, heads, "bias")
        Y = np.zeros((self.num_rows, Q.shape[1]), dtype=np.float32)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsmhd_forward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, None if bias is None else bias.ctypes.data, heads, Q.shape[1] // heads, float(scale),
                                        float(drop_p), int(seed), int(offset), Y.ctypes.data, lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, Q, K, V, gY, lse, bias, heads, scale, drop_p, seed, offset, want_gbias=True):
        """hsmhd_backward, the host form: Q and gY (num_rows, heads * d), K and V (num_cols, heads * d), lse (num_rows, heads), bias (nnz,
        heads) or None; returns (gQ, gK, gV, gbias (nnz, heads)) float32, gbias None with want_gbias=False (the call then passes NULL)."""
        heads = int(heads)
        Q, gY = self._features(Q, self.num_rows, heads, "Q"), self._features(gY, self.num_rows, heads, "gY")
        K, V = self._features(K, self.num_cols, heads, "K"), self._features(V, self.num_cols, heads, "V")
        w = Q.shape[1]
        if not w == K.shape[1] == V.shape[1] == gY.shape[1]:
            raise DeviceError(-1, f"backward: Q has {w} words per row, K {K.shape[1]}, V {V.shape[1]}, gY {gY.shape[1]}")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows, heads):
            raise DeviceError(-1, f"lse must be ({self.num_rows}, {heads}) float32, not {lse.shape}")
        if bias is not None:
            bias = _entries(self.nnz, bias, heads, "bias")
        gQ = np.zeros((self.num_rows, w), dtype=np.float32)
        gK, gV = (np.zeros((self.num_cols, w), dtype=np.float32) for _ in range(2))
        gB = np.zeros((self.nnz, heads), dtype=np.float32) if want_gbias else None
        self._check(lib().hsmhd_backward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, None if bias is None else bias.ctypes.data, heads,
                                         w // heads, float(scale), float(drop_p), int(seed), int(offset), gQ.ctypes.data, gK.ctypes.data, gV.ctypes.data,
                                         gB.ctypes.data if want_gbias else None))
        return gQ, gK, gV, gB

    def forward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, bias_ptr, ldb, heads, d, scale, drop_p, seed, offset, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsmhd_forward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, bias_ptr may be None (rows of
        ldb words per entry otherwise), lse_ptr may be None; one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsmhd_forward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(bias_ptr or None), int(ldb),
                                               int(heads), int(d), float(scale), float(drop_p), int(seed), int(offset), vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, ldl, bias_ptr, ldb, heads, d, scale, drop_p, seed, offset, gq_ptr, ldgq, gk_ptr, ldgk,
                        gv_ptr, ldgv, gbias_ptr=None, ldgb=0):
        """hsmhd_backward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, lse in rows of ldl words, bias
        (may be None) and gbias (may be None) in rows of ldb and ldgb words per entry; two kernel launches, asynchronous on the object's
        stream; one backward call in flight per object."""
        vp = C.c_void_p
        self._check(lib().hsmhd_backward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                                vp(lse_ptr or None), int(ldl), vp(bias_ptr or None), int(ldb), int(heads), int(d), float(scale), float(drop_p), int(seed),
                                                int(offset), vp(gq_ptr or None), int(ldgq), vp(gk_ptr or None), int(ldgk), vp(gv_ptr or None), int(ldgv), vp(gbias_ptr or None),
                                                int(ldgb)))
