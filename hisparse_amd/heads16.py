"""hisparse_amd.heads16 — ctypes binding of include/hisparse_heads_bf16.h: the multi-head attention object of hisparse_amd.heads with bf16
operands.  Q, K, V, gY, Y, gQ, gK and gV are bf16 bit patterns in uint16 arrays stored [index][head][feature] (d in {8, 16, ..., 256},
heads * d <= 512); lse stays float32 (rows, heads), so a forward in one precision may be followed by a backward in the other.

`MultiHeadAttentionBF16` IS a `heads.MultiHeadAttention`: one object, one pattern on the device, construction, `info`, `set_stream` and
`sync` inherited; its four compute methods call hsmh16_* where the base class calls hsmh_*.  The fp32 methods of the same object stay
reachable through the base class (`heads.MultiHeadAttention.forward(obj, ...)`).  As everywhere in this package there is no Python
compute path and no fallback; `to_bf16` / `from_bf16` only convert arrays.
"""
import ctypes as C

import numpy as np

from . import heads
from .device import DeviceError

EXPORTS = ["hsmh16_forward_device", "hsmh16_forward", "hsmh16_backward_device", "hsmh16_backward"]

MAX_WIDTH = 512   # heads * d
DS = (8, 16, 32, 64, 128, 256)

_bound = None


def lib():
    """heads.lib() with the hsmh16_* prototypes set as well."""
    global _bound
    l = heads.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsmh16_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64]
        l.hsmh16_forward.argtypes = [vp, vp, vp, vp, u32, u32, f32, vp, vp]
        l.hsmh16_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64, vp, u64]
        l.hsmh16_backward.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, f32, vp, vp, vp]
        _bound = l
    return l


def to_bf16(a):
    """float32 array -> uint16 array of bf16 bit patterns, round to nearest even; NaN stays NaN (quiet), +-inf and -0 survive"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    rounded = (bits + (np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (bits >> np.uint32(16)) | np.uint32(0x0040), rounded).astype(np.uint16)


def from_bf16(a):
    """uint16 array of bf16 bit patterns -> float32 array of the same values (exact)"""
    return (np.ascontiguousarray(a, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


class MultiHeadAttentionBF16(heads.MultiHeadAttention):
    def _features16(self, a, n, heads_, what):
        a = np.asarray(a)
        if a.dtype != np.uint16:
            raise DeviceError(-1, f"{what} must hold bf16 bit patterns in uint16 (heads16.to_bf16), not {a.dtype}")
        a = np.ascontiguousarray(a)
        if a.ndim != 2 or a.shape[0] != n or heads_ < 1 or a.shape[1] % heads_:
            raise DeviceError(-1, f"{what} must be ({n}, heads * d) uint16 with heads = {heads_}, not {a.shape}")
        return a

    def forward(self, Q, K, V, heads, scale, want_lse=True):
        """hsmh16_forward, the host form: Q (num_rows, heads * d), K and V (num_cols, heads * d) uint16; returns (Y (num_rows, heads * d)
        uint16, lse (num_rows, heads) float32), or Y alone with want_lse=False (the call then passes NULL for lse)."""
        heads = int(heads)
        Q, K, V = self._features16(Q, self.num_rows, heads, "Q"), self._features16(K, self.num_cols, heads, "K"), self._features16(V, self.num_cols, heads, "V")
        if not Q.shape[1] == K.shape[1] == V.shape[1]:
            raise DeviceError(-1, f"forward: Q has {Q.shape[1]} elements per row, K {K.shape[1]}, V {V.shape[1]}")
        Y = np.zeros((self.num_rows, Q.shape[1]), dtype=np.uint16)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsmh16_forward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, heads, Q.shape[1] // heads, float(scale), Y.ctypes.data,
                                         lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, Q, K, V, gY, lse, heads, scale):
        """hsmh16_backward, the host form: Q and gY (num_rows, heads * d), K and V (num_cols, heads * d) uint16, lse (num_rows, heads)
        float32; returns (gQ (num_rows, heads * d), gK (num_cols, heads * d), gV (num_cols, heads * d)) uint16."""
        heads = int(heads)
        Q, gY = self._features16(Q, self.num_rows, heads, "Q"), self._features16(gY, self.num_rows, heads, "gY")
        K, V = self._features16(K, self.num_cols, heads, "K"), self._features16(V, self.num_cols, heads, "V")
        w = Q.shape[1]
        if not w == K.shape[1] == V.shape[1] == gY.shape[1]:
            raise DeviceError(-1, f"backward: Q has {w} elements per row, K {K.shape[1]}, V {V.shape[1]}, gY {gY.shape[1]}")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows, heads):
            raise DeviceError(-1, f"lse must be ({self.num_rows}, {heads}) float32, not {lse.shape}")
        gQ = np.zeros((self.num_rows, w), dtype=np.uint16)
        gK, gV = (np.zeros((self.num_cols, w), dtype=np.uint16) for _ in range(2))
        self._check(lib().hsmh16_backward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, heads, w // heads, float(scale), gQ.ctypes.data,
                                          gK.ctypes.data, gV.ctypes.data))
        return gQ, gK, gV

    def forward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, heads, d, scale, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsmh16_forward_device: pointers (int) into device memory, features 16-byte aligned, ld in ELEMENTS (multiples of 8), lse_ptr may
        be None (rows of ldl float32 words otherwise); one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsmh16_forward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), int(heads), int(d), float(scale),
                                                vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, ldl, heads, d, scale, gq_ptr, ldgq, gk_ptr, ldgk, gv_ptr, ldgv):
        """hsmh16_backward_device: pointers (int) into device memory, features 16-byte aligned, ld in ELEMENTS, lse in rows of ldl float32
        words; two kernel launches, asynchronous on the object's stream; one backward call in flight per object, whichever precision."""
        vp = C.c_void_p
        self._check(lib().hsmh16_backward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                                 vp(lse_ptr or None), int(ldl), int(heads), int(d), float(scale), vp(gq_ptr or None), int(ldgq), vp(gk_ptr or None), int(ldgk),
                                                 vp(gv_ptr or None), int(ldgv)))
