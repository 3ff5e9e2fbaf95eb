"""hisparse_amd.gat — ctypes binding of include/hisparse_gat.h: the graph attention (GAT) step on the multi-head attention object of
hisparse_amd.heads.  The score is additive, x[e][h] = el[row(e)][h] + er[col(e)][h] and t = LeakyReLU(x, slope), followed by the same row
softmax and the same weighted sum of V[col(e)]; the backward returns gel, ger and gV.  el, gel and lse are float32 (num_rows, heads), er
and ger float32 (num_cols, heads), V, gY, Y and gV float32 (n, heads * d).  A model forms el = a_l . Wh and er = a_r . Wh per node and head
before the call; there is no Q, no K, no scale and no per-entry array.

`GraphAttention` IS a `heads.MultiHeadAttention`: one object, one pattern on the device, made by hsmh_create; the dot-product calls stay
reachable through the base class (`heads.MultiHeadAttention.forward(obj, ...)`).  As everywhere in this package there is no Python
compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import heads
from .device import DeviceError

EXPORTS = ["hsgat_forward_device", "hsgat_forward", "hsgat_backward_device", "hsgat_backward"]

_bound = None


def lib():
    """heads.lib() with the hsgat_* prototypes set as well."""
    global _bound
    l = heads.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsgat_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64]
        l.hsgat_forward.argtypes = [vp, vp, vp, vp, u32, u32, f32, vp, vp]
        l.hsgat_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64, vp, u64]
        l.hsgat_backward.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, f32, vp, vp, vp]
        _bound = l
    return l


def _head_words(n, a, heads_, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (n, heads_):
        raise DeviceError(-1, f"{what} must be ({n}, {heads_}) float32, one word per node and head, not {a.shape}")
    return a


class GraphAttention(heads.MultiHeadAttention):
    def forward(self, el, er, V, heads, slope, want_lse=True):
        """hsgat_forward, the host form: el (num_rows, heads), er (num_cols, heads), V (num_cols, heads * d); returns (Y (num_rows,
        heads * d), lse (num_rows, heads)) float32, or Y alone with want_lse=False (the call then passes NULL for lse)."""
        heads = int(heads)
        V = self._features(V, self.num_cols, heads, "V")
        el, er = _head_words(self.num_rows, el, heads, "el"), _head_words(self.num_cols, er, heads, "er")
        Y = np.zeros((self.num_rows, V.shape[1]), dtype=np.float32)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsgat_forward(self._h, el.ctypes.data, er.ctypes.data, V.ctypes.data, heads, V.shape[1] // heads, float(slope), Y.ctypes.data,
                                        lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, el, er, V, gY, lse, heads, slope):
        """hsgat_backward, the host form: el and lse (num_rows, heads), er (num_cols, heads), V (num_cols, heads * d), gY (num_rows,
        heads * d); returns (gel (num_rows, heads), ger (num_cols, heads), gV (num_cols, heads * d)) float32."""
        heads = int(heads)
        V, gY = self._features(V, self.num_cols, heads, "V"), self._features(gY, self.num_rows, heads, "gY")
        w = V.shape[1]
        if w != gY.shape[1]:
            raise DeviceError(-1, f"backward: V has {w} words per row, gY {gY.shape[1]}")
        el, er = _head_words(self.num_rows, el, heads, "el"), _head_words(self.num_cols, er, heads, "er")
        lse = _head_words(self.num_rows, lse, heads, "lse")
        gel = np.zeros((self.num_rows, heads), dtype=np.float32)
        ger = np.zeros((self.num_cols, heads), dtype=np.float32)
        gV = np.zeros((self.num_cols, w), dtype=np.float32)
        self._check(lib().hsgat_backward(self._h, el.ctypes.data, er.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, heads, w // heads, float(slope), gel.ctypes.data,
                                         ger.ctypes.data, gV.ctypes.data))
        return gel, ger, gV

    def forward_device(self, el_ptr, ldel, er_ptr, lder, v_ptr, ldv, heads, d, slope, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsgat_forward_device: pointers (int) into device memory, V and Y 16-byte aligned, ld in words, el, er and lse in rows of ldel,
        lder and ldl words per node, lse_ptr may be None; one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsgat_forward_device(self._h, vp(el_ptr or None), int(ldel), vp(er_ptr or None), int(lder), vp(v_ptr or None), int(ldv), int(heads), int(d), float(slope),
                                               vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, el_ptr, ldel, er_ptr, lder, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, ldl, heads, d, slope, gel_ptr, ldgel, ger_ptr, ldger, gv_ptr, ldgv):
        """hsgat_backward_device: pointers (int) into device memory, V, gY and gV 16-byte aligned, ld in words, the five head arrays in
        rows of their ld words per node; two kernel launches, asynchronous on the object's stream; one backward call in flight per
        object."""
        vp = C.c_void_p
        self._check(lib().hsgat_backward_device(self._h, vp(el_ptr or None), int(ldel), vp(er_ptr or None), int(lder), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                                vp(lse_ptr or None), int(ldl), int(heads), int(d), float(slope), vp(gel_ptr or None), int(ldgel), vp(ger_ptr or None), int(ldger),
                                                vp(gv_ptr or None), int(ldgv)))
