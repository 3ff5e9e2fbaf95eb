"""hisparse_amd.gatv2 — ctypes binding of include/hisparse_gatv2.h: the GATv2 step on the multi-head attention object of
hisparse_amd.heads.  Per head the score is t[e] = a . LeakyReLU(XD[row(e)] + XS[col(e)], slope), a d-term dot over a non-linearity of a
sum of two rows, followed by the same row softmax and the weighted sum of the same rows XS[col(e)]; the backward returns gXD, gXS and ga.
XD, gY, Y and gXD are float32 (num_rows, heads * d), XS and gXS float32 (num_cols, heads * d), a and ga float32 (heads, d) or
(heads * d,), lse float32 (num_rows, heads).  A model forms XD = W_dst x and XS = W_src x before the call; there is no per-entry array.

`GraphAttentionV2` IS a `heads.MultiHeadAttention`: one object, one pattern on the device, made by hsmh_create; the dot-product calls stay
reachable through the base class.  The device form of the backward works in a workspace the caller owns, `work_bytes(heads, d)` bytes of
device memory.  As everywhere in this package there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import heads
from .device import DeviceError

EXPORTS = ["hsgat2_forward_device", "hsgat2_forward", "hsgat2_work_bytes", "hsgat2_backward_device", "hsgat2_backward"]

_bound = None


def lib():
    """heads.lib() with the hsgat2_* prototypes set as well."""
    global _bound
    l = heads.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsgat2_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u32, u32, f32, vp, u64, vp, u64]
        l.hsgat2_forward.argtypes = [vp, vp, vp, vp, u32, u32, f32, vp, vp]
        l.hsgat2_work_bytes.argtypes = [vp, u32, u32, C.POINTER(u64)]
        l.hsgat2_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, u64, u32, u32, f32, vp, u64, vp, u64, vp, vp, u64]
        l.hsgat2_backward.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, f32, vp, vp, vp]
        _bound = l
    return l


def _vector(a, width, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size != width:
        raise DeviceError(-1, f"{what} must hold heads * d = {width} float32 words, not {a.shape}")
    return a.reshape(width)


class GraphAttentionV2(heads.MultiHeadAttention):
    def forward(self, XD, XS, a, heads, slope, want_lse=True):
        """hsgat2_forward, the host form: XD (num_rows, heads * d), XS (num_cols, heads * d), a (heads, d); returns (Y (num_rows,
        heads * d), lse (num_rows, heads)) float32, or Y alone with want_lse=False (the call then passes NULL for lse)."""
        heads = int(heads)
        XD, XS = self._features(XD, self.num_rows, heads, "XD"), self._features(XS, self.num_cols, heads, "XS")
        w = XS.shape[1]
        if w != XD.shape[1]:
            raise DeviceError(-1, f"forward: XS has {w} words per row, XD {XD.shape[1]}")
        a = _vector(a, w, "a")
        Y = np.zeros((self.num_rows, w), dtype=np.float32)
        lse = np.zeros((self.num_rows, heads), dtype=np.float32) if want_lse else None
        self._check(lib().hsgat2_forward(self._h, XD.ctypes.data, XS.ctypes.data, a.ctypes.data, heads, w // heads, float(slope), Y.ctypes.data, lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def backward(self, XD, XS, a, gY, lse, heads, slope):
        """hsgat2_backward, the host form: XD, gY (num_rows, heads * d), XS (num_cols, heads * d), a (heads, d), lse (num_rows, heads);
        returns (gXD (num_rows, heads * d), gXS (num_cols, heads * d), ga (heads, d)) float32."""
        heads = int(heads)
        XD, XS, gY = self._features(XD, self.num_rows, heads, "XD"), self._features(XS, self.num_cols, heads, "XS"), self._features(gY, self.num_rows, heads, "gY")
        w = XS.shape[1]
        if w != XD.shape[1] or w != gY.shape[1]:
            raise DeviceError(-1, f"backward: XS has {w} words per row, XD {XD.shape[1]}, gY {gY.shape[1]}")
        a = _vector(a, w, "a")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows, heads):
            raise DeviceError(-1, f"lse must be ({self.num_rows}, {heads}) float32, not {lse.shape}")
        gXD = np.zeros((self.num_rows, w), dtype=np.float32)
        gXS = np.zeros((self.num_cols, w), dtype=np.float32)
        ga = np.zeros((heads, w // heads), dtype=np.float32)
        self._check(lib().hsgat2_backward(self._h, XD.ctypes.data, XS.ctypes.data, a.ctypes.data, gY.ctypes.data, lse.ctypes.data, heads, w // heads, float(slope), gXD.ctypes.data,
                                          gXS.ctypes.data, ga.ctypes.data))
        return gXD, gXS, ga

    def work_bytes(self, heads, d):
        """hsgat2_work_bytes: the bytes of device memory backward_device needs as its workspace for this object, heads and d."""
        out = C.c_uint64(0)
        rc = lib().hsgat2_work_bytes(self._h, int(heads), int(d), C.byref(out))
        if rc != 0:
            raise DeviceError(rc, f"hsgat2_work_bytes refuses heads = {heads}, d = {d}")
        return int(out.value)

    def forward_device(self, xd_ptr, ldxd, xs_ptr, ldxs, a_ptr, heads, d, slope, y_ptr, ldy, lse_ptr=None, ldl=0):
        """hsgat2_forward_device: pointers (int) into device memory, 16-byte aligned, ld in words, a heads * d contiguous words, lse in
        rows of ldl words, lse_ptr may be None; one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsgat2_forward_device(self._h, vp(xd_ptr or None), int(ldxd), vp(xs_ptr or None), int(ldxs), vp(a_ptr or None), int(heads), int(d), float(slope),
                                                vp(y_ptr or None), int(ldy), vp(lse_ptr or None), int(ldl)))

    def backward_device(self, xd_ptr, ldxd, xs_ptr, ldxs, a_ptr, gy_ptr, ldgy, lse_ptr, ldl, heads, d, slope, gxd_ptr, ldgxd, gxs_ptr, ldgxs, ga_ptr, work_ptr, work_bytes):
        """hsgat2_backward_device: pointers (int) into device memory, 16-byte aligned, ld in words; work_ptr is work_bytes(heads, d) bytes
        of the caller's; three kernel launches, asynchronous on the object's stream; one backward call in flight per object."""
        vp = C.c_void_p
        self._check(lib().hsgat2_backward_device(self._h, vp(xd_ptr or None), int(ldxd), vp(xs_ptr or None), int(ldxs), vp(a_ptr or None), vp(gy_ptr or None), int(ldgy),
                                                 vp(lse_ptr or None), int(ldl), int(heads), int(d), float(slope), vp(gxd_ptr or None), int(ldgxd), vp(gxs_ptr or None), int(ldgxs),
                                                 vp(ga_ptr or None), vp(work_ptr or None), int(work_bytes)))
