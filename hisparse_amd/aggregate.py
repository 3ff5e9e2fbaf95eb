"""hisparse_amd.aggregate — ctypes binding of include/hisparse_aggregate.h: neighbour aggregation over a CSR pattern, on the pattern object
of hisparse_amd.wide.

    ysum[r][j] = sum  over row r's entries e of X[col(e)][j]            SUM   (MEAN: that sum over the row's length, in the same output)
    ymax[r][j] = max  over row r's entries e of X[col(e)][j]            MAX   amax[r][j] = the CSR index of the winner
    ymin[r][j] = min  ...                                               MIN   amin[r][j] = the CSR index of the winner
    gx[c][j]   = sum over column c's entries k, r = row(k), of  w_r gsum[r][j] + [amax[r][j] == e_k] gmax[r][j] + [amin[r][j] == e_k] gmin[r][j]

One forward call computes every aggregator of `ops` from one gather of X[col(e)] per entry; NaN outranks everything for both extremes and
among equal words the smallest CSR index wins, so ymax[r][j] is bit for bit X[indices[amax[r][j]]][j].  A row without entries gives +0.0
and NONE.  X, the outputs and the gradients are float32 (n, d) with 1 <= d <= 256, the arg arrays uint32 of the same shape.

`NeighborAggregate` IS a `wide.WideProducts`: one object, one pattern on the device, made by hsw_create; sddmm / spmm / spmm_t stay
reachable on it.  The backward needs transposed=True (the default).  The symbols are bound on the handle `device.lib()` returns, so
HISPARSE_HIP_LIB selects libhisparse_cpu.so here as elsewhere -- there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import wide
from .device import DeviceError

EXPORTS = ["hsagg_forward_device", "hsagg_backward_device", "hsagg_forward", "hsagg_backward"]

SUM, MEAN, MAX, MIN = 1, 2, 4, 8
NONE = 0xFFFFFFFF
# every legal `ops` word: at most one of SUM and MEAN, any of MAX and MIN, not nothing
LEGAL_OPS = tuple(s | x | n for s in (0, SUM, MEAN) for x in (0, MAX) for n in (0, MIN) if s | x | n)

_bound = None


def lib():
    """wide.lib() with the hsagg_* prototypes set as well."""
    global _bound
    l = wide.lib()
    if _bound is not l:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        l.hsagg_forward_device.argtypes = [vp, u32, vp, u64, u32, vp, vp, vp, vp, vp, u64]
        l.hsagg_backward_device.argtypes = [vp, u32, vp, vp, vp, vp, vp, u64, u32, vp, u64]
        l.hsagg_forward.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp]
        l.hsagg_backward.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp]
        _bound = l
    return l


def _ptr(a):
    return None if a is None else a.ctypes.data


class NeighborAggregate(wide.WideProducts):
    def _args(self, a, what):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        if a.ndim != 2 or a.shape[0] != self.num_rows:
            raise DeviceError(-1, f"{what} must be ({self.num_rows}, d) uint32, not {a.shape}")
        return a

    def forward(self, X, ops, want_args=True):
        """hsagg_forward, the host form: X (num_cols, d).  Returns a dict with the float32 (num_rows, d) arrays "sum" (for SUM or MEAN),
        "max" and "min" that `ops` asks for and, with want_args, the uint32 arrays "amax" and "amin" beside them (want_args=False passes
        NULL for both)."""
        ops = int(ops)
        X = self._features(X, self.num_cols, "X")
        shape = (self.num_rows, X.shape[1])
        out = {}
        if ops & (SUM | MEAN):
            out["sum"] = np.zeros(shape, dtype=np.float32)
        for bit, name in ((MAX, "max"), (MIN, "min")):
            if ops & bit:
                out[name] = np.zeros(shape, dtype=np.float32)
                if want_args:
                    out["a" + name] = np.zeros(shape, dtype=np.uint32)
        self._check(lib().hsagg_forward(self._h, ops, X.ctypes.data, X.shape[1], _ptr(out.get("sum")), _ptr(out.get("max")), _ptr(out.get("amax")), _ptr(out.get("min")),
                                        _ptr(out.get("amin"))))
        return out

    def backward(self, ops, gsum=None, gmax=None, amax=None, gmin=None, amin=None):
        """hsagg_backward, the host form (needs transposed=True): the gradients (num_rows, d) float32 and the arg arrays (num_rows, d)
        uint32 of the aggregators in `ops`; returns gx (num_cols, d) float32."""
        ops = int(ops)
        given = [None if a is None else (self._features(a, self.num_rows, n) if n[0] == "g" else self._args(a, n))
                 for n, a in (("gsum", gsum), ("gmax", gmax), ("amax", amax), ("gmin", gmin), ("amin", amin))]
        widths = {a.shape[1] for a in given if a is not None}
        if len(widths) != 1:
            raise DeviceError(-1, f"backward: the operands have {sorted(widths)} words per row")
        d = widths.pop()
        gx = np.zeros((self.num_cols, d), dtype=np.float32)
        self._check(lib().hsagg_backward(self._h, ops, *(_ptr(a) for a in given), d, gx.ctypes.data))
        return gx

    def forward_device(self, ops, x_ptr, ldx, d, ysum_ptr, ymax_ptr, amax_ptr, ymin_ptr, amin_ptr, ldy):
        """hsagg_forward_device: pointers (int) into device memory, 16-byte aligned, ld in words; the pointers of outputs `ops` does not
        ask for, and amax_ptr / amin_ptr, may be None; one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsagg_forward_device(self._h, int(ops), vp(x_ptr or None), int(ldx), int(d), vp(ysum_ptr or None), vp(ymax_ptr or None), vp(amax_ptr or None),
                                               vp(ymin_ptr or None), vp(amin_ptr or None), int(ldy)))

    def backward_device(self, ops, gsum_ptr, gmax_ptr, amax_ptr, gmin_ptr, amin_ptr, ldg, d, gx_ptr, ldgx):
        """hsagg_backward_device (needs transposed=True): one kernel launch, asynchronous on the object's stream."""
        vp = C.c_void_p
        self._check(lib().hsagg_backward_device(self._h, int(ops), vp(gsum_ptr or None), vp(gmax_ptr or None), vp(amax_ptr or None), vp(gmin_ptr or None), vp(amin_ptr or None),
                                                int(ldg), int(d), vp(gx_ptr or None), int(ldgx)))
