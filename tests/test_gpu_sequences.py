"""Seeded sequences of entry points on one context against the model of tests/context_model.py: what the fixed scenarios of
tests/test_gpu_carry.py, tests/test_spmspv.py and tests/test_gpu_options.py cover one call pattern at a time -- state that outlives a call
(an owed combine pass, the cached batch graph, bindings, the stream, a reloaded matrix, the SpMSpV staging and overflow word, the value
map) -- explored in random order.  Plan x numeric mode x seed, about 50 ops each; every plan asserts through hs_get_stats that it got the
format, slice count and kernel it forces.  At every observation point ALL tracked buffers are compared: bit for bit in fixed point; in the
float modes against the float64 bound of the route's rounding class, the oracle to 1e-4 and, for a product seen before on the same route,
bit for bit its earlier words.  A mismatch prints the plan, seed, op index and the ops so far as replayable Python.  An unexpected
HS_ERR_HIP ends the whole run: nothing more is started on a device that has faulted.  docs/sequence_tests.md has the measured run."""
import ctypes as C

import numpy as np
import pytest

from hisparse_amd import device

import context_model as cm
import float_contract as fc

pytestmark = pytest.mark.gpu


class HipMemory:
    def __init__(self):
        rt = self.rt = C.CDLL("libamdhip64.so")
        rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        rt.hipFree.argtypes = [C.c_void_p]
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        rt.hipStreamSynchronize.argtypes = [C.c_void_p]
        rt.hipStreamDestroy.argtypes = [C.c_void_p]

    def ok(self, rc, what):
        if rc != 0:
            raise cm.DeviceFault(f"{what} failed with HIP error {rc}")

    def alloc(self, words):
        p = C.c_void_p()
        self.ok(self.rt.hipMalloc(C.byref(p), 4 * words), "hipMalloc")
        return p.value

    def free(self, addr):
        self.ok(self.rt.hipFree(addr), "hipFree")

    def write(self, addr, words):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        self.ok(self.rt.hipMemcpy(addr, words.ctypes.data, words.nbytes, 1), "hipMemcpy (host to device)")

    def read(self, addr, words):
        out = np.empty(words, dtype=np.uint32)
        self.ok(self.rt.hipMemcpy(out.ctypes.data, addr, out.nbytes, 2), "hipMemcpy (device to host)")
        return out

    def stream_create(self):
        s = C.c_void_p()
        self.ok(self.rt.hipStreamCreateWithFlags(C.byref(s), 1), "hipStreamCreateWithFlags")      # non-blocking, like the library's own
        return s.value

    def stream_sync(self, handle):
        self.ok(self.rt.hipStreamSynchronize(handle), "hipStreamSynchronize")

    def device_sync(self):
        self.ok(self.rt.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def stream_destroy(self, handle):
        self.ok(self.rt.hipStreamDestroy(handle), "hipStreamDestroy")


class Device:
    """the backend of context_model.Player on the GPU"""

    def __init__(self):
        self.memory = HipMemory()

    def engine(self, impl, ob_bank, vb_bank):
        return device.SpmvEngine(impl, ob_bank=ob_bank, vb_bank=vb_bank)

    def packets(self, mat):
        return mat.cp()

    def update_values_raw(self, eng, values, nnz):
        return device.lib().hs_update_values(eng._h, values.ctypes.data, nnz)

    def spmspv_status(self, eng):
        flag = C.c_uint32(7)
        rc = device.lib().hs_spmspv_status(eng._h, C.byref(flag), None)
        if rc != 0:
            raise device.DeviceError(rc, "hs_spmspv_status")
        return flag.value

    def plan_info(self, eng, plan, impl, mat):
        """what the load gave, asserted against what the plan forces (as _assert_forced_plan of tests/test_gpu_parity.py), and what the
        float contract needs to know about it"""
        st = eng.stats()
        fmt = device.STREAM_FORMATS[st["stream_format"]]
        assert st["nnz"] == mat.nnz and st["retiled_on_gpu"] in (0, 1)
        if plan.fmt is not None:
            assert fmt == plan.fmt, (plan.name, fmt)
        if plan.light is not None:
            assert st["light_kernel"] == plan.light, (plan.name, st["light_kernel"])
        if plan.slices == 0 and st["col_slices"] == 1:
            pytest.skip("the BITMAP builder does not slice this matrix")
        if plan.slices:
            assert st["col_slices"] == plan.slices, (plan.name, st["col_slices"])
        info = dict(stats=st, fmt=fmt, slices=st["col_slices"], mfma=False, L=1)
        if impl != 0:
            variant = "light" if st["light_kernel"] else fmt
            info["L"] = fc.chain(variant, mat.scipy(), eng.read_tiles() if fmt == "delta" else None)
            info["mfma"] = fmt == "bitmap" and eng.read_mfma_image().size > 0
            if plan.name == "bitmap":
                assert info["mfma"], "the float BITMAP plan has the matrix engine's image"
        return info


def _guarded(play, *args):
    try:
        return play(Device(), *args)
    except cm.DeviceFault as e:
        pytest.exit(f"the device reported a fault; nothing more is started on it:\n{e}", returncode=3)


@pytest.mark.parametrize("seed", cm.SEEDS)
@pytest.mark.parametrize("impl", cm.IMPLS)
@pytest.mark.parametrize("plan", cm.PLANS, ids=lambda p: p.name)
def test_sequence(plan, impl, seed):
    p = _guarded(cm.play_sequence, plan, impl, seed)
    assert p.observations >= 3 and len(p.done) > cm.LENGTH


@pytest.mark.parametrize("seed", cm.SEEDS)
@pytest.mark.parametrize("impl", cm.IMPLS)
def test_two_engines_on_one_stream(impl, seed):
    a, b = _guarded(cm.play_two_engines, impl, seed)
    assert a.observations >= 2 and b.observations >= 2
