"""ISA invariants of the fused attention backward step's two kernels (hisparse_amd/csrc/attention_backward.hip) in the shipped gfx950 code
(CPU test, with the helpers of tests/test_isa_invariants.py), exactly what tests/test_isa_wide.py checks of its kernels: both present, no
scratch, no memory-side atomics, no matrix engine, and 16-byte gathers -- one `global_load_dwordx4` brings four features of an entry's
row."""
import os
import re
import shutil

import pytest

from test_isa_invariants import LIB, LLVM, _code_objects, _disassembly, _metadata


@pytest.fixture(scope="module")
def shipped(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip("libhisparse_hip.so has not been built")
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("no llvm-objdump / llvm-readelf")
    tmp = tmp_path_factory.mktemp("isa_attention_backward")
    meta, code = {}, {}
    for co in _code_objects(tmp):
        meta.update(_metadata(co))
        code.update(_disassembly(co))
    shutil.rmtree(tmp, ignore_errors=True)
    return meta, code


def test_backward_kernels_stay_in_registers_and_gather_16_bytes(shipped):
    meta, code = shipped
    kernels = sorted(n for n in meta if "attention_backward_rows_kernel" in n or "attention_backward_cols_kernel" in n)
    assert len(kernels) == 2 and sum("attention_backward_rows_kernel" in n for n in kernels) == 1, kernels      # the row side and the column side
    for n in kernels:
        body = code[n]
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        assert not [i for i in body if i.startswith("scratch_")], f"{n}: scratch access"
        assert not [i for i in body if re.match(r"(global|flat|buffer)_atomic", i)], f"{n}: memory-side atomics"
        assert not [i for i in body if i.startswith("v_mfma")], f"{n}: MFMA"
        assert [i for i in body if i.startswith("global_load_dwordx4")], f"{n}: no 16-byte gather"
