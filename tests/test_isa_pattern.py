"""ISA invariants of the sampled dense product's kernels (hisparse_amd/csrc/sddmm.hip) in the shipped gfx950 code (CPU test, with the
helpers of tests/test_isa_invariants.py): registers only -- no scratch, no memory-side atomics, no matrix engine -- and 16-byte loads and
stores on the entry stream."""
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
    tmp = tmp_path_factory.mktemp("isa_pattern")
    meta, code = {}, {}
    for co in _code_objects(tmp):
        meta.update(_metadata(co))
        code.update(_disassembly(co))
    shutil.rmtree(tmp, ignore_errors=True)
    return meta, code


def test_sddmm_kernels_stay_in_registers_and_move_16_bytes(shipped):
    meta, code = shipped
    product = [n for n in meta if re.search(r"sddmm_kernelILb[01]ELb[01]ELb[01]E", n)]
    assert len(product) == 8, product                      # fixed | float  x  staged | direct  x  accumulate | overwrite
    others = [n for n in meta if "expand_rows_kernel" in n or "stage4_kernel" in n]
    assert len(others) == 2, others
    for n in product + others:
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        body = code[n]
        assert not [i for i in body if i.startswith("scratch_")], f"{n}: scratch access"
        assert not [i for i in body if re.match(r"(global|flat|buffer)_atomic", i)], f"{n}: memory-side atomics"
        assert not [i for i in body if i.startswith("v_mfma")], f"{n}: MFMA"
        assert meta[n].get("group_segment_fixed_size", 0) == 0, f"{n} uses LDS"
    for n in product:
        body = code[n]
        loads = [i for i in body if i.startswith("global_load_dwordx4")]
        stores = [i for i in body if i.startswith("global_store_dwordx4")]
        assert len(loads) >= 2 and stores, (n, len(loads), len(stores))
        assert sum(" nt" in i for i in loads) >= 2, f"{n}: row[] and col[] are streamed once and carry the non-temporal hint"
        staged = re.search(r"sddmm_kernelILb[01]ELb([01])", n).group(1) == "1"
        if staged:
            assert len(loads) >= 2 + 8, f"{n}: four entries x two operands of 16-byte gathers per group"
    stage = [n for n in others if "stage4" in n][0]
    assert [i for i in code[stage] if i.startswith("global_store_dwordx4")], stage
