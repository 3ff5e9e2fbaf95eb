"""ISA invariants of the row softmax's kernels (hisparse_amd/csrc/row_softmax.hip) in the shipped gfx950 code (CPU test, with the
helpers of tests/test_isa_invariants.py): no scratch, no matrix engine, no memory-side atomics; shuffles for the group reductions and
barriers plus a few bytes of LDS for the long rows.  One kernel per direction holds every class's instance (one launch per call), so
the long-row instance's LDS is the kernel's: four doubles, one per wavefront -- what the workgroup reductions need and no more."""
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
    tmp = tmp_path_factory.mktemp("isa_rows")
    meta, code = {}, {}
    for co in _code_objects(tmp):
        meta.update(_metadata(co))
        code.update(_disassembly(co))
    shutil.rmtree(tmp, ignore_errors=True)
    return meta, code


def test_row_softmax_kernels_use_registers_shuffles_and_a_few_bytes_of_lds(shipped):
    meta, code = shipped
    kernels = sorted(n for n in meta if "row_softmax" in n)
    assert len(kernels) == 2 and [bool(re.search(r"row_softmax_kernelILb%dEE" % b, n)) for b, n in enumerate(kernels)] == [True, True], kernels      # forward, backward
    for n in kernels:
        body = code[n]
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        assert not [i for i in body if i.startswith("scratch_")], f"{n}: scratch access"
        assert not [i for i in body if i.startswith("v_mfma")], f"{n}: MFMA"
        assert not [i for i in body if re.match(r"(global|flat|buffer)_atomic", i)], f"{n}: memory-side atomics"
        assert not [i for i in body if re.match(r"ds_(add|sub|min|max|cmpst|cmpswap|wrxchg|pk_add|inc|dec|and|or|xor)", i)], f"{n}: LDS atomics"
        # the long rows: workgroup barriers and one double per wavefront; the groups add nothing to it (their reductions are lane shuffles)
        assert meta[n].get("group_segment_fixed_size", 0) == 4 * 8, (n, meta[n].get("group_segment_fixed_size"))
        assert [i for i in body if i.startswith("s_barrier")], f"{n}: no workgroup barrier"
        # shuffles: log2 G exchanges per reduction for G = 4 ... 64 and the long rows' wavefront step, 26 in all, two words each for a double
        assert len([i for i in body if i.startswith("ds_bpermute_b32")]) >= 2 * 26, f"{n}: the group reductions are not lane shuffles"
        # the workgroup step of the long rows: one double per wavefront written to LDS, the four read back
        assert [i for i in body if i.startswith("ds_write_b64")] and [i for i in body if re.match(r"ds_read(2)?_b(64|128)", i)], f"{n}: no LDS traffic for the long rows"
        assert [i for i in body if i.startswith("global_load_dword")] and [i for i in body if i.startswith("global_store_dword")], n
    forward = code[kernels[0]]
    assert [i for i in forward if i.startswith("v_exp_f32")], "expf's core instruction is missing from the forward kernel"
    assert [i for i in forward if i.startswith("v_div_scale_f64")] and [i for i in forward if i.startswith("v_add_f64")], "the row sum and the quotient are taken in double"
