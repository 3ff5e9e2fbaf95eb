"""Code-object metadata of the four kernels of the GATv2 step (hisparse_amd/csrc/gatv2_attention.hip) in the shipped gfx950 code (CPU
test, with the helpers of tests/test_isa_invariants.py; metadata only, nothing is disassembled): exactly the four kernels, none of them
with a private segment (no scratch, no spills), no more LDS than the per-wavefront, per-lane sums each kernel declares for the merge of a
long row's four wavefronts, wavefronts of 64 in workgroups of 256.  Prints the register counts DESIGN.md section 6e records."""
import os
import shutil

import pytest

from test_isa_invariants import LIB, LLVM, _code_objects, _metadata

WAVES, LANES = 4, 64
# per wavefront and lane: the forward's four sums and l as doubles and m as a float; the row side's D and four each of A, B, A' and B'
# (its ga sums reuse those words); the column side's four sums of P gY and four of GT dz; the sum of the vectors uses none
LDS = {"gatv2_forward_kernel": WAVES * LANES * (4 * 8 + 8 + 4), "gatv2_backward_rows_kernel": WAVES * LANES * 17 * 8, "gatv2_backward_cols_kernel": WAVES * LANES * 8 * 8,
       "gatv2_reduce_kernel": 0}


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip("libhisparse_hip.so has not been built")
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    tmp = tmp_path_factory.mktemp("isa_gatv2")
    found = {}
    for co in _code_objects(tmp):
        found.update(_metadata(co))
    shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_exactly_the_four_kernels_without_scratch_and_with_the_declared_lds(meta):
    kernels = sorted(n for n in meta if "gatv2_" in n)
    for want in LDS:
        assert sum(want in n for n in kernels) == 1, (want, kernels)
    assert len(kernels) == 4, kernels
    for n in kernels:
        assert not any(old in n for old in ("gat_", "heads_forward", "heads_backward", "attention_backward_", "pattern_attention", "heads16_", "biased_attention_", "dropout_attention_")), n
        want = next(k for k in LDS if k in n)
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        assert meta[n].get("group_segment_fixed_size", 0) <= LDS[want], f"{n}: {meta[n].get('group_segment_fixed_size')} bytes of LDS, {LDS[want]} declared"
        assert meta[n].get("wavefront_size", 64) == 64 and meta[n].get("max_flat_workgroup_size", 256) == 256, n
        print(f"{want}: {meta[n].get('vgpr_count')} VGPRs, {meta[n].get('agpr_count', 0)} AGPRs, {meta[n].get('sgpr_count')} SGPRs, {meta[n].get('group_segment_fixed_size', 0)} bytes of LDS")
