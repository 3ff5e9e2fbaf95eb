"""Code-object metadata of the three bf16 kernels of the multi-head attention step with a bias and dropout
(hisparse_amd/csrc/heads16_dropout_attention.hip) in the shipped gfx950 code (CPU test, with the helpers of tests/test_isa_invariants.py;
metadata only, nothing is disassembled): exactly the three kernels, under names no other kernel count matches, none of them with a
private segment (no scratch: the generator's words and the bias stay in registers), no more LDS than the arrays the kernels of
heads16_attention.hip declare for the merge of a long row's four wavefronts (the bias and the generator add none), wavefronts of 64 in
workgroups of 256.  Prints the register counts DESIGN.md section 6c-bf16 records."""
import os
import shutil

import pytest

from test_isa_invariants import LIB, LLVM, _code_objects, _metadata

WAVES, LANES = 4, 64
# what the bf16 kernels declare: the sums of a chunk (8 forward, 16 backward) as doubles per wavefront and lane, and per wavefront and lane
# l (double) and m (float) of the forward, D (double) of the backward's row side
LDS = {"bf16_drop_forward_kernel": WAVES * LANES * (8 * 8 + 8 + 4), "bf16_drop_rows_kernel": WAVES * LANES * (16 * 8 + 8), "bf16_drop_cols_kernel": WAVES * LANES * 16 * 8}
OTHERS = ("heads16_", "dropout_attention_", "biased_attention_", "heads_forward", "heads_backward", "gat_", "gatv2_", "pattern_attention", "attention_backward_")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    assert os.path.exists(LIB), "libhisparse_hip.so has not been built"
    assert os.path.exists(f"{LLVM}/llvm-readelf"), "no llvm-readelf"
    tmp = tmp_path_factory.mktemp("isa_heads16_dropout")
    found = {}
    for co in _code_objects(tmp):
        found.update(_metadata(co))
    shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_exactly_the_three_kernels_without_scratch_and_with_the_declared_lds(meta):
    kernels = sorted(n for n in meta if "bf16_drop_" in n)
    for want in LDS:
        assert sum(want in n for n in kernels) == 1, (want, kernels)
    assert len(kernels) == 3, kernels
    for n in kernels:
        assert not any(old in n for old in OTHERS), n      # the other kernel counts do not see them
        want = next(k for k in LDS if k in n)
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        assert meta[n].get("group_segment_fixed_size", 0) <= LDS[want], f"{n}: {meta[n].get('group_segment_fixed_size')} bytes of LDS, {LDS[want]} declared"
        assert meta[n].get("wavefront_size", 64) == 64 and meta[n].get("max_flat_workgroup_size", 256) == 256, n
        print(f"{want}: {meta[n].get('vgpr_count')} VGPRs, {meta[n].get('agpr_count', 0)} AGPRs, {meta[n].get('sgpr_count')} SGPRs, {meta[n].get('group_segment_fixed_size', 0)} bytes of LDS")
