"""Code-object metadata of the kernels of the neighbour aggregation (hisparse_amd/csrc/neighbor_aggregate.hip) in the shipped gfx950 code
(CPU test, with the helpers of tests/test_isa_invariants.py; metadata only, nothing is disassembled): exactly the seven instantiations
of each of the two kernel templates -- sum, maximum and minimum wanted or not, not all three left out -- none of them with a private
segment (no scratch, no spills), no more LDS than the per-wavefront, per-lane words the instantiation's merge of a long row's four
wavefronts declares, wavefronts of 64 in workgroups of 256.  Prints the register counts DESIGN.md section 6f records."""
import os
import re
import shutil

import pytest

from test_isa_invariants import LIB, LLVM, _code_objects, _metadata

WAVES, LANES = 4, 64
SUMS = WAVES * LANES * 4 * 8              # four double sums per wavefront and lane
PAIRS = WAVES * LANES * 4 * (4 + 4)       # four (value, index) pairs per wavefront and lane
MASKS = sorted((s, x, n) for s in (0, 1) for x in (0, 1) for n in (0, 1) if s or x or n)


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip("libhisparse_hip.so has not been built")
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    tmp = tmp_path_factory.mktemp("isa_aggregate")
    found = {}
    for co in _code_objects(tmp):
        found.update(_metadata(co))
    shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_exactly_the_fourteen_kernels_without_scratch_and_with_the_declared_lds(meta):
    kernels = sorted(n for n in meta if "neighbor_" in n)
    assert len(kernels) == 14, kernels
    for side in ("neighbor_forward_kernel", "neighbor_backward_kernel"):
        got = {}
        for n in kernels:
            m = re.search(side + r"ILb([01])ELb([01])ELb([01])E", n)
            if m:
                got[tuple(int(b) for b in m.groups())] = n
        assert sorted(got) == MASKS, (side, kernels)
        for (s, x, m_), n in sorted(got.items()):
            assert not any(old in n for old in ("wide_dot_kernel", "wide_gather_kernel", "gat_", "gatv2_", "heads_forward", "heads_backward", "attention_backward_", "pattern_attention",
                                                "heads16_", "biased_attention_", "dropout_attention_", "bf16_drop_", "row_softmax")), n
            # forward: the sums and a pair array per extreme the instantiation carries; backward: every term lands in the four sums
            lds = s * SUMS + (x + m_) * PAIRS if "forward" in side else SUMS
            assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
            assert meta[n].get("group_segment_fixed_size", 0) <= lds, f"{n}: {meta[n].get('group_segment_fixed_size')} bytes of LDS, {lds} declared"
            assert meta[n].get("wavefront_size", 64) == 64 and meta[n].get("max_flat_workgroup_size", 256) == 256, n
            print(f"{side}<sum {s}, max {x}, min {m_}>: {meta[n].get('vgpr_count')} VGPRs, {meta[n].get('agpr_count', 0)} AGPRs, {meta[n].get('sgpr_count')} SGPRs, "
                  f"{meta[n].get('group_segment_fixed_size', 0)} bytes of LDS")
