"""ISA invariants of spmv_rowblock_kernel_delta24, the SpMV kernel of DELTA images with 24-bit value fields (CPU test, in the manner of
test_isa_invariants.py: unbundles hisparse_amd/lib/libhisparse_hip.so and disassembles it).  Names only what must be there:
the instantiations, the ring in accumulator registers -- one dwordx2 plus one 16-bit stream load per record, behind `s_nop 4`, read
behind counted waits -- and a consumer loop with no other vector-memory instruction in it.
"""
import re

import pytest

from test_isa_invariants import AGPR, shipped      # noqa: F401  (the module-scoped fixture that disassembles the shipped library)

DELTA24 = re.compile(r"spmv_rowblock_kernel_delta24ILb([01])ELi(\d+)E")
VMEM = re.compile(r"(global|flat|buffer|scratch)_(load|store|atomic)")


def _kernels(meta):
    return {n: DELTA24.search(n) for n in meta if DELTA24.search(n)}


def test_packed_instantiations_exist_for_both_cache_policies_and_fixed_point_only(shipped):
    meta, code = shipped
    kernels = _kernels(meta)
    assert sorted((int(m.group(1)), int(m.group(2))) for m in kernels.values()) == [(0, 0), (1, 0)], list(kernels)      # `nt` and `sc1`, no profiling build
    for n, m in kernels.items():
        policy = " sc1" if int(m.group(1)) else " nt"
        stream = [i for i in code[n] if i.startswith("global_load_") and AGPR.search(i.split(" ", 1)[1])]
        assert stream and all(i.endswith(policy) for i in stream), f"{n}: stream loads without the{policy} policy"
        # fixed point only: 64-bit integer row sums, no double accumulators anywhere
        assert any(i.startswith("ds_add_u64") or i.startswith("ds_add_rtn_u64") for i in code[n])
        assert not any(i.startswith(("ds_add_f64", "ds_add_rtn_f64", "v_add_f64", "v_cvt_f64_f32")) for i in code[n]), f"{n}: float arithmetic in the fixed-point kernel"
        assert meta[n].get("private_segment_fixed_size", 0) == 0, f"{n} spills to scratch"
        assert meta[n]["agpr_count"] == 32, f"{n}: the ring is a0..a31, the compiler allocates none itself"


def test_ring_is_one_dwordx2_and_one_16_bit_load_per_record_behind_counted_waits(shipped):
    meta, code = shipped
    kernels = _kernels(meta)
    assert len(kernels) == 2
    for n in kernels:
        body = code[n]
        wide = [k for k, i in enumerate(body) if i.startswith("global_load_dwordx2") and AGPR.search(i.split(" ", 1)[1])]
        narrow = [k for k, i in enumerate(body) if i.startswith(("global_load_ushort", "global_load_dword ")) and AGPR.search(i.split(" ", 1)[1])]
        reads = [k for k, i in enumerate(body) if i.startswith("v_accvgpr_read_b32")]
        # prime (8 records) + the two consumer loops (dense rows / plain), 8 ring slots each
        assert len(wide) == len(narrow) == 24 and len(reads) == 2 * 8 * 3, (n, len(wide), len(narrow), len(reads))
        for k in wide:
            assert body[k - 1] == "s_nop 4" and k + 1 in narrow, f"{n}: `{body[k]}` between `{body[k - 1]}` and `{body[k + 1]}`"
            assert "offset:512" in body[k + 1]
        for k in reads:
            assert body[k - 1].startswith(("s_waitcnt vmcnt(14)", "v_accvgpr_read_b32")), f"{n}: `{body[k]}` follows `{body[k - 1]}`"
        for k, ins in enumerate(body):      # nothing else touches an accumulator register
            if AGPR.search(ins.split(" ", 1)[1] if " " in ins else ""):
                assert k in wide or k in narrow or k in reads, f"{n}: `{ins}` touches an accumulator register outside the hand-written ring"
        # Inside the consumer loops -- from the first counted wait after the prime to the last ring load -- the stream loads are the only vector memory.
        # The two loops (dense rows, plain) lie apart; between a loop's own first wait and its own last ring load nothing else may load or store.
        in_loop = wide[8:]
        for first, last in ((in_loop[0], in_loop[7]), (in_loop[8], in_loop[15])):
            begin = max(k for k, i in enumerate(body[:first]) if i.startswith("s_waitcnt vmcnt(14)"))      # the counted wait of the loop's first step
            assert body[begin + 1].startswith("v_accvgpr_read_b32")
            other = [body[k] for k in range(begin, last + 2) if VMEM.match(body[k]) and k not in wide and k not in narrow]
            assert not other, f"{n}: vector memory inside the consumer loop besides the ring: {other[:3]}"
