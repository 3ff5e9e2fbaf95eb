"""tests/delta24_cases.py — the seeded matrices of the packed DELTA tests (test_delta24_cpu.py, test_gpu_delta24.py), each made once.

The shared matrix: 30 000 x 20 000, twelve values below 1.0 per row -- and, so that one matrix reaches every slot kind the packed record has,
stretches of twenty EMPTY rows (positions jump by more than 16 bits there: bridge slots) and a tail of 1000 rows of a hundred values each (blocks flagged
kBlockDenseRows).  Row partitions of 8192 rows (ob_bank 64), so that hs_run_partition has four of them to walk.
"""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from hisparse_amd import device, host
from oracle import oracle as orc

import cases
import delta24_decoder as dd
import option_variants as ov

VB_BANK, OB_BANK = 4096, 64
DENSE_ROWS = 1        # Block::flags bit kBlockDenseRows
# the empty rows of the shared matrix: stretches of twenty, all over it -- at 256 workgroups a lane's run is one or two slots long, and only some
# of the stretches leave a lane with a bridge slot AND the element behind it
HOLES = tuple(r for start in range(100, 29000, 1500) for r in range(start, start + 20))
KINDS = ("first slot", "last slot", "after a bridge", "plain block", "saturating row", "low bits", "dense block, first slot", "dense block, last slot")
PLANTED = {"first slot": 1.0, "last slot": 2.5, "after a bridge": 17.25, "plain block": 255.0, "saturating row": 300.0,
           "low bits": float(np.float32(1.0) + np.float32(2.0 ** -23)), "dense block, first slot": 300.0, "dense block, last slot": 100.0}

Case = namedtuple("Case", "m cp xw want")


def random_rows(rows, cols, per_row, seed, dense_tail=0, empty=()):
    """seeded CSR with values in [0.01, 0.99): `per_row` columns per row (duplicates dropped), 100 per row in the last `dense_tail` rows"""
    rng = np.random.default_rng(seed)
    r = np.concatenate([np.repeat(np.arange(rows - dense_tail), per_row), np.repeat(np.arange(rows - dense_tail, rows), 100)])
    c = rng.integers(0, cols, r.size)
    keep = ~np.isin(r, np.asarray(empty, dtype=np.int64))
    key = np.unique(r[keep].astype(np.int64) * cols + c[keep])
    data = rng.uniform(0.01, 0.99, key.size).astype(np.float32)
    m = sp.csr_matrix((data, (key // cols, key % cols)), shape=(rows, cols))
    m.sort_indices()
    return m


def word(value):
    return int(host.pack_vector(0, np.array([value], dtype=np.float32))[0])


def build(cp, impl, fmt, workgroups, **options):
    """the host builder's tiles under STREAM_FORMAT = fmt (None: unforced) and further options"""
    with ov.environment(dict(options, stream_format=fmt) if fmt else options):
        return device.build_tiles(cp, impl, cp.ob_bank, cp.vb_bank, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, workgroups)


def oracle_y(cp, impl, xw):
    return orc.spmv(impl, [cp.channel_ptr(c)[0] for c in range(16)], xw, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions,
                    cp.ob_bank, cp.vb_bank)


def records(t):
    return sum(int(b["total_steps"][w]) for b in t["blocks"] for w in range(dd.CONSUMERS))


def same(a, b):
    return a["image"].tobytes() == b["image"].tobytes() and a["blocks"].tobytes() == b["blocks"].tobytes() and a["units"].tobytes() == b["units"].tobytes()


def _case(m, impl=0, x_scale=1.0, x_seed=5, banks=(VB_BANK, OB_BANK)):
    _, cp = cases.formatted(m, impl, banks[0], banks[1], True)
    xw = host.pack_vector(impl, cases.random_x(cp.num_cols, x_seed, impl) * np.float32(x_scale))
    want = oracle_y(cp, impl, xw)
    for a in (xw, want):
        a.setflags(write=False)
    return Case(m, cp, xw, want)


_MADE = {}


def _once(name, make):
    if name not in _MADE:
        _MADE[name] = make()
    return _MADE[name]


def below_one():
    """case 1: all values below 1.0"""
    return _once("below_one", lambda: _case(random_rows(30000, 20000, 12, 11, dense_tail=1000, empty=HOLES)))


def integers():
    """case 3: values drawn from {1.0, 2.0, 3.0, 255.0}; x small enough that no row saturates"""
    def make():
        m = random_rows(8000, 20000, 12, 12)
        m.data = np.random.default_rng(12).choice(np.array([1.0, 2.0, 3.0, 255.0], dtype=np.float32), m.nnz)
        return _case(m, x_scale=0.01, x_seed=6)
    return _once("integers", make)


def over_the_cap():
    """case 4: one element in 1000 is >= 2^24"""
    def make():
        m = random_rows(8000, 20000, 12, 13)
        m.data[::1000] = np.float32(1.5)
        return _case(m, x_seed=8)
    return _once("over_the_cap", make)


def tall(rows):
    """case 5: `rows` x 20 000 at 8 per row: with two column slices the row ranges hold 2300 rows and more, head positions pass 2^24"""
    return _once(("tall", rows), lambda: _case(random_rows(rows, 20000, 8, 14), x_seed=7))


def float_case(impl):
    def make():
        m = random_rows(3000, 20000, 40, 15)
        m.data = np.random.default_rng(15).normal(0.0, 1.0, m.nnz).astype(np.float32)
        return _case(m, impl=impl, banks=host.default_banks(impl))
    return _once(("float", impl), make)


def _element(m, blk, unit, pos):
    """(row of the matrix, column, index into m.data) of the element at position `pos` of a unit of block `blk`"""
    row, col = int(blk["row0"]) + (int(pos) >> 13), int(unit["col0"]) + (int(pos) & 8191)
    lo, hi = m.indptr[row], m.indptr[row + 1]
    k = lo + int(np.searchsorted(m.indices[lo:hi], col))
    assert k < hi and m.indices[k] == col
    return row, col, k


def pick_slots(m, plain):
    """{kind: (row, column, index into m.data)}: eight element slots of the plain DELTA image `plain` of m, one per kind of KINDS.  The dealing
    does not depend on the values, so a packed build of the same pattern under the same plan puts them into the same slots."""
    blocks, units = plain["blocks"], plain["units"]
    assert (blocks["flags"] & DENSE_ROWS).any() and not (blocks["flags"] & DENSE_ROWS).all()
    picks, used = {}, set()

    def take(kind, r, s, l):
        real = r.value[s, l] != 0 and r.gap[s, l] != dd.BRIDGE
        at = (r.block, r.unit, int(r.pos[s, l]))
        if kind not in picks and real and at not in used:
            used.add(at)
            picks[kind] = _element(m, blocks[r.block], units[r.unit], r.pos[s, l])

    for r in dd.runs(plain):
        live = np.nonzero(((r.value != 0) & (r.gap != dd.BRIDGE)).any(axis=1))[0]
        if not live.size:
            continue
        last = int(live[-1])                       # the run's last slot (behind it: at most the dead slot of an odd run)
        lanes = np.nonzero(r.value[last] != 0)[0]
        if blocks[r.block]["flags"] & DENSE_ROWS:
            take("dense block, first slot", r, 0, 7)
            take("dense block, last slot", r, last, int(lanes[-1]))
        else:
            take("first slot", r, 0, 5)
            take("last slot", r, last, int(lanes[0]))
            after = np.argwhere((r.gap[:-1] == dd.BRIDGE) & (r.gap[1:] != dd.BRIDGE) & (r.value[1:] != 0))
            if after.size:
                take("after a bridge", r, int(after[0][0]) + 1, int(after[0][1]))
            take("plain block", r, min(3, last), 20)
            take("saturating row", r, min(2, last), 40)
            take("low bits", r, min(4, last), 33)
        if len(picks) == len(KINDS):
            break
    assert sorted(picks) == sorted(KINDS), sorted(picks)
    return picks


Planted = namedtuple("Planted", "m cp xw want picks outliers saturated_row")


def planted(workgroups, **options):
    """case 2: the matrix of case 1 with eight words planted that do not fit 24 bits, in slots of the kinds of KINDS under the plan the builder makes
    for `workgroups` workgroups and `options`; outliers: the (row of the matrix, column, value word) the outlier lists must hold, sorted"""
    def make():
        base = below_one()
        plain = build(base.cp, 0, "delta32", workgroups, **options)
        assert plain["format"] == "delta" and plain["value_bits"] == 32
        picks = pick_slots(base.m, plain)
        m = base.m.copy()
        for kind, (_, _, k) in picks.items():
            m.data[k] = np.float32(PLANTED[kind])
        assert word(PLANTED["first slot"]) == 0x1000000 and word(PLANTED["saturating row"]) == 0xFFFFFFFF and word(PLANTED["low bits"]) == 0x1000002
        _, cp = cases.formatted(m, 0, VB_BANK, OB_BANK, True)
        xw = base.xw.copy()
        xw[picks["saturating row"][1]] = word(3.0)      # 256 x 3.0: the row's sum leaves Q8.24
        want = oracle_y(cp, 0, xw)
        assert want[picks["saturating row"][0]] == 0xFFFFFFFF
        for a in (xw, want):
            a.setflags(write=False)
        return Planted(m, cp, xw, want, picks, sorted((row, col, word(PLANTED[kind])) for kind, (row, col, _) in picks.items()), picks["saturating row"][0])
    return _once(("planted", workgroups, tuple(sorted(options.items()))), make)


def found_outliers(tiles):
    """the outlier lists of a packed image as sorted (row of the matrix, column, value word); asserts (delta24_decoder.unpack) that every entry names a
    slot of its own block and that the slot carries field 0"""
    _, found = dd.unpack(tiles)
    return sorted((int(tiles["blocks"][b]["row0"]) + row, col, value) for b, row, col, value in found)


def feedback_reference(y_words, x_words, scale, shift):
    """hs_feedback in fixed point: x[i] = sat(round(scale * y[i]) + shift) for i < min(rows, columns)"""
    n = min(len(y_words), len(x_words))
    out = x_words.copy()
    prod = np.minimum((y_words[:n].astype(object) * int(scale) + (1 << 23)) >> 24, 0xFFFFFFFF)
    out[:n] = np.minimum(prod + int(shift), 0xFFFFFFFF).astype(np.uint32)
    return out
