"""tests/delta24_decoder.py — the packed DELTA record (stream_tiles.h: kRecordBytes24) read back in numpy, next to tile_emulator.

Test infrastructure.  `runs(tiles)` walks every (block, unit, wavefront) run of a DELTA image, plain or packed, slot by slot;
`unpack(tiles)` turns a packed image into the plain one with the same dealing -- value word = field << value_shift, every outlier
put back into the slot it left -- so that tile_emulator.run, with all its assertions, can walk it; on the way it checks what only
the packed form has: the outlier lists name real slots of their own block, those slots carry field 0, and the lists lie behind the records.
"""
from collections import namedtuple

import numpy as np

from hisparse_amd import device

import tile_emulator

WAVE, CONSUMERS, SUB_TILE, BRIDGE = 64, 14, 8192, 0xFFFF
PLAIN_BYTES, PACKED_BYTES = 768, 640

# value / gap / pos: [slot, lane] over the run's slots AFTER the head (2 x records - 1 of them); head: [lane]
Run = namedtuple("Run", "block unit wave first_record records head value gap pos")


def _record_slots(image, at, packed, shift):
    """(value words [2, 64], gaps [2, 64], head positions [64]) of the record at byte `at`"""
    if not packed:
        rec = image[at: at + PLAIN_BYTES]
        vals = rec[:WAVE * 8].view(np.uint32).reshape(WAVE, 2).T.astype(np.int64)
        gaps = rec[WAVE * 8:].view(np.uint16).reshape(WAVE, 2).T.astype(np.int64)
        return vals, gaps, vals[0]
    rec = image[at: at + PACKED_BYTES]
    word = rec[:WAVE * 8].view(np.uint64)
    field_a, field_b = (word & np.uint64(0xFFFFFF)).astype(np.int64), ((word >> np.uint64(24)) & np.uint64(0xFFFFFF)).astype(np.int64)
    gap_a, gap_b = (word >> np.uint64(48)).astype(np.int64), rec[WAVE * 8:].view(np.uint16).astype(np.int64)
    return np.stack([field_a << shift, field_b << shift]), np.stack([gap_a, gap_b]), field_a | (gap_a << 24)


def runs(tiles):
    packed = tiles["value_bits"] == 24
    stride, shift = (PACKED_BYTES, tiles["value_shift"]) if packed else (PLAIN_BYTES, 0)
    image, blocks, units = tiles["image"], tiles["blocks"], tiles["units"]
    out = []
    for b, blk in enumerate(blocks):
        step = [0] * CONSUMERS
        for u in range(int(blk["unit_begin"]), int(blk["unit_end"])):
            for w in range(CONSUMERS):
                end, base = int(units[u]["end_step"][w]), int(blk["wave_offset"][w])
                if end > step[w]:
                    recs = [_record_slots(image, base + s * stride, packed, shift) for s in range(step[w], end)]
                    value = np.concatenate([r[0] for r in recs])[1:]
                    gap = np.concatenate([r[1] for r in recs])[1:]
                    head = recs[0][2]
                    out.append(Run(b, u, w, step[w], end - step[w], head, value, gap, (head[None, :] + np.cumsum(gap, axis=0)) & 0xFFFFFFFF))
                step[w] = end
    return out


def outlier_lists(tiles):
    """{block index: structured array of its outliers (row, col, value)}; checks where the lists lie"""
    assert tiles["value_bits"] == 24
    blocks, image = tiles["blocks"], tiles["image"]
    records_end = max((int(blk["wave_offset"][w]) + int(blk["total_steps"][w]) * PACKED_BYTES for blk in blocks for w in range(CONSUMERS)), default=0)
    lists, total = {}, 0
    for b, blk in enumerate(blocks):
        n = int(blk["outlier_count"])
        assert int(blk["value_bits"]) == 24 and int(blk["value_shift"]) == tiles["value_shift"]
        if n:
            at = int(blk["outlier_lo"]) | int(blk["outlier_hi"]) << 32
            assert at >= records_end and at % 4 == 0 and at + 12 * n <= image.size
            lists[b] = image[at: at + 12 * n].view(device.OUTLIER_DTYPE)
            total += n
    assert image.size == records_end + (12 * total + 15) // 16 * 16          # the records, then the lists, 16-byte aligned as a whole
    return lists


def unpack(tiles):
    """the plain DELTA tiles of a packed image (a new dict; image and Block table are new arrays) and the outliers as (block, row, col, value) tuples"""
    assert tiles["format"] == "delta" and tiles["value_bits"] == 24
    blocks = tiles["blocks"].copy()
    shift = tiles["value_shift"]
    assert (tiles["blocks"]["wave_offset"] % PACKED_BYTES == 0).all()
    blocks["wave_offset"] = tiles["blocks"]["wave_offset"] // PACKED_BYTES * PLAIN_BYTES
    for name in ("outlier_lo", "outlier_hi", "outlier_count", "value_shift", "value_bits"):
        blocks[name] = 0
    lists = outlier_lists(tiles)
    records = sum(int(blk["total_steps"][w]) for blk in blocks for w in range(CONSUMERS))
    image = np.zeros(records * PLAIN_BYTES, dtype=np.uint8)
    pending = {(b, int(o["row"]), int(o["col"])): int(o["value"]) for b, lst in lists.items() for o in lst}
    assert len(pending) == sum(len(lst) for lst in lists.values())              # no (block, row, column) twice
    found = []
    for r in runs(tiles):
        col0 = int(tiles["units"][r.unit]["col0"])
        value, gap = np.vstack([r.head[None, :], r.value]), np.vstack([np.zeros((1, WAVE), dtype=np.int64), r.gap])
        assert (r.value >> shift << shift == r.value).all() and (r.value < (1 << (24 + shift))).all()
        for key in [k for k in pending if k[0] == r.block and col0 <= k[2] < col0 + SUB_TILE]:
            hit = np.argwhere((r.pos == key[1] * SUB_TILE + key[2] - col0) & (r.gap != BRIDGE))
            for s, l in hit:                                                     # (a position occurs once: the unit's elements are distinct)
                if key in pending:
                    assert r.value[s, l] == 0                                    # the outlier's slot carries field 0
                    value[s + 1, l] = pending.pop(key)
                    found.append((r.block, key[1], key[2], int(value[s + 1, l])))
        at = int(blocks[r.block]["wave_offset"][r.wave]) + r.first_record * PLAIN_BYTES
        rec = image[at: at + r.records * PLAIN_BYTES].reshape(r.records, PLAIN_BYTES)
        rec[:, :WAVE * 8] = value.astype(np.uint32).reshape(r.records, 2, WAVE).transpose(0, 2, 1).reshape(r.records, -1).view(np.uint8)
        rec[:, WAVE * 8:] = gap.astype(np.uint16).reshape(r.records, 2, WAVE).transpose(0, 2, 1).reshape(r.records, -1).view(np.uint8)
    assert not pending, pending                                                  # every outlier names a slot of its own block
    plain = dict(tiles, image=image, blocks=blocks, value_bits=32, value_shift=0)
    return plain, found


def run(tiles, impl, x_words, num_rows, **kw):
    """tile_emulator.run over a DELTA image of either kind"""
    if tiles["format"] == "delta" and tiles["value_bits"] == 24:
        tiles = unpack(tiles)[0]
    return tile_emulator.run(tiles, impl, x_words, num_rows, **kw)
