"""Every plan-time option of hs_set_option on the host builder (no GPU): the table of tests/option_variants.py, built for 256 workgroups.
Per variant: (a) the emulated kernel (tests/tile_emulator.py) over the image gives the oracle's y -- bit for bit in fixed point, within 1e-4
and within the float64 bound of its rounding class in the float modes; (b) the image, Block[], Unit[] or the matrix engine's image differs
from the build without the option -- a variant whose option changes nothing tests nothing; (c) the structural fact the option promises.
And a ratchet: every key of kOptionKeys (hs_api.cpp) is in the table or named, with its test file, in COVERED_ELSEWHERE.
The same variants on the device: tests/test_gpu_option_matrix.py."""
import os
import re

import numpy as np
import pytest

from hisparse_amd import device

import cases
import float_contract as fc
import option_variants as ov
import tile_emulator


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for k in ov.option_keys():
        monkeypatch.delenv("HISPARSE_" + k, raising=False)


def _runs(t, blk):
    """the sixteen wavefront runs of a BITMAP block"""
    heads = t["units"][int(blk["unit_begin"]): int(blk["unit_end"])].view(np.uint8).reshape(tile_emulator.BITMAP_WAVES, 5 * 64)
    return np.ascontiguousarray(heads[:, :64]).view(tile_emulator.WAVESEG_DTYPE).reshape(-1)


def _structure(v, t, base, cp):
    changed = {k for k in v.options if v.options.get(k) != v.base.get(k)}
    if "cross_partitions" in changed:
        assert (t["blocks"]["last_part"] == t["blocks"]["row_part"]).all()
        assert (base["blocks"]["last_part"] != base["blocks"]["row_part"]).any()      # ... which the default plan does not keep
        assert cp.num_row_partitions > 1
    if "pow2_slices" in changed:
        assert t["col_slices"] in (1, 2, 4, 8) and base["col_slices"] not in (1, 2, 4, 8)
    if "light_wgs" in changed:
        n = int(v.options["light_wgs"])
        assert len(t["blocks"]) <= ov.WORKGROUPS * n and t["num_workgroups"] <= ov.WORKGROUPS * n
        assert t["format"] == "pairs" and t["col_slices"] == 1
    if "max_rows" in changed:
        n = int(v.options["max_rows"])
        assert t["blocks"]["nrows"].max() <= n < base["blocks"]["nrows"].max() and t["max_block_rows"] <= n
    if "xcd_affinity" in changed:
        assert t["col_slices"] == 4 and sorted(t["block_order"].tolist()) == list(range(len(t["blocks"])))
    if "delta_deal" in changed:
        assert t["format"] == "delta" and t["image"].size == base["image"].size      # the same records, dealt differently
        assert t["col_slices"] == int(v.options["col_slices"])
    if "plan_census" in changed:
        assert t["col_slices"] > 1 and base["col_slices"] == 1
    if "bitmap_skew" in changed:
        assert t["format"] == "bitmap"
        weights = [int(w) for w in v.options["bitmap_skew"].split("/")]
        whole = 0
        for blk in t["blocks"]:
            nrows = int(blk["nrows"])
            runs = _runs(t, blk)
            rows = runs["row_end"].astype(np.int64) - runs["row_begin"]
            if not rows.any():
                continue                                      # a block of empty rows: sixteen idle runs
            if nrows * 2 > tile_emulator.BITMAP_WAVES:        # whole rows per wavefront
                whole += 1
                if len(set(weights)) == 1:
                    assert rows.max() - rows.min() <= 1, (int(blk["row0"]), rows.tolist())
                else:                                         # 9999 : 1: the four wavefronts of the heavy place hold (nearly) all the rows
                    heavy = weights.index(max(weights))
                    assert rows[4 * heavy: 4 * heavy + 4].sum() >= nrows - 3, (int(blk["row0"]), rows.tolist())
            elif len(set(weights)) == 1:                      # pieces of rows: equal shares of the block's groups
                steps = (runs["g_end"].astype(np.int64) - runs["g_begin"])[rows > 0]
                assert steps.max() - steps.min() <= 1, (int(blk["row0"]), steps.tolist())
        assert (whole > 0) == (v.matrix == "thin-300"), whole
    if "mfma_chunk" in changed:
        groups = (cp.num_cols + 63) // 64
        chunk = int(v.options["mfma_chunk"])                  # (a unit of all the groups or more is the whole row)
        assert t["mfma_chunk"] == chunk and t["mfma_chunks"] == ((groups + chunk - 1) // chunk + 3) // 4 * 4
        assert t["image"].tobytes() == base["image"].tobytes()      # the SpMV image is not touched
    if "no_mfma_image" in changed:
        assert t["mfma"].size == 0 and base["mfma"].size > 0 and t["image"].tobytes() == base["image"].tobytes()


@pytest.mark.parametrize("name,impl", ov.params())
def test_variant_on_the_host_builder(name, impl):
    v = ov.BY_NAME[name]
    c = ov.case(v.matrix, impl)
    cp = c.cp
    t = ov.build(v.options, v.matrix, impl)
    base = ov.build(v.base, v.matrix, impl)
    assert t["nnz"] == c.m.nnz
    # (b) teeth
    assert not ov.same_tiles(t, base), "the option changes nothing on this matrix: the variant would test nothing"
    # (c)
    _structure(v, t, base, cp)
    # (a)
    outs = {"run": tile_emulator.run(t, impl, c.xw, cp.num_rows)}
    if "cross_partitions" in v.options or "xcd_affinity" in v.options:      # hs_run_partition's walk over Block::next_part
        y = np.zeros(cp.num_rows, dtype=np.uint32)
        for j in range(cp.num_row_partitions):
            y = tile_emulator.run(t, impl, c.xw, cp.num_rows, row_part_filter=j, y_init=y, rows_per_part=128 * cp.ob_bank)
        outs["partitions"] = y
    for what, y in outs.items():
        if impl == 0:
            assert np.array_equal(y, c.want), (what, np.nonzero(y != c.want)[0][:8])
        else:
            assert cases.float_close(y, c.want), what
            ov.reference(v.matrix, impl).check(y, L=fc.chain(v.chain, c.m, t), slices=int(t["col_slices"]), what=f"{name} {what}")
    if t["mfma"].size:      # the matrix engine's image, walked unit by unit: fp32 products summed in double
        y = tile_emulator.run_mfma(t["mfma"], t["mfma_chunk"], t["mfma_chunks"], cp.num_rows, cp.num_cols, c.xw)[0]
        assert cases.float_close(y, c.want)
        ov.reference(v.matrix, impl).check(y, L=1, what=f"{name} matrix engine image")


def test_a_unit_of_all_the_groups_or_more_is_the_whole_row():
    """mfma_chunk beyond the groups of a row, up to the cap: the image of chunk = groups, four units per tile"""
    cp = ov.case("mfma-17", 1).cp
    groups = (cp.num_cols + 63) // 64
    want = ov.build({"stream_format": "bitmap", "mfma_chunk": str(groups)}, "mfma-17", 1)
    for n in (groups + 1, 1000, 65536):
        t = ov.build({"stream_format": "bitmap", "mfma_chunk": str(n)}, "mfma-17", 1)
        assert t["mfma_chunk"] == n and t["mfma_chunks"] == 4 and ov.same_tiles(t, want), n


@pytest.mark.parametrize("value", ["0", "-3", "65537", "1431655766", "2147483648", "99999999999999999999", "12x", "abc", " 5", "4.0"])
def test_a_chunk_the_kernel_cannot_take_is_refused(value):
    """Not clamped: 1431655766 x 3 wraps to 2 in the kernel's 32 bits (unit 3 of a tile would begin again at group 2 and read values past the
    tile's), std::atoi of a longer number is undefined, and 0 or -3 used to become 1 silently.  From the environment the load refuses with
    HS_ERR_BAD_ARG (hs_set_option refuses the same values itself: tests/test_gpu_option_matrix.py); fixed point has no such image and
    never reads the switch."""
    cp = ov.case("mfma-17", 1).cp
    with ov.environment({"stream_format": "bitmap", "mfma_chunk": value}):
        with pytest.raises(device.DeviceError) as e:
            device.build_tiles(cp, 1, cp.ob_bank, cp.vb_bank, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, ov.WORKGROUPS)
    assert e.value.code == -1 and "MFMA_CHUNK" in str(e.value)


def test_every_option_key_is_tested():
    """The ratchet: a key of kOptionKeys is either set by a variant of the table or named in COVERED_ELSEWHERE with a test file that mentions it."""
    keys = ov.option_keys()
    assert len(keys) >= 32 and len(set(keys)) == len(keys) and "DELTA_DEAL" in keys
    table = ov.table_keys()
    assert table <= set(keys) and set(ov.COVERED_ELSEWHERE) <= set(keys)      # nothing stale on either side
    for k in keys:
        if k in table:
            continue
        assert k in ov.COVERED_ELSEWHERE, f"option {k} is neither in tests/option_variants.py's table nor in COVERED_ELSEWHERE"
        path = os.path.join(ov.ROOT, ov.COVERED_ELSEWHERE[k])
        assert os.path.exists(path), path
        # the key as a whole word where an option is set: HISPARSE_<KEY> of the environment, or the quoted lower-case key of hs_set_option
        # ("light" does not count for "light_wgs", nor a file's name for anything)
        sets = re.compile(rf"HISPARSE_{k}(?![A-Za-z0-9_])|[\"']{k.lower()}[\"']")
        assert path != os.path.abspath(__file__) and sets.search(open(path).read()), f"{ov.COVERED_ELSEWHERE[k]} does not set {k}"
    for want in ("DELTA_DEAL", "BITMAP_SKEW", "MFMA_CHUNK", "NO_MFMA_IMAGE", "LIGHT_WGS", "POW2_SLICES", "CROSS_PARTITIONS", "PLAN_CENSUS", "XCD_AFFINITY",
                 "MAX_ROWS"):
        assert want in table, want
