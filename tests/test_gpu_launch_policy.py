"""The stream cache policy is taken per launch, by the image's reuse distance (hs_api.cpp: launch_args; reuse_tracker.h): the results are the same words
whatever the tracker decides.  Two power-law matrices A and B (the 40 000 x 70 000 case of tests/test_gpu_options.py and a second seed of it) on ONE
stream, launched in the order A, A, A, B, A, B, B, A -- cold, warm, warm, cold, ... as far as their images let them -- with a read-back after every
launch, through every entry point that launches the SpMV kernel.  Fixed point: bit for bit against the oracle.  Float modes: bit for bit against the
same plan with `nt` forced (the cache policy of a load cannot change a bit), which itself is within the float tolerance of the oracle.
Launch i runs on vector i % 2, so that a result left over from the previous launch never passes.  Which instantiation ran is not observed here."""
import numpy as np
import pytest

from hisparse_amd import device, host

import cases
import delta24_cases as dc
import option_variants as ov

pytestmark = pytest.mark.gpu

ROWS, COLS = 40000, 70000
ORDER = "AAABABBA"
KINDS = ("run", "batch", "graph", "partition", "iterate")
PLANS = [(fmt, slices, carry) for fmt in ("pairs", "delta", "delta24", "sweep") for slices, carry in ((1, None), (3, "0"), (3, "1"))]
_MADE = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ov.option_keys():
        monkeypatch.delenv("HISPARSE_" + k, raising=False)


def _feedback_words(impl):
    if impl == 0:
        return dc.word(0.01), dc.word(0.001)
    return tuple(int(np.array([v], dtype=np.float32).view(np.uint32)[0]) for v in (0.01, 0.001))


def _matrices(impl):
    """{name: ChannelPackets}, the two vectors, and the oracle's y per (name, vector) -- made once per numeric mode, never written again"""
    if impl not in _MADE:
        cps, wants = {}, {}
        for name, seed in (("A", 71 + impl), ("B", 171 + impl)):
            g = host.CSRMatrix.generate("powerlaw", ROWS, COLS, a=2.2e6, b=0.35, c=1.0 if impl == 0 else 2.0, seed=seed)
            cps[name] = host.format_matrix(g, impl, skip_empty_rows=True)
        xs = [host.pack_vector(impl, cases.random_x(cps["A"].num_cols, 13 + k, impl)) for k in range(2)]
        for name, cp in cps.items():
            for k, xw in enumerate(xs):
                wants[name, k] = dc.oracle_y(cp, impl, xw)
        for a in xs + list(wants.values()):
            a.setflags(write=False)
        _MADE[impl] = (cps, xs, wants)
    return _MADE[impl]


def _iterate_wants(impl):
    """fixed point: the oracle's y after three steps of x = scale * y + shift, per (name, vector)"""
    key = ("iterate", impl)
    if key not in _MADE:
        cps, xs, wants = _matrices(impl)
        scale, shift = _feedback_words(impl)
        out = {}
        for (name, k), y in wants.items():
            x = np.array(xs[k])
            for _ in range(2):
                x = dc.feedback_reference(y, x, scale, shift)
                y = dc.oracle_y(cps[name], impl, x)
            y.setflags(write=False)
            out[name, k] = y
        _MADE[key] = out
    return _MADE[key]


def _engine(impl, cp, fmt, slices, carry, resident=None):
    eng = device.SpmvEngine(impl)
    eng.set_option("stream_format", fmt)
    eng.set_option("col_slices", str(slices))
    eng.set_option("light", "0")
    if carry is not None:
        eng.set_option("carry_combine", carry)
    if resident is not None:
        eng.set_option("stream_resident", resident)
    eng.load_matrix(cp)
    st = eng.stats()
    assert device.STREAM_FORMATS[st["stream_format"]] == fmt.replace("delta24", "delta") and st["col_slices"] == slices, st
    if fmt == "delta24":
        assert st["value_bits"] == 24
    return eng


def _launch(eng, kind, cp, xw, impl):
    """one launch of the loaded image through entry point `kind` on vector xw, and its read-back"""
    eng.load_vector(xw)
    if kind == "run":
        eng.run()
    elif kind in ("batch", "graph"):      # (graph: the option is set around the whole sequence, so that a captured graph is kept and replayed)
        eng.run_batch(4)
        if kind == "graph":
            eng.run_batch(4)
    elif kind == "partition":
        for j in range(cp.num_row_partitions):
            eng.run_partition(j, cp.part_len(j))
    else:
        eng.iterate(3, *_feedback_words(impl))
    return eng.read_result()


def _sequence(engines, cps, xs, impl, kind, order=ORDER):
    """the read-backs of `order` launched through `kind`: [(name, vector index, y)]"""
    for eng in engines.values():
        eng.set_option("batch_graph", "1" if kind == "graph" else "0")
    out = []
    for i, name in enumerate(order):
        out.append((name, i % 2, _launch(engines[name], kind, cps[name], xs[i % 2], impl)))
    return out


def _references(impl, fmt, slices, carry):
    """{kind: {(name, vector): y}}: fixed point: the oracle; float modes: the same plan with `nt` forced, checked against the oracle's tolerance"""
    cps, xs, wants = _matrices(impl)
    if impl == 0:
        return {kind: (_iterate_wants(impl) if kind == "iterate" else wants) for kind in KINDS}
    refs = {kind: {} for kind in KINDS}
    for name, cp in cps.items():
        with _engine(impl, cp, fmt, slices, carry, resident="0") as eng:
            assert eng.stats()["stream_resident"] == 0
            for kind in KINDS:
                eng.set_option("batch_graph", "1" if kind == "graph" else "0")
                for k in range(2):
                    refs[kind][name, k] = _launch(eng, kind, cp, xs[k], impl)
                    if kind != "iterate":
                        assert cases.float_close(refs[kind][name, k], wants[name, k]), (kind, name, k)
    return refs


def _check(impl, fmt, slices, carry):
    cps, xs, _ = _matrices(impl)
    refs = _references(impl, fmt, slices, carry)
    a = _engine(impl, cps["A"], fmt, slices, carry)
    b = _engine(impl, cps["B"], fmt, slices, carry)
    try:
        assert a.stats()["stream_resident"] == 1 and b.stats()["stream_resident"] == 1      # eligible: the tracker decides every launch below
        b.set_stream(a.get_stream())
        engines = {"A": a, "B": b}
        for kind in KINDS:
            for i, (name, k, y) in enumerate(_sequence(engines, cps, xs, impl, kind)):
                assert np.array_equal(y, refs[kind][name, k]), (kind, i, name)
    finally:
        b.set_stream(None)
        b.close()
        a.close()


@pytest.mark.parametrize("fmt,slices,carry", PLANS)
def test_fixed_point_is_bit_exact_whatever_the_tracker_decides(fmt, slices, carry):
    _check(0, fmt, slices, carry)


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("fmt,slices,carry", [p for p in PLANS if p[0] != "delta24"])      # (the float modes keep the plain record)
def test_float_modes_match_the_forced_nt_result_bit_for_bit(impl, fmt, slices, carry):
    _check(impl, fmt, slices, carry)


def test_a_reload_between_launches_starts_cold_and_changes_nothing():
    """A, A, reload A, A, A, B, A: the reloaded image has a new id -- cold once, then warm again -- and every read-back is the oracle's"""
    cps, xs, wants = _matrices(0)
    a = _engine(0, cps["A"], "delta24", 3, "1")
    b = _engine(0, cps["B"], "delta24", 3, "1")
    try:
        b.set_stream(a.get_stream())
        engines = {"A": a, "B": b}
        for i, name in enumerate("AArAABA"):
            if name == "r":
                a.load_matrix(cps["A"])
                assert a.stats()["stream_resident"] == 1 and a.stats()["value_bits"] == 24
                continue
            assert np.array_equal(_launch(engines[name], "run", cps[name], xs[i % 2], 0), wants[name, i % 2]), (i, name)
    finally:
        b.set_stream(None)
        b.close()
        a.close()
