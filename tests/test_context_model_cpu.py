"""The sequence harness of tests/context_model.py without a GPU: the model's arithmetic against the oracle, the generator's
determinism and coverage, the input condition that keeps saturation from hiding errors, the teeth of the driver against a fake engine with
planted defects, the driver on libhisparse_cpu.so, and the ratchet that keeps every entry point inside the sequences or named with a
reason.  The same driver on the device: tests/test_gpu_sequences.py."""
import inspect
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from hisparse_amd import device, host
from oracle import oracle as orc

import context_model as cm
import option_variants as ov
from test_gpu_parity import _feedback_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "hisparse_amd", "lib", "libhisparse_cpu.so")


def committed_sequences():
    """(label, ops) of every sequence tests/test_gpu_sequences.py plays"""
    for plan in cm.PLANS:
        for impl in cm.IMPLS:
            for seed in cm.SEEDS:
                yield f"{plan.name}-{impl}-{seed}", cm.generate(plan, impl, seed)
    for impl in cm.IMPLS:
        for seed in cm.SEEDS:
            for i, name in enumerate(cm.TWO_ENGINES):
                yield f"two-engines-{impl}-{seed}-{name}", cm.generate(cm.PLAN[name], impl, seed + 300 * i, cm.LENGTH // 2, "shared")


@pytest.mark.parametrize("impl", cm.IMPLS)
@pytest.mark.parametrize("plan", cm.PLANS, ids=lambda p: p.name)
def test_model_arithmetic_is_the_oracles(plan, impl):
    mat = cm.plan_matrix(plan, impl)
    same = (lambda a, b: np.array_equal(a, b)) if impl == 0 else cases_close
    xw = cm.x_words(impl, mat.cols, 1)
    y = mat.spmv(xw)
    assert same(y, mat.oracle_spmv(xw))
    assert impl != 0 or y.any()
    scale, shift = cm.scale_shift(impl)
    assert np.array_equal(cm.feedback_words(impl, y, xw, scale, shift), _feedback_reference(impl, y, xw, scale, shift))
    sat = np.full(8, cm.SAT, dtype=np.uint32)      # the saturating ends of the fixed-point feedback
    assert np.array_equal(cm.feedback_words(impl, sat, sat, scale, shift), _feedback_reference(impl, sat, sat, scale, shift))
    a = mat.scipy()[: plan.rows, : plan.cols].T.tocsr()
    a.sort_indices()
    t = cm.Mat.from_scipy(impl, a)
    rng = np.random.default_rng(3)
    idx = rng.choice(plan.cols, 150, replace=False)
    idx = np.concatenate([idx, idx[:40], idx[:3]]).astype(np.uint32)          # repeated entries: several passes
    w = cm.x_words(impl, len(idx), 2)
    want = orc.spmspv(impl, t.indptr.astype(np.uint32), t.indices.astype(np.uint32), t.words, plan.rows, plan.cols, idx, w)
    assert same(cm.spmspv_words(t, plan.rows, idx, w), want)
    assert not cm.spmspv_words(t, plan.rows, idx[:0], w[:0]).any()


def cases_close(a, b):
    import cases
    return cases.float_close(a, b)


def test_fixed_point_products_round_and_saturate():
    assert int(cm.q_mul(cm.SAT, cm.SAT)) == cm.SAT and int(cm.q_mul(1 << 24, 12345)) == 12345
    assert int(cm.q_mul(1, 1 << 23)) == 1 and int(cm.q_mul(1, (1 << 23) - 1)) == 0            # AP_RND: half rounds up
    m = cm.Mat(0, 128, 8, [0, 3] + [3] * 127, [0, 1, 2], [200.0, 100.0, 0.3333333])            # the row of tests/test_cpu_backend.py
    xw = host.pack_vector(0, np.array([1.5, 1.0, 0.7, 0, 0, 0, 0, 0], dtype=np.float32))
    assert m.spmv(xw)[0] == cm.SAT and np.array_equal(m.spmv(xw), m.oracle_spmv(xw))


def test_generator_is_deterministic_by_seed():
    plan = cm.PLAN["pairs-4-carry"]
    assert cm.generate(plan, 0, 1) == cm.generate(plan, 0, 1)
    assert cm.generate(plan, 0, 1) != cm.generate(plan, 0, 2) and cm.generate(plan, 0, 1) != cm.generate(plan, 1, 1)
    for _, ops in committed_sequences():
        assert all(isinstance(op, tuple) and eval(repr(op)) == op for op in ops)      # printed sequences are replayable


def test_every_op_and_every_pair_occurs():
    ops_seen, pairs, refusals = Counter(), Counter(), Counter()
    for _, ops in committed_sequences():
        for a, b in zip(ops, ops[1:]):
            for name, (first, second) in cm.PAIRS.items():
                pairs[name] += bool(first(a) and second(b))
        for op in ops:
            ops_seen[op[0]] += 1
            if op[0] == "refused":
                refusals[op[1]] += 1
    print(dict(ops_seen), dict(pairs), dict(refusals))
    assert set(ops_seen) == set(cm.OPS)
    for name in cm.OPS:
        assert ops_seen[name] >= 5, (name, ops_seen[name])
    for kind in cm.REFUSALS:
        assert refusals[kind] >= 5, (kind, refusals[kind])
    for name in cm.PAIRS:
        assert pairs[name] >= 1, name
    flat = [op for _, ops in committed_sequences() for op in ops]
    assert {op[1] for op in flat if op[0] == "run_batch"} == {1, 2, 7}
    assert {op[1] for op in flat if op[0] == "iterate"} == {1, 2, 31, 32, 33}
    assert {op[1] for op in flat if op[0] == "spmm"} >= {1, 2, 3, 4, 5, 6, 16, 21}
    assert {op[1] for op in flat if op[0] == "spmspv"} == {"unique", "repeated", "empty"}
    assert {op[3] for op in flat if op[0] == "spmspv"} == {None, "sparse", "auto", "dense", "crossover"}
    assert {op[1] for op in flat if op[0] == "bind_result"} == {"A", "B", "V", None}
    runs = "".join("r" if op[0] == "run" else "." for op in flat)
    assert "r" * 9 in runs and ".r." in runs


_PLAYED = {}


def played(plan, seed):
    """the plan's sequence of `seed` in fixed point on the fake engine, once"""
    key = (plan.name, seed)
    if key not in _PLAYED:
        _PLAYED[key] = cm.play_sequence(cm.FakeBackend(), plan, 0, seed)
    return _PLAYED[key]


@pytest.mark.parametrize("plan", cm.PLANS, ids=lambda p: p.name)
def test_input_condition(plan):
    """Saturation must not hide errors: at every observation of every committed fixed-point sequence the model's y has fewer than 2 %
    saturated rows, fewer than 5 % zero rows among the rows that hold elements, and at least half of its words distinct.  (Looked at
    wherever the result target holds a product: a freshly loaded matrix's y is zero and a caller's buffer no step has written holds its
    fill pattern, both by contract; the in-place target is x as well and is measured through the other targets.)"""
    for seed in cm.SEEDS:
        p = played(plan, seed)
        assert p.observations >= 3 and len(p.conditions) >= 2
        _assert_condition(p, seed)


def _assert_condition(p, seed):
    for at, saturated, zero, distinct in p.conditions:
        assert saturated < 0.02 and zero < 0.05 and distinct >= 0.5, (p.label, seed, at, saturated, zero, distinct)


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_input_condition_of_the_two_engine_sequences(seed):
    """the same condition over both halves of the committed two-engine sequences (other generator seeds, iterate up to 33)"""
    for p in cm.play_two_engines(cm.FakeBackend(), 0, seed):
        assert p.observations >= 2 and p.conditions
        _assert_condition(p, seed)


def test_input_condition_sees_the_in_place_target():
    measured = 0
    for seed in cm.SEEDS:
        p = played(cm.PLAN["square-inplace"], seed)
        bound = None
        at_bound = set()
        for i, op in enumerate(p.done):
            if op[0] == "bind_result":
                bound = op[1]
            if op[0] == "reload":
                bound = None
            if bound == "V" and op[0] in ("read_result", "sync_copy"):
                at_bound.add(i + 1)
        measured += len(at_bound & {at for at, *_ in p.conditions})
    assert measured >= 2, measured


@pytest.mark.parametrize("impl", (1, 2))
def test_whole_op_table_in_the_float_modes_on_the_fake_engine(impl):
    for plan in (cm.PLAN["bitmap"], cm.PLAN["pairs-1"], cm.PLAN["square-inplace"]):
        for seed in cm.SEEDS:
            assert cm.play_sequence(cm.FakeBackend(), plan, impl, seed).observations >= 3
    for seed in cm.SEEDS:
        a, b = cm.play_two_engines(cm.FakeBackend(), impl, seed)
        assert a.observations >= 2 and b.observations >= 2


@pytest.mark.parametrize("defect", sorted(cm.DEFECTS))
def test_teeth_each_planted_defect_is_reported(defect):
    caught = []
    for plan in cm.PLANS:
        for seed in cm.SEEDS:
            if caught:
                break                         # (the first report is enough: each sequence costs a few tenths of a second)
            try:
                cm.play_sequence(cm.FakeBackend(defect), plan, 0, seed)
            except cm.Mismatch as e:
                text = str(e)
                assert f"plan {plan.name}, impl 0, seed {seed}" in text and "ops = [" in text
                caught.append((plan.name, seed, text.splitlines()[0]))
    print(defect, cm.DEFECTS[defect], caught)
    assert caught, f"no committed fixed-point sequence reports defect ({defect}): {cm.DEFECTS[defect]}"


def test_a_mismatch_names_the_buffer_the_row_and_the_replay():
    class Off(cm.FakeBackend):
        def engine(self, impl, ob_bank, vb_bank):
            eng = super().engine(impl, ob_bank, vb_bank)
            run = eng.run

            def off_by_one():
                run()
                eng.m.y_dst.w[5] ^= 1
            eng.run = off_by_one
            return eng
    with pytest.raises(cm.Mismatch) as e:
        cm.play_sequence(Off(), cm.PLAN["pairs-1"], 0, 0)
    text = str(e.value)
    assert "first at word 5" in text and "expected 0x" in text and "observed 0x" in text and "buffer" in text
    ops = eval(text.split("ops = ", 1)[1])
    with pytest.raises(cm.Mismatch):
        cm.replay(Off(), "pairs-1", 0, 0, ops[:-1] if ops[-1] == ("finish",) else ops)
    cm.replay(cm.FakeBackend(), "pairs-1", 0, 0, [op for op in ops if op != ("finish",)])


def test_an_unexpected_hip_error_is_a_device_fault():
    class Faulting(cm.FakeBackend):
        def engine(self, impl, ob_bank, vb_bank):
            eng = super().engine(impl, ob_bank, vb_bank)

            def run():
                raise device.DeviceError(cm.HIP_ERROR, "an illegal memory access was encountered")
            eng.run = run
            return eng
    with pytest.raises(cm.DeviceFault):
        cm.play_sequence(Faulting(), cm.PLAN["pairs-1"], 0, 0)


@pytest.mark.parametrize("where", ["first_load", "reload", "set_option", "create", "device_result", "spmspv_status", "plan_info"])
def test_a_hip_error_outside_the_op_calls_is_a_device_fault_too(where):
    """an asynchronous fault surfaces in the next synchronising call, whichever it is: the loads, the reads behind them, hs_create,
    hs_set_option and hs_spmspv_status included"""
    def hip_error(*a, **k):
        raise device.DeviceError(cm.HIP_ERROR, "an illegal memory access was encountered")

    class Faulting(cm.FakeBackend):
        loads = 0

        def engine(self, impl, ob_bank, vb_bank):
            if where == "create":
                hip_error()
            eng = super().engine(impl, ob_bank, vb_bank)
            load = eng.load_matrix_csr

            def counted(*a, **k):
                self.loads += 1
                if where == "first_load" or (where == "reload" and self.loads > 1):
                    hip_error()
                return load(*a, **k)
            eng.load_matrix_csr = counted
            if where == "set_option":
                eng.set_option = hip_error
            if where == "device_result":
                eng.device_result = hip_error
            return eng

        def spmspv_status(self, eng):
            return hip_error() if where == "spmspv_status" else super().spmspv_status(eng)

        def plan_info(self, eng, plan, impl, mat):
            return hip_error() if where == "plan_info" else {}
    ops = [("load_vector", 1), ("run",), ("run",), ("reload", False), ("load_csc", True), ("spmspv_overflow", False), ("read_result",)]
    cm.replay(cm.FakeBackend(), "pairs-1", 0, 0, ops)
    with pytest.raises(cm.DeviceFault):
        cm.replay(Faulting(), "pairs-1", 0, 0, ops)


@pytest.mark.parametrize("plan", [p for p in cm.PLANS if p.fmt], ids=lambda p: p.name)
def test_plans_take_their_forced_format_at_256_workgroups(plan):
    """the host builder's plan for the plan's matrix and options (what the device test asserts through hs_get_stats; `planner` forces
    nothing and is asserted on the device to be a known format)"""
    for impl in (0, 1):
        mat = cm.plan_matrix(plan, impl)
        cp = mat.cp()
        with ov.environment(plan.options):
            tiles = device.build_tiles(cp, impl, cp.ob_bank, cp.vb_bank, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, ov.WORKGROUPS)
        assert tiles["format"] == plan.fmt, (plan.name, tiles["format"])
        if plan.slices:
            assert tiles["col_slices"] == plan.slices, (plan.name, tiles["col_slices"])
    if plan.name == "pairs-1":       # a one-slice plan whose blocks reach over row-partition borders: hs_run_partition goes through partition_y
        b = tiles["blocks"]
        per = 128 * cm.OB_BANK
        assert (b["row0"] // per != (b["row0"] + np.maximum(b["nrows"], 1) - 1) // per).any() and cp.num_row_partitions >= 3


CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
from hisparse_amd import device
import context_model as cm

class CpuLibrary:
    memory = None
    no_options = True
    float_contract = False          # host threads add in another order: bit exact in fixed point, 1e-4 in the float modes
    def engine(self, impl, ob_bank, vb_bank):
        return device.SpmvEngine(impl, ob_bank=ob_bank, vb_bank=vb_bank)
    def packets(self, mat):
        return mat.cp()
    def update_values_raw(self, eng, values, nnz):
        return device.lib().hs_update_values(eng._h, values.ctypes.data, nnz)

played = 0
for name in ("pairs-1", "bitmap", "light"):
    for impl in cm.IMPLS:
        for seed in cm.SEEDS:
            p = cm.play_sequence(CpuLibrary(), cm.PLAN[name], impl, seed, flavour="cpu")
            assert p.observations >= 3
            played += 1
with device.SpmvEngine(0, ob_bank=cm.OB_BANK, vb_bank=cm.VB_BANK) as eng:
    mat = cm.plan_matrix(cm.PLAN["pairs-1"], 0)
    eng.load_matrix_csr((mat.rows, mat.cols, mat.indptr, mat.indices, mat.data))
    eng.load_vector(cm.x_words(0, mat.cols, 1))
    x = np.zeros(4, dtype=np.uint32)
    extensions = [lambda: eng.feedback(0, 0), lambda: eng.iterate(1, 0, 0), lambda: eng.set_option("batch_graph", "1"), lambda: eng.set_stream(None),
                  lambda: eng.get_stream(), lambda: eng.bind_device_result(None), lambda: eng.bind_device_vector(None), lambda: eng.device_result(),
                  lambda: eng.push_result([16], 4), lambda: eng.spmm(np.zeros((1, mat.cols), dtype=np.uint32)), lambda: eng.spmspv_async(x[:1], x[:1]),
                  lambda: eng.spmspv_device(16, 1), lambda: eng.load_matrix_csc(x[:2], x[:1], x[:1], 1), lambda: eng.update_values_device(16, mat.nnz)]
    for call in extensions:
        try:
            call()
            raise SystemExit("an extension answered on the CPU backend")
        except device.DeviceError as e:
            assert e.code == cm.UNSUPPORTED, e
print("sequences on the cpu library ok", played)
"""


def test_driver_on_the_cpu_library():
    """The subset libhisparse_cpu.so implements (load, CSR and transposed load, load_vector, run, run_batch, run_partition, read_result,
    update_values, time_runs), in a child process through HISPARSE_HIP_LIB; the extensions answer HS_ERR_UNSUPPORTED."""
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sequences on the cpu library ok 27" in r.stdout, r.stdout + r.stderr


def test_every_entry_point_is_an_op_or_excluded_with_a_reason():
    """The ratchet: a new hs_* prototype of include/hisparse_hip.h, or a new public method of device.SpmvEngine, is an op of the table or
    named in an exclusion dict with its reason."""
    protos = cm.header_entry_points()
    assert len(protos) >= 43 and "hs_run" in protos and "hs_tiles_free" in protos and set(device.EXPORTS) == set(protos)
    op_points = {v for v in cm.OPS.values() if v}
    covered = op_points | set(cm.ALSO_REACHED) | set(cm.EXCLUDED_ENTRY_POINTS)
    assert covered <= set(protos), covered - set(protos)                                   # nothing stale
    assert not op_points & set(cm.EXCLUDED_ENTRY_POINTS) and not set(cm.ALSO_REACHED) & set(cm.EXCLUDED_ENTRY_POINTS)
    for name in protos:
        assert name in covered, f"{name} is neither reached by an op of tests/context_model.py nor in EXCLUDED_ENTRY_POINTS"
    assert all(reason for reason in list(cm.EXCLUDED_ENTRY_POINTS.values()) + list(cm.ALSO_REACHED.values()) + list(cm.EXCLUDED_METHODS.values()))
    methods = {n for n, f in inspect.getmembers(device.SpmvEngine, inspect.isfunction) if not n.startswith("_")}
    assert set(cm.EXCLUDED_METHODS) <= methods
    players = {n[3:] for n, _ in inspect.getmembers(cm.Player, inspect.isfunction) if n.startswith("op_")}
    assert players == set(cm.OPS)                                                           # every op has its handler and the other way round
    for name in methods:
        assert name in cm.OPS or name in cm.EXCLUDED_METHODS, f"SpmvEngine.{name} is neither an op nor in EXCLUDED_METHODS"
    fake = {n for n, f in inspect.getmembers(cm.FakeEngine, inspect.isfunction) if not n.startswith("_")}
    assert {n for n in methods if n in cm.OPS} <= fake                                      # the fake engine answers every op's method
