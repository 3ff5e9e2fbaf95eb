"""The cases of the row softmax (include/hisparse_rows.h), shared by tests/test_rows_cpu.py (libhisparse_cpu.so, in a child process) and
tests/test_gpu_rows.py (the HIP library, on the device): float64 references stated from the header, the bounds of its ARITHMETIC block,
and the general / exact / non-finite / edge / refusal cases written against the memory interface of tests/pattern_cases.py.

References.  Forward: t = float32(scale) * s and d = t - max_row t in fp32 (numpy float32: the words the header defines), E = exp(d)
in float64, P = E / math.fsum(E) per row, and |p - P| <= 3 * 2^-23 * P + 2^-125; an entry with d = -inf must be exactly 0; a row that holds
a NaN, a +inf or only -inf must be NaN in every entry.  Backward: the products p gp in float64 (exact), D = math.fsum of a row's
products, G = scale p (gp - D) in float64, A = fsum |p gp|, and |gs - G| <= 2^-23 |G| + |scale| p (n + 4) 2^-52 (A + |gp|) + 2^-149.
Every check returns the largest error / bound it saw."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import rows

from pattern_cases import HipMemory, HostMemory  # noqa: F401  (the test files take them from here)

BAD_ARG, BAD_MATRIX = -1, -4
FILL = 0xDEADBEEF
LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256, 257, 1023, 1024, 1025, 5000)
CONFIGS = ((1.0, 4.0), (0.125, 300.0), (-2.5, 30.0), (1.0, 1e4))      # (scale, score magnitude)


# ---- references --------------------------------------------------------------------------------------------------------------------
def indptr_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint32)


def entry_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(np.asarray(indptr, dtype=np.int64)))


def row_sums(indptr, x64):
    """math.fsum of every row: the correctly rounded sums"""
    xs, ip = np.asarray(x64, dtype=np.float64).tolist(), np.asarray(indptr, dtype=np.int64).tolist()
    return np.array([math.fsum(xs[ip[i]: ip[i + 1]]) for i in range(len(ip) - 1)], dtype=np.float64)


def forward_reference(indptr, s, scale):
    """(P in float64, rows that must be NaN (per entry), entries that must be exactly 0)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    s = np.asarray(s, dtype=np.float32)
    of = entry_rows(indptr)
    starts = indptr[:-1][np.diff(indptr) > 0]
    with np.errstate(all="ignore"):
        t = np.float32(scale) * s                                     # one fp32 multiply
        m = np.full(len(indptr) - 1, -np.inf, dtype=np.float32)
        nan_row = np.zeros(len(indptr) - 1, dtype=bool)
        if s.size:
            live = np.diff(indptr) > 0
            m[live] = np.fmax.reduceat(t, starts)                      # exact; a NaN is never the maximum
            nan_row[live] = np.add.reduceat(np.isnan(t).astype(np.int64), starts) > 0
        bad = (nan_row | np.isinf(m))[of]                              # a NaN, a +inf, or only -inf
        d = t - m[of]                                                  # one fp32 subtract
        E = np.where(bad, 0.0, np.exp(d.astype(np.float64)))
        S = row_sums(indptr, E)
        P = np.where(bad, np.nan, E / np.where(bad, 1.0, S[of]))
    return P, bad, ~bad & np.isneginf(d)


def forward_check(indptr, s, scale, p, what):
    p = np.asarray(p, dtype=np.float32)
    P, bad, zero = forward_reference(indptr, s, scale)
    assert p.shape == P.shape, (what, p.shape, P.shape)
    assert np.isnan(p[bad]).all(), f"{what}: {int((~np.isnan(p[bad])).sum())} entries of rows with a NaN, a +inf or only -inf are not NaN"
    good = ~bad
    assert np.isfinite(p[good]).all(), f"{what}: non-finite words in finite rows"
    assert not p[zero].any(), f"{what}: a -inf score under a finite maximum does not give exactly 0"
    err = np.abs(p[good].astype(np.float64) - P[good])
    bound = 3.0 * 2.0 ** -23 * P[good] + 2.0 ** -125
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: forward error / bound = {ratio:.3f} over {int(good.sum())} entries")
    assert ratio <= 1.0, f"{what}: {int((err > bound).sum())} entries break the forward bound, worst error / bound = {ratio:.3f}"
    return ratio


def backward_check(indptr, p, gp, scale, gs, what):
    indptr = np.asarray(indptr, dtype=np.int64)
    of = entry_rows(indptr)
    p64, g64, got = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, gp, gs))
    assert got.shape == p64.shape, (what, got.shape, p64.shape)
    prod = p64 * g64                                                   # exact in float64
    D, A = row_sums(indptr, prod), row_sums(indptr, np.abs(prod))
    sc = float(np.float32(scale))
    G = sc * p64 * (g64 - D[of])
    n = np.diff(indptr)[of]
    bound = 2.0 ** -23 * np.abs(G) + abs(sc) * p64 * (n + 4) * 2.0 ** -52 * (A[of] + np.abs(g64)) + 2.0 ** -149
    assert np.isfinite(got).all(), f"{what}: non-finite gradient words"
    err = np.abs(got - G)
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: backward error / bound = {ratio:.3f} over {err.size} entries")
    assert ratio <= 1.0, f"{what}: {int((err > bound).sum())} entries break the backward bound, worst error / bound = {ratio:.3f}"
    return ratio


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def general_lengths():
    """every length of LENGTHS (each class border on both sides) and 200 random ones in 0 ... 39, shuffled with a fixed seed so that the
    classes interleave; an empty row is moved to each end"""
    rng = np.random.default_rng(20261018)
    lengths = np.array(list(LENGTHS) + list(rng.integers(0, 40, 200)), dtype=np.int64)
    rng.shuffle(lengths)
    zeros = np.nonzero(lengths == 0)[0]
    assert zeros.size >= 2
    for at, z in ((0, zeros[0]), (lengths.size - 1, zeros[-1])):
        lengths[at], lengths[z] = lengths[z], lengths[at]
    assert lengths[0] == 0 and lengths[-1] == 0 and 12000 < lengths.sum() < 14000
    return lengths


def scores(n, magnitude, seed):
    return np.random.default_rng(seed).uniform(-magnitude, magnitude, n).astype(np.float32)


def grads(n, seed):
    return np.random.default_rng(seed).normal(0.0, 3.0, n).astype(np.float32)


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_forward(mem, rs, s, scale, in_place=False):
    """hsr_softmax_device over fresh buffers; returns (p, the words s's buffer holds afterwards)"""
    bs = mem.alloc(words(s))
    bp = bs if in_place else mem.alloc(np.full(rs.nnz, FILL, dtype=np.uint32))
    rs.softmax_device(bs.ptr, scale, bp.ptr)
    return mem.read(rs, bp).view(np.float32), mem.read(rs, bs).view(np.float32)


def device_backward(mem, rs, p, gp, scale, in_place=False):
    bp, bg = mem.alloc(words(p)), mem.alloc(words(gp))
    bo = bg if in_place else mem.alloc(np.full(rs.nnz, FILL, dtype=np.uint32))
    rs.softmax_backward_device(bp.ptr, bg.ptr, scale, bo.ptr)
    out = mem.read(rs, bo).view(np.float32)
    assert np.array_equal(mem.read(rs, bp), words(p)) and (in_place or np.array_equal(mem.read(rs, bg), words(gp))), "an input was written"
    return out


def both_ways(mem, rs, indptr, s, gp, scale, what):
    """forward and backward, host form and device form, out of place and in place: every word inside its bound, all forms the same words.
    Returns (p, gs)."""
    p = rs.softmax(s, scale)
    forward_check(indptr, s, scale, p, what + ", host form")
    dev, kept = device_forward(mem, rs, s, scale)
    forward_check(indptr, s, scale, dev, what + ", device form")
    assert np.array_equal(words(kept), words(s)), what + ": the scores were written"
    assert np.array_equal(words(dev), words(p)), what + ": device form and host form differ"
    inp, _ = device_forward(mem, rs, s, scale, in_place=True)
    assert np.array_equal(words(inp), words(dev)), what + ": in place differs from out of place"
    gs = rs.softmax_backward(p, gp, scale)
    backward_check(indptr, p, gp, scale, gs, what + ", host form")
    gdev = device_backward(mem, rs, p, gp, scale)
    backward_check(indptr, p, gp, scale, gdev, what + ", device form")
    assert np.array_equal(words(gdev), words(gs)), what + ": backward device form and host form differ"
    ginp = device_backward(mem, rs, p, gp, scale, in_place=True)
    assert np.array_equal(words(ginp), words(gdev)), what + ": backward in place differs from out of place"
    return p, gs


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def general(mem):
    """about 13 000 entries in 223 rows of every class, four (scale, magnitude) pairs"""
    lengths = general_lengths()
    indptr = indptr_of(lengths)
    of = entry_rows(indptr)
    with rows.RowSoftmax(indptr) as rs:
        assert rs.nnz == int(lengths.sum()) and rs.num_rows == lengths.size
        for i, (scale, magnitude) in enumerate(CONFIGS):
            s, gp = scores(rs.nnz, magnitude, 100 + i), grads(rs.nnz, 200 + i)
            p, _ = both_ways(mem, rs, indptr, s, gp, scale, f"general, scale {scale}, magnitude {magnitude}")
            assert (p[lengths[of] == 1] == np.float32(1.0)).all()
    return indptr


def exact_answers(mem):
    lengths = general_lengths()
    indptr = indptr_of(lengths)
    of = entry_rows(indptr)
    with rows.RowSoftmax(indptr) as rs:
        s = scores(rs.nnz, 300.0, 301)
        want = np.array([1.0 / n for n in lengths[of].tolist()], dtype=np.float64).astype(np.float32)      # float32(1 / n)
        for got in (rs.softmax(s, 0.0), device_forward(mem, rs, s, 0.0)[0], device_forward(mem, rs, s, 0.0, in_place=True)[0]):
            assert np.array_equal(words(got), words(want)), "scale = 0 is not float32(1 / n) bit for bit"
        for scale, magnitude in CONFIGS:
            one = lengths[of] == 1
            for got in (rs.softmax(scores(rs.nnz, magnitude, 302), scale), device_forward(mem, rs, scores(rs.nnz, magnitude, 302), scale)[0]):
                assert one.sum() >= 5 and np.array_equal(words(got[one]), words(np.ones(int(one.sum())))), "a row of one entry is not 1.0f"
    indptr = indptr_of([2, 0, 2])
    s = np.array([0.0, -200.0, -200.0, 0.0], dtype=np.float32)
    with rows.RowSoftmax(indptr) as rs:
        for got in (rs.softmax(s, 1.0), device_forward(mem, rs, s, 1.0)[0]):
            assert got[0] == 1.0 and got[3] == 1.0 and 0.0 <= got[1] < 2.0 ** -126 and 0.0 <= got[2] < 2.0 ** -126, got


def non_finite(mem):
    """-inf entries under a finite maximum in rows of four classes; a NaN, a +inf and a row of only -inf, each in a group row and in a long
    row; every other row finite"""
    lengths = general_lengths()
    indptr = indptr_of(lengths)
    row_of_length = {int(n): int(np.nonzero(lengths == n)[0][0]) for n in LENGTHS if n}
    s = scores(int(lengths.sum()), 4.0, 401)
    rng = np.random.default_rng(402)
    masked = 0
    for n in (2, 17, 129, 1025, 5000):
        lo = int(indptr[row_of_length[n]])
        hit = rng.choice(n, max(1, n // 3), replace=False)
        s[lo + hit] = -np.inf
        masked += hit.size
    nan_rows = []
    for n, value in ((5, np.nan), (1023, np.nan), (9, np.inf), (1024, np.inf), (65, None), (257, None)):
        r = row_of_length[n]
        lo = int(indptr[r])
        nan_rows.append(r)
        if value is None:
            s[lo: lo + n] = -np.inf
        else:
            s[lo + n // 2] = value
    of = entry_rows(indptr)
    with rows.RowSoftmax(indptr) as rs:
        for scale in (1.0, 0.125):
            for got in (rs.softmax(s, scale), device_forward(mem, rs, s, scale)[0], device_forward(mem, rs, s, scale, in_place=True)[0]):
                forward_check(indptr, s, scale, got, f"non-finite scores, scale {scale}")
                assert np.array_equal(np.isnan(got), np.isin(of, nan_rows)), "NaN outside the six rows, or missing inside them"
                assert int((got == 0).sum()) >= masked


def edge_patterns():
    return [("nnz = 0", [0, 0, 0, 0, 0]), ("one row of one entry", [1]), ("all rows empty but the last", [0] * 49 + [7]),
            ("one row of 70 000 entries", [70000])]


def edges(mem):
    for name, lengths in edge_patterns():
        indptr = indptr_of(lengths)
        with rows.RowSoftmax(indptr) as rs:
            assert rs.nnz == sum(lengths) and rs.info()["nnz"] == rs.nnz
            s, gp = scores(rs.nnz, 30.0, 501), grads(rs.nnz, 502)
            if rs.nnz:
                both_ways(mem, rs, indptr, s, gp, 0.125, name)
                continue
            # nothing to do: the calls succeed and touch nothing
            assert rs.softmax(s, 1.0).size == 0 and rs.softmax_backward(s, s, 1.0).size == 0
            a, b, c = (mem.alloc(np.full(4, FILL + i, dtype=np.uint32)) for i in range(3))
            rs.softmax_device(a.ptr, 1.0, b.ptr)
            rs.softmax_device(a.ptr, 1.0, a.ptr)
            rs.softmax_backward_device(a.ptr, b.ptr, 1.0, c.ptr)
            for i, buf in enumerate((a, b, c)):
                assert (mem.read(rs, buf) == FILL + i).all(), name


def _create(num_rows, indptr):
    l = rows.lib()
    h = C.c_void_p(0xBAD)
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint32)
    return l.hsr_create(C.byref(h), 0, num_rows, None if indptr is None else indptr.ctypes.data), h


def refusals(mem):
    l = rows.lib()
    vp, f = C.c_void_p, C.c_float
    indptr = indptr_of([3, 0, 5, 1, 300])
    for what, args, code in (("no rows", (0, indptr), BAD_ARG), ("null indptr", (5, None), BAD_ARG),
                             ("indptr decreases", (5, [0, 3, 2, 8, 9, 309]), BAD_MATRIX), ("indptr[0] = 1", (5, [1, 3, 3, 8, 9, 309]), BAD_MATRIX)):
        rc, h = _create(*args)
        assert rc == code and not h.value and l.hsr_last_error(None), (what, rc, h.value)
    assert l.hsr_create(None, 0, 5, indptr.ctypes.data) == BAD_ARG and l.hsr_last_error(None)
    assert l.hsr_info(None, None, None) == BAD_ARG and l.hsr_sync(None) == BAD_ARG and l.hsr_set_stream(None, None) == BAD_ARG
    assert l.hsr_softmax_device(None, vp(16), f(1.0), vp(16)) == BAD_ARG and l.hsr_softmax_backward_device(None, vp(16), vp(32), f(1.0), vp(48)) == BAD_ARG
    assert l.hsr_softmax(None, vp(16), f(1.0), vp(16)) == BAD_ARG and l.hsr_softmax_backward(None, vp(16), vp(32), f(1.0), vp(48)) == BAD_ARG
    assert l.hsr_destroy(None) == 0
    with rows.RowSoftmax(indptr) as rs:
        n = rs.nnz
        s, gp = scores(n, 4.0, 601), grads(n, 602)
        want = rs.softmax(s, 0.5)
        forward_check(indptr, s, 0.5, want, "refusals")
        want_gs = rs.softmax_backward(want, gp, 0.5)
        backward_check(indptr, want, gp, 0.5, want_gs, "refusals")
        # two nnz-word ranges in each buffer, so that a partial overlap stays inside it
        bs, bp, bg = mem.alloc(np.zeros(2 * n, np.uint32)), mem.alloc(np.zeros(2 * n, np.uint32)), mem.alloc(np.zeros(2 * n, np.uint32))
        S, P, Gp = bs.ptr, bp.ptr, bg.ptr
        inf, nan = float("inf"), float("nan")

        def usable(what):
            assert np.array_equal(words(rs.softmax(s, 0.5)), words(want)) and np.array_equal(words(rs.softmax_backward(want, gp, 0.5)), words(want_gs)), f"unusable after {what}"

        for what, a in (("null s", (None, 1.0, P)), ("null p", (S, 1.0, None)), ("misaligned s", (S + 2, 1.0, P)), ("misaligned p", (S, 1.0, P + 1)),
                        ("scale inf", (S, inf, P)), ("scale -inf", (S, -inf, P)), ("scale NaN", (S, nan, P)),
                        ("p one word into s", (S, 1.0, S + 4)), ("p one word before s's end", (S, 1.0, S + 4 * (n - 1))), ("s one word into p", (P + 4, 1.0, P))):
            rc = l.hsr_softmax_device(rs._h, vp(a[0]), f(a[1]), vp(a[2]))
            assert rc == BAD_ARG and l.hsr_last_error(rs._h), (what, rc)
            usable(what)
        for what, a in (("null p", (None, Gp, 1.0, S)), ("null gp", (P, None, 1.0, S)), ("null gs", (P, Gp, 1.0, None)),
                        ("misaligned p", (P + 2, Gp, 1.0, S)), ("misaligned gp", (P, Gp + 3, 1.0, S)), ("misaligned gs", (P, Gp, 1.0, S + 1)),
                        ("scale inf", (P, Gp, inf, S)), ("scale NaN", (P, Gp, nan, S)),
                        ("gs is p", (P, Gp, 1.0, P)), ("gs one word into p", (P, Gp, 1.0, P + 4)), ("p one word into gs", (S + 4, Gp, 1.0, S)),
                        ("gs one word into gp", (P, Gp, 1.0, Gp + 4)), ("gp one word into gs", (P, S + 4, 1.0, S))):
            rc = l.hsr_softmax_backward_device(rs._h, vp(a[0]), vp(a[1]), f(a[2]), vp(a[3]))
            assert rc == BAD_ARG and l.hsr_last_error(rs._h), (what, rc)
            usable(what)
        # ranges that touch without sharing a word are fine
        rs.softmax_device(S, 1.0, S + 4 * n)
        rs.softmax_backward_device(P, Gp, 1.0, Gp + 4 * n)
        rs.sync()
        hs, hp, hg = np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32)
        H, Hp, Hg = hs.ctypes.data, hp.ctypes.data, hg.ctypes.data
        for what, a in (("host null s", (None, 1.0, Hp)), ("host null p", (H, 1.0, None)), ("host scale inf", (H, inf, Hp)), ("host overlap", (H, 1.0, H + 4))):
            assert l.hsr_softmax(rs._h, vp(a[0]), f(a[1]), vp(a[2])) == BAD_ARG and l.hsr_last_error(rs._h), what
            usable(what)
        for what, a in (("host null p", (None, Hg, 1.0, H)), ("host null gp", (Hp, None, 1.0, H)), ("host null gs", (Hp, Hg, 1.0, None)), ("host scale NaN", (Hp, Hg, nan, H)),
                        ("host gs is p", (Hp, Hg, 1.0, Hp)), ("host gs into gp", (Hp, Hg, 1.0, Hg + 4))):
            assert l.hsr_softmax_backward(rs._h, vp(a[0]), vp(a[1]), f(a[2]), vp(a[3])) == BAD_ARG and l.hsr_last_error(rs._h), what
            usable(what)
        rs.set_stream(None)
        rs.sync()


# ---- at scale (tests/test_gpu_rows.py) ------------------------------------------------------------------------------------------------
def checked_on_device(mem, indptr, scale, magnitude, seed, what):
    """one forward and one backward call through the device form over `indptr`, every word inside its bound"""
    indptr = np.asarray(indptr, dtype=np.uint32)
    with rows.RowSoftmax(indptr) as rs:
        s, gp = scores(rs.nnz, magnitude, seed), grads(rs.nnz, seed + 1)
        p, _ = device_forward(mem, rs, s, scale)
        forward_check(indptr, s, scale, p, what)
        gs = device_backward(mem, rs, p, gp, scale)
        backward_check(indptr, p, gp, scale, gs, what)
    return p, gs
