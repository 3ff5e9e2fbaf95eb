"""hs_load_matrix wall time on a named config, three loads in one process (the first pays the code-object loads):
python tools/load_time.py <config>   (HISPARSE_PLAN_DEBUG=1 prints the phases, HISPARSE_RETILE=host the host builder)
python tools/load_time.py <config> --transpose [--loads N]
    A^T three ways, the median of N (5) loads each after one warm-up load: (a) hs_load_matrix_csr of A, (b) hs_load_matrix_csr_transposed of A,
    (c) what a caller did before it existed: transpose on the host (scipy's .T.tocsr(), and the library's own hsf_csr_to_csc), then
    hs_load_matrix_csr of the result.  Load times are hs_stats.load_seconds (the library's own clock around the load)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hisparse_amd import host, device, datasets

name = sys.argv[1]
cfg, csr = datasets.load(name)
impl = host.impl_id(cfg.impl)
if "--transpose" in sys.argv:
    import numpy as np
    import scipy.sparse as sp
    loads = int(sys.argv[sys.argv.index("--loads") + 1]) if "--loads" in sys.argv else 5
    ip, ix, dv = csr.arrays()
    rows, cols = csr.num_rows, csr.num_cols
    A = (rows, cols, ip, ix, dv)

    def median_ms(eng, arrays, transpose):
        eng.load_matrix_csr(arrays, transpose=transpose)                 # warm-up
        ms = []
        for _ in range(loads):
            eng.load_matrix_csr(arrays, transpose=transpose)
            ms.append(eng.stats()["load_seconds"] * 1e3)
        return float(np.median(ms)), ms

    t0 = time.perf_counter()
    mt = sp.csr_matrix((dv, ix, ip), shape=(rows, cols)).T.tocsr()
    scipy_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host.csr_to_csc(csr, impl)
    own_ms = (time.perf_counter() - t0) * 1e3
    AT = (cols, rows, mt.indptr.astype(np.uint32), mt.indices.astype(np.uint32), mt.data)
    with device.SpmvEngine(impl) as eng:
        a, a_all = median_ms(eng, A, False)
        fmt_a = device.STREAM_FORMATS[eng.stats()["stream_format"]]
        b, b_all = median_ms(eng, A, True)
        fmt_t = device.STREAM_FORMATS[eng.stats()["stream_format"]]
        at, at_all = median_ms(eng, AT, False)
    fmt = lambda v: " ".join("%.1f" % x for x in v)
    print("%-16s nnz %d, %s; A^T: %s" % (name, dv.size, fmt_a, fmt_t))
    print("  (a) hs_load_matrix_csr(A)                 %8.1f ms   [%s]" % (a, fmt(a_all)))
    print("  (b) hs_load_matrix_csr_transposed(A)      %8.1f ms   [%s]   (b)/(a) = %.2f" % (b, fmt(b_all), b / a))
    print("      hs_load_matrix_csr(host-transposed)   %8.1f ms   [%s]" % (at, fmt(at_all)))
    print("  (c) scipy .T.tocsr() %.1f ms + that load   %8.1f ms   (b)/(c) = %.3f" % (scipy_ms, scipy_ms + at, b / (scipy_ms + at)))
    print("  (c) hsf_csr_to_csc %.1f ms + that load     %8.1f ms   (b)/(c) = %.3f" % (own_ms, own_ms + at, b / (own_ms + at)), flush=True)
    sys.exit(0)
cp = host.format_matrix(csr, impl, skip_empty_rows=cfg.skip_empty_rows)
if os.environ.get("LOAD_CSR"):       # hs_load_matrix_csr: no csr2cpsr at all
    with device.SpmvEngine(impl) as eng:
        for k in range(3):
            print("---- CSR load %d" % k, file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            eng.load_matrix_csr(csr)
            wall = time.perf_counter() - t0
            st = eng.stats()
            print("%-16s CSR load %d: %.1f ms (python wall %.1f ms incl. the array copies out of the CSR handle), %s, image %.1f MB" % (
                name, k, st["load_seconds"] * 1e3, wall * 1e3, device.STREAM_FORMATS[st["stream_format"]], st["stream_bytes"] / 1e6), flush=True)
    sys.exit(0)
with device.SpmvEngine(impl) as eng:
    for k in range(3):
        print("---- load %d" % k, file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        eng.load_matrix(cp)
        wall = time.perf_counter() - t0
        st = eng.stats()
        print("%-16s load %d: %.1f ms (python wall %.1f ms), %s re-tile, %s, image %.1f MB, CPSR %.1f MB" % (
            name, k, st["load_seconds"] * 1e3, wall * 1e3, "gpu" if st["retiled_on_gpu"] else "host",
            device.STREAM_FORMATS[st["stream_format"]], st["stream_bytes"] / 1e6, st["cpsr_bytes"] / 1e6), flush=True)
