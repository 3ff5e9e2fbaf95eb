"""Byte identity of the host tile builder (hs_tiles_build: no GPU) between two builds of libhisparse_hip.so -- the gate of a refactor of
stream_tiles.cpp / stream_plan.h: every matrix must get the same plan, the same image bytes and the same tables.

    python tools/tiles_ab.py LIB_A LIB_B [--only GROUP,...] [--list] [--record FILE]

Every case runs in a child process once per library (HISPARSE_HIP_LIB, as hisparse_amd/device.py reads it at import; cases of one matrix
share the child, so the matrix is generated once per library), with HISPARSE_PLAN_DEBUG=1.  Compared per case, failing on the first
difference with the case and the field named: return code and error text, every scalar device.build_tiles returns, the bytes of image /
blocks / units / wg_first / block_order (length + SHA-256), and the builder's stderr with the numbers of the `re-tile ... ms` lines removed.
Run it with the same library on both sides first: a difference there means the build itself is not deterministic for that case.
The corpus reaches every branch of the planner a host build can reach (the list is GROUPS below); it takes minutes, it is not a test."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARK = "@@ tiles_ab case "
ARRAYS = ("image", "blocks", "units", "wg_first", "block_order")
IMPLS = ("fixed", "float_pob", "float_stall")
PLAN_KEYS = ("STREAM_FORMAT", "COL_SLICES", "MAX_ROWS", "LIGHT", "LIGHT_WGS", "SWEEP", "SPMM_VECTORS", "POW2_SLICES", "ROW_RUNS", "AUX_BITS", "DELTA_DEAL",
             "XCD_AFFINITY", "PLAN_CENSUS", "BITMAP_BUILD", "CROSS_PARTITIONS")


def V(tag, impl, env=None, wgs=256, banks=None, mutate=None):
    """one case of a group: numeric mode, plan switches (without the HISPARSE_ prefix), workgroups, (vb_bank, ob_bank), channel mutation"""
    return dict(tag=tag, impl=impl, env=env or {}, wgs=wgs, banks=banks, mutate=mutate)


def forced_variants(impl):
    f = [V(f"format={x}", impl, {"STREAM_FORMAT": x}) for x in ("pairs", "delta", "delta24", "delta32", "owner", "owner24", "bitmap", "sweep")]
    f += [V("aux_bits=24", impl, {"AUX_BITS": "24"}), V("aux_bits=24,format=pairs", impl, {"AUX_BITS": "24", "STREAM_FORMAT": "pairs", "COL_SLICES": "1"})]
    f += [V(f"col_slices={s}", impl, {"COL_SLICES": str(s)}) for s in (1, 2, 4, 7)]
    f += [V("max_rows=64", impl, {"MAX_ROWS": "64"}), V("max_rows=64,light=1", impl, {"MAX_ROWS": "64", "LIGHT": "1"}), V("light=0", impl, {"LIGHT": "0"}),
          V("light=1", impl, {"LIGHT": "1"}), V("light_wgs=2", impl, {"LIGHT_WGS": "2"}), V("light=1,light_wgs=2", impl, {"LIGHT": "1", "LIGHT_WGS": "2"}),
          V("row_runs=0", impl, {"ROW_RUNS": "0", "STREAM_FORMAT": "delta"}), V("row_runs=1", impl, {"ROW_RUNS": "1", "STREAM_FORMAT": "delta"}),
          V("row_runs=0,unforced", impl, {"ROW_RUNS": "0"}), V("row_runs=1,unforced", impl, {"ROW_RUNS": "1"}),
          V("delta_deal=wave", impl, {"DELTA_DEAL": "wave", "STREAM_FORMAT": "delta"}), V("plan_census=0", impl, {"PLAN_CENSUS": "0"}),
          V("pow2_slices=1", impl, {"POW2_SLICES": "1"}), V("sweep=0", impl, {"SWEEP": "0"}), V("sweep=1", impl, {"SWEEP": "1"}),
          V("spmm_vectors=4", impl, {"SPMM_VECTORS": "4"}),
          V("xcd_affinity=1,col_slices=2,wgs=64", impl, {"XCD_AFFINITY": "1", "COL_SLICES": "2"}, wgs=64),
          V("format=bogus", impl, {"STREAM_FORMAT": "bogus"}), V("unforced", impl),
          V("truncated channel", impl, mutate="truncate")]
    return f


def groups():
    """name -> (matrix builder, cases).  Builders return a scipy matrix or a host.CSRMatrix."""
    import planner_check as pc
    import scipy.sparse as sp
    from hisparse_amd import host
    g = {}
    for name, _, build in pc.CASES:      # every out-of-sample matrix of the planner check, in all three numeric modes
        g[name] = (build, [V(IMPLS[i], i) for i in range(3)])
    # HISPARSE_POW2_SLICES only acts in the cost loop of a wide (more than sixteen sub-tiles) non-OWNER matrix: these two take 5 and 6 slices without it
    for name in ("rmat19_45_15_15", "er_300k_30"):
        g[name][1].append(V("fixed,pow2_slices=1,light=0", 0, {"POW2_SLICES": "1", "LIGHT": "0"}))
    # the matrices of tests/test_planner_cpu.py
    g["t_banded_200k"] = (lambda: pc.banded(200_000, 20, 1_000, 1, 0), [V("fixed", 0), V("fixed,plan_census=0", 0, {"PLAN_CENSUS": "0"})])
    g["t_blockdiag_120k"] = (lambda: pc.block_diagonal(120_000, 512, 0.10, 3, 0), [V("fixed", 0)])
    g["t_hubs_200k"] = (lambda: pc.hubs(200_000, 12, 24, 80_000, 14, 0), [V("fixed", 0), V("float_pob", 1)])
    g["t_blockdiag_360k_float"] = (lambda: pc.block_diagonal(360_000, 64, 0.5, 4, 1), [V("float_pob", 1), V("float_stall", 2), V("fixed", 0)])
    g["t_wide_2k_x_4m"] = (lambda: pc.uniform(2_048, 4_000_000, 800, 27, 0), [V("fixed", 0)])
    g["t_mouse_gene_slab8"] = (lambda: pc.reference("mouse_gene_slab8"), [V("fixed", 0), V("float_pob", 1)])
    # 512 x 33 288 dense-row layers: the sliced-DELTA preference at both of its sites, LIGHT and BITMAP
    for pct in (5, 10, 20, 40):
        cases = [V("fixed", 0)] + ([V("float_pob", 1)] if pct == 20 else [])
        g[f"layer_512_x_33288_d{pct}"] = (lambda pct=pct: host.CSRMatrix.generate("bernoulli", 512, 33288, b=pct / 100.0, c=0.05, seed=100 - pct), cases)
    g["empty_matrix"] = (lambda: sp.csr_matrix((1024, 4096), dtype=np.float32), [V(IMPLS[i], i) for i in range(3)])
    g["one_row"] = (lambda: sp.csr_matrix((np.ones(300, dtype=np.float32), (np.zeros(300, dtype=np.int64), np.arange(0, 3000, 10))), shape=(1, 4096)),
                    [V(IMPLS[i], i) for i in range(3)])
    # every plan switch, on the power-law matrix of tests/test_tiles_cpu.py
    g["forced_powerlaw_fixed"] = (lambda: host.CSRMatrix.generate("powerlaw", 30000, 50000, a=600000, b=0.4, c=1.0, seed=3), forced_variants(0))
    g["forced_powerlaw_float"] = (lambda: host.CSRMatrix.generate("powerlaw", 30000, 50000, a=600000, b=0.4, c=2.0, seed=3), forced_variants(1))
    # hyper-sparse and too wide for LIGHT: OWNER24 by itself, the forced OWNER forms
    g["hypersparse_300k_x_400k"] = (lambda: host.CSRMatrix.generate("powerlaw", 300000, 400000, a=200000, b=0.4, c=1.0, seed=3),
                                    [V("fixed", 0), V("float_pob", 1), V("float_pob,format=owner", 1, {"STREAM_FORMAT": "owner"}),
                                     V("float_pob,format=owner24,col_slices=4", 1, {"STREAM_FORMAT": "owner24", "COL_SLICES": "4"}),
                                     V("fixed,format=owner24,max_rows=500", 0, {"STREAM_FORMAT": "owner24", "MAX_ROWS": "500"})])

    def many_partitions():
        import cases
        return cases.random_csr(2500, 300, 0.03, 21, 0)
    g["row_partitions"] = (many_partitions, [V("cross_partitions=0", 0, {"CROSS_PARTITIONS": "0"}, wgs=16, banks=(4, 1)),
                                             V("cross_partitions=1", 0, {"CROSS_PARTITIONS": "1"}, wgs=16, banks=(4, 1)),
                                             V("default", 0, wgs=16, banks=(4, 1))])

    def dense_with_duplicate():      # BITMAP refused (one column twice in a row) -> element streams
        rng = np.random.default_rng(7)
        rows, cols, per_row = 256, 4096, 1200
        ix = np.concatenate([np.sort(rng.choice(cols, per_row, replace=False)) for _ in range(rows)]).astype(np.uint32)
        ix[1] = ix[0]
        ip = (np.arange(rows + 1) * per_row).astype(np.uint32)
        return host.CSRMatrix.from_arrays(rows, cols, ip, ix, rng.uniform(0.0, 1.0, ix.size).astype(np.float32))
    g["dense_rows_with_duplicate"] = (dense_with_duplicate, [V("fixed", 0, wgs=16), V("float_pob", 1, wgs=16), V("fixed,format=bitmap", 0, {"STREAM_FORMAT": "bitmap"}, wgs=16)])
    return g


def child(group):
    """builds every case of one group with the library HISPARSE_HIP_LIB names; one JSON line per case on stdout, the builder's stderr between markers"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hisparse_amd import device, host
    build, cases = groups()[group]
    m = build()
    csr = m if isinstance(m, host.CSRMatrix) else host.CSRMatrix.from_scipy(m)
    packets = {}
    for v in cases:
        key = (v["impl"], v["banks"])
        if key not in packets:
            vb, ob = v["banks"] or (None, None)
            packets[key] = host.format_matrix(csr, v["impl"], vb_bank=vb, ob_bank=ob, skip_empty_rows=True)
        cp = packets[key]
        for k in PLAN_KEYS:
            os.environ.pop("HISPARSE_" + k, None)
        for k, val in v["env"].items():
            os.environ["HISPARSE_" + k] = val
        src = cp
        if v["mutate"] == "truncate":      # a channel shorter than its partition headers
            src = [cp.channel(c) for c in range(16)]
            src[3] = src[3][: cp.num_partitions * 2 - 1]
        sys.stderr.write(f"{MARK}{v['tag']}\n")
        sys.stderr.flush()
        res = {"tag": v["tag"], "rc": 0, "error": ""}
        try:
            t = device.build_tiles(src, v["impl"], cp.ob_bank, cp.vb_bank, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, v["wgs"])
            for k, val in t.items():
                if k in ARRAYS:
                    raw = np.ascontiguousarray(val).tobytes()
                    res[k] = f"{len(raw)} bytes sha256 {hashlib.sha256(raw).hexdigest()}"
                else:
                    res[k] = val
        except device.DeviceError as e:
            res["rc"], res["error"] = e.code, str(e)
        print(json.dumps(res), flush=True)


TIMES = re.compile(r"^(re-tile .*?)\s+[0-9.]+ ms$", re.M)


def run_child(lib, group):
    env = dict(os.environ, HISPARSE_HIP_LIB=os.path.abspath(lib), HISPARSE_PLAN_DEBUG="1")
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", group], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def parse(proc, out, err):
    if proc.returncode != 0:
        raise SystemExit(f"child failed ({proc.returncode}):\n{err[-2000:]}")
    results = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    logs = {}
    for piece in err.split(MARK)[1:]:
        tag, _, text = piece.partition("\n")
        logs[tag] = TIMES.sub(r"\1 # ms", text)
    return results, logs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--record", default=None, help="write the list of cases (format, slices, image bytes) and the verdict to this file")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    names = list(groups())
    if a.list:
        print("\n".join(names))
        return
    if len(a.libs) != 2:
        ap.error("LIB_A LIB_B")
    pick = a.only.split(",") if a.only else names
    lines, n = [], 0
    for group in pick:
        pa, pb = run_child(a.libs[0], group), run_child(a.libs[1], group)      # the two libraries side by side
        oa, ea = pa.communicate()
        ob, eb = pb.communicate()
        (ra, la), (rb, lb) = parse(pa, oa, ea), parse(pb, ob, eb)
        if len(ra) != len(rb):
            raise SystemExit(f"DIFFERENCE in {group}: {len(ra)} cases against {len(rb)}")
        for x, y in zip(ra, rb):
            case = f"{group} [{x['tag']}]"
            for field in sorted(set(x) | set(y)):
                if x.get(field) != y.get(field):
                    raise SystemExit(f"DIFFERENCE in {case}, field {field}:\n  A: {x.get(field)}\n  B: {y.get(field)}")
            if la.get(x["tag"]) != lb.get(x["tag"]):
                import difflib
                d = "\n".join(list(difflib.unified_diff(la.get(x["tag"], "").splitlines(), lb.get(x["tag"], "").splitlines(), "A", "B", lineterm=""))[:40])
                raise SystemExit(f"DIFFERENCE in {case}, field stderr:\n{d}")
            n += 1
            what = (f"{x['format']:8s} x{x['col_slices']:<2d} {x['image'].split()[0]:>11s} image bytes, {x['num_workgroups']} workgroups, {len(la.get(x['tag'], '').splitlines())} debug lines"
                    if x["rc"] == 0 else f"error {x['rc']}: {x['error'][:90]}")
            lines.append(f"{case:62s} {what}")
            print(lines[-1], flush=True)
    verdict = f"{n} cases, 0 differences"
    print(verdict)
    if a.record:
        with open(a.record, "w") as f:
            f.write("\n".join(lines + [verdict]) + "\n")


if __name__ == "__main__":
    main()
