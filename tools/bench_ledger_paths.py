"""Account paths at the workload's size: cstark_ledger_open_accounts and cstark_account_check_paths against the per-level launches of a
ledger apply (the same merges) and against the same folds on this machine's CPU.  Prints one JSON line.  Run on a GPU box.

    python tools/bench_ledger_paths.py [--min-seconds 1.0] [--out profiles/ledger_paths_bench.json]
        golden_1024_d15:    the 1,996 accounts of the committed witness (tests/golden/witness_1024_d15.npz) in a ledger of depth 15:
                            open_ms = host clock around Ledger.open, check_ms = around AccountOpening.check (values and presence given:
                            the leaf hash runs); both calls are synchronous; warm-up first, then at least --min-seconds of calls
        synthetic_d31 / synthetic_d15: check_ms of 2,048 paths and of ONE path of seeded reduced words in digest mode (a path is a
                            latency chain: one should take about what 2,048 take), folded roots compared with the host's
        host_fold_s:        the SAME 2,048 paths folded by the host `merge` of hostgadgets.h (tests/cpp/ledger_open_check.cpp --time,
                            g++ -O2), one path after the other
    python tools/bench_ledger_paths.py --trace-run 5
        five checks of 2,048 paths at depth 15 and five applies of the 1024-transfer batch at depth 15 (16 k_ledger_merge launches of
        2,048 merges each: the same 32,768 merges) and nothing else: the program to put behind
        `rocprofv3 --kernel-trace --output-format csv -d DIR --`
    python tools/bench_ledger_paths.py --kernel-trace DIR/.../*_kernel_trace.csv [--out ...]
        folds such a trace into device time: k_path_check against the sixteen k_ledger_merge launches of one apply"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

P = 2**62 + 2**56 + 2**55 + 1


def timed(fn, min_seconds, warmup=3):
    for _ in range(warmup):
        fn()
    samples = []
    t_end = time.perf_counter() + min_seconds
    while time.perf_counter() < t_end or len(samples) < 5:
        t0 = time.perf_counter()
        fn()
        samples.append(time.perf_counter() - t0)
    return {"median": round(1e3 * statistics.median(samples), 4), "min": round(1e3 * min(samples), 4), "max": round(1e3 * max(samples), 4),
            "repeats": len(samples)}


def synthetic(count, depth, seed=0x9A7B):
    """(indices, paths): seeded reduced words that are no tree's; the fold costs what a real path's costs"""
    rng = np.random.default_rng(seed + depth)
    indices = rng.integers(0, 1 << depth, count, dtype=np.uint64)
    paths = rng.integers(0, P, (count, depth + 1, 7), dtype=np.uint64)
    return indices, paths


def golden_ledger(backend):
    import ledger_cases as LC
    from certificate_stark_amd.prover import Ledger
    w = LC.golden_1024()
    indices, initial = LC.initial_accounts(w)
    led = Ledger(w.depth, backend)
    led.set_accounts(indices, initial)
    return w, led, indices, initial


def bench_golden(backend, min_seconds):
    w, led, indices, initial = golden_ledger(backend)
    o = led.open(indices)
    assert np.array_equal(o.root, w.initial_roots[0]) and np.array_equal(o.values, initial) and o.present.all() and not o.check().any()
    out = {"accounts": int(len(indices)), "depth": int(w.depth), "merges_per_check": int(len(indices)) * (int(w.depth) + 1)}
    out["open_ms"] = timed(lambda: led.open(indices), min_seconds)
    out["check_ms"] = timed(o.check, min_seconds)
    led.close()
    return out


def host_fold(indices, paths, tmp):
    """-> (seconds, roots) of the stand-alone host program on these paths"""
    exe, path = os.path.join(tmp, "ledger_open_check"), os.path.join(tmp, "paths_%d.bin" % (paths.shape[1] - 1))
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_open_check.cpp")])
    with open(path, "wb") as f:
        for a in (np.array([len(indices), paths.shape[1] - 1], np.uint64), indices, paths):
            f.write(np.ascontiguousarray(a, "<u8").tobytes())
    res = subprocess.run([exe, "--time", path], capture_output=True, text=True)
    if res.returncode != 0 or "seconds=" not in res.stdout:
        raise RuntimeError("host fold failed: " + res.stdout + res.stderr)
    return float(res.stdout.split("seconds=")[1].split()[0]), np.fromfile(path + ".roots", np.uint64).reshape(-1, 7)


def bench_synthetic(backend, depth, min_seconds, tmp):
    indices, paths = synthetic(2048, depth)
    root = np.zeros(7, np.uint64)
    verdicts, folded = backend.account_check_paths(indices, paths, root, want_roots=True)
    assert (verdicts == backend.PATH_ROOT).all()
    out = {"depth": depth, "merges": 2048 * depth}
    if tmp is not None:
        seconds, host_roots = host_fold(indices, paths, tmp)
        assert np.array_equal(host_roots, folded), "the host's folds differ from the device's"
        out["host_fold_s"] = round(seconds, 4)
        out["host_us_per_merge"] = round(1e6 * seconds / (2048 * depth), 2)
    out["check_2048_ms"] = timed(lambda: backend.account_check_paths(indices, paths, root), min_seconds)
    out["check_1_ms"] = timed(lambda: backend.account_check_paths(indices[:1], paths[:1], root), min_seconds)
    if tmp is not None:
        out["speedup_vs_host_2048"] = round(1e3 * out["host_fold_s"] / out["check_2048_ms"]["median"], 1)
    return out


def trace_run(backend, repeats):
    w, led, indices, initial = golden_ledger(backend)
    tr = tuple(getattr(w, f) for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))
    idx, paths = synthetic(2048, 15)
    root = np.zeros(7, np.uint64)
    for _ in range(repeats):
        backend.account_check_paths(idx, paths, root)
        led.set_accounts(indices, initial)
        led.apply(tr, want_witness=False)
    led.close()


def fold_trace(path):
    check, merge = [], []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            row = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0))
            if "k_path_check" in name:
                check.append(row)
            elif "k_ledger_merge" in name:
                merge.append(row)
    check.sort()
    merge.sort()
    # the apply's launches are those of 2,048 merges, the largest grid in the trace: set_accounts hashes 1,996 leaves and fewer parents
    largest = max(m[2] for m in merge)
    full = [m for m in merge if m[2] == largest]
    out = {"k_path_check": {"launches": len(check), "last_us": round((check[-1][1] - check[-1][0]) / 1e3, 2),
                            "median_us": round(statistics.median(e - s for s, e, _ in check) / 1e3, 2)}}
    out["k_ledger_merge_2048"] = {"launches": len(full), "median_us": round(statistics.median(e - s for s, e, _ in full) / 1e3, 2),
                                  "last_sixteen_us": round(sum(e - s for s, e, _ in full[-16:]) / 1e3, 2),
                                  "last_sixteen_span_us": round((full[-1][1] - full[-16][0]) / 1e3, 2)}
    out["check_over_sixteen_merge_launches"] = round(out["k_path_check"]["median_us"] / (16 * out["k_ledger_merge_2048"]["median_us"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_trace:
        result = {"kernel_trace_2048_d15": fold_trace(args.kernel_trace)}
    else:
        from certificate_stark_amd.backend import Backend
        b = Backend()
        if args.trace_run:
            trace_run(b, args.trace_run)
            result = {"trace_run": args.trace_run}
        else:
            result = {"config": "cstark_ledger_open_accounts and cstark_account_check_paths, MI355X; host clock around the synchronous calls"}
            result["golden_1024_d15"] = bench_golden(b, args.min_seconds)
            with tempfile.TemporaryDirectory() as tmp:
                for depth in (31, 15):
                    result["synthetic_d%d" % depth] = bench_synthetic(b, depth, args.min_seconds, None if args.no_baseline else tmp)
        b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
