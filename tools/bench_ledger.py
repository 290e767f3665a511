"""The account ledger at the workload's size: cstark_ledger_apply of 1024 transfers against the sequential loop it replaces.  Two cases:
the committed witness (tests/golden/witness_1024_d15.npz, depth 15) and a generated one at depth 31.  Prints one JSON line.  Run on a
GPU box.

    python tools/bench_ledger.py [--min-seconds 1.0] [--out profiles/ledger_bench.json]
        apply_ms:           host clock around Ledger.apply (the call ends in a synchronise), witness left on the device; warm-up first,
                            then at least --min-seconds of applies; the ledger is reset by set_accounts outside the timed region
        apply_copy_ms:      the same with the eleven arrays copied back to the host
        set_accounts_ms:    the reset itself (bulk insert of every account)
        host_executor_s:    the SAME job lists run by the stand-alone host executor (tests/cpp/ledger_plan_check.cpp --time, g++ -O2) on
                            this machine's CPU: the loop the reference runs (src/lib.rs:341-422), one merge after the other
    python tools/bench_ledger.py --trace-run 5
        five applies per case and nothing else: the program to put behind `rocprofv3 --kernel-trace --output-format csv -d DIR --`
    python tools/bench_ledger.py --kernel-trace DIR/.../*_kernel_trace.csv [--out ...]
        folds such a trace into per-launch times: device time of the merge launches and of the gathers, and the gaps between them"""
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


def cases():
    import ledger_cases as LC
    from certificate_stark_amd.prover import TransactionMetadata
    return [("golden_1024_d15", LC.golden_1024()), ("generated_1024_d31", TransactionMetadata.build_random(1024, 31, seed=31))]


def transfers(w):
    return tuple(getattr(w, f) for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))


def time_case(backend, w, min_seconds, trace_run=0):
    import ledger_cases as LC
    from certificate_stark_amd.prover import Ledger
    indices, initial = LC.initial_accounts(w)
    led = Ledger(w.depth, backend)
    tr = transfers(w)
    out = {"n_tx": int(w.n_tx), "depth": int(w.depth), "accounts": int(len(indices)), "merges": 2 * int(w.n_tx) * (int(w.depth) + 1)}

    def run(want, repeats=None):
        apply_s, reset_s = [], []
        t_end = time.perf_counter() + min_seconds
        while (len(apply_s) < repeats) if repeats else (time.perf_counter() < t_end or len(apply_s) < 5):
            t0 = time.perf_counter()
            led.set_accounts(indices, initial)
            t1 = time.perf_counter()
            m = led.apply(tr, want_witness=want)
            t2 = time.perf_counter()
            reset_s.append(t1 - t0)
            apply_s.append(t2 - t1)
        return apply_s, reset_s, m

    if trace_run:
        run(False, trace_run)
        led.close()
        return out
    _, _, m = run(True, 3)  # warm-up; the arrays are the reference's
    assert np.array_equal(m.s_paths, w.s_paths) and np.array_equal(m.r_paths, w.r_paths) and np.array_equal(m.final_root, w.final_root)
    for name, want in (("apply_ms", False), ("apply_copy_ms", True)):
        a, r, _ = run(want)
        out[name] = {"median": round(1e3 * statistics.median(a), 4), "min": round(1e3 * min(a), 4), "max": round(1e3 * max(a), 4), "repeats": len(a)}
        out["set_accounts_ms"] = round(1e3 * statistics.median(r), 4)
    led.close()
    return out


def host_executor_seconds(w, tmp):
    import ledger_cases as LC
    exe, path = os.path.join(tmp, "ledger_plan_check"), os.path.join(tmp, "case.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_plan_check.cpp")])
    LC.write_case(path, w)
    res = subprocess.run([exe, path, "--time"], capture_output=True, text=True)
    if res.returncode != 0 or "seconds=" not in res.stdout:
        raise RuntimeError("host executor failed: " + res.stdout + res.stderr)
    return float(res.stdout.split("seconds=")[1].split()[0])


def fold_trace(path):
    """per apply of each case: the merge launches, the gathers, and the idle time between the first launch's start and the last one's end"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_ledger_" in name:
                rows.append(("merge" if "k_ledger_merge" in name else "gather", int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                             int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)))
    rows.sort(key=lambda x: x[1])
    # an apply is a run of merge launches followed by two gathers; set_accounts and ledger creation end without a gather pair
    applies, cur = [], []
    for r in rows:
        cur.append(r)
        if len(cur) >= 2 and cur[-1][0] == "gather" and cur[-2][0] == "gather":
            applies.append(cur)
            cur = []
        elif r[0] == "merge" and len(cur) >= 2 and cur[-2][0] == "gather":
            cur = [r]  # a single gather: not an apply
    by_shape = {}
    for a in applies:
        merges = [x for x in a if x[0] == "merge"]
        # --trace-run resets the ledger before every apply: depth + 1 launches of set_accounts, then the depth + 1 of the apply itself
        # (the first apply of a case also follows the ledger's creation: an odd count, left out)
        if len(merges) % 2:
            continue
        tail = merges[len(merges) // 2:]
        gathers = [x for x in a if x[0] == "gather"]
        span = gathers[-1][2] - tail[0][1]
        busy = sum(x[2] - x[1] for x in tail + gathers)
        by_shape.setdefault(len(tail), []).append({"merge_launches": len(tail), "merge_us_each": round(statistics.mean(x[2] - x[1] for x in tail) / 1e3, 2),
                                                   "merge_us_total": round(sum(x[2] - x[1] for x in tail) / 1e3, 2),
                                                   "gather_witness_us": round((gathers[0][2] - gathers[0][1]) / 1e3, 2),
                                                   "gather_commit_us": round((gathers[1][2] - gathers[1][1]) / 1e3, 2),
                                                   "span_us": round(span / 1e3, 2), "gaps_us": round((span - busy) / 1e3, 2)})
    out = {}
    for k, v in by_shape.items():
        last = v[-1]  # the last apply of a shape: everything warm
        last["applies_in_trace"] = len(v)
        out["depth_%d" % (k - 1)] = last
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
        result = {"kernel_trace": fold_trace(args.kernel_trace)}
    else:
        from certificate_stark_amd.backend import Backend
        b = Backend()
        result = {"config": "cstark_ledger_apply, 1024 transfers, MI355X; host clock around the synchronous call", "cases": {}}
        with tempfile.TemporaryDirectory() as tmp:
            for name, w in cases():
                r = time_case(b, w, args.min_seconds, args.trace_run)
                if not args.trace_run and not args.no_baseline:
                    r["host_executor_s"] = round(host_executor_seconds(w, tmp), 4)
                    r["host_us_per_merge"] = round(1e6 * r["host_executor_s"] / r["merges"], 2)
                    r["speedup_vs_host_executor"] = round(1e3 * r["host_executor_s"] / r["apply_ms"]["median"], 1)
                result["cases"][name] = r
        b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
