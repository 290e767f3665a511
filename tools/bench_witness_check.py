"""cstark_tx_witness_check at the workload's size: the committed 1024-transfer depth-15 witness (tests/golden/witness_1024_d15.npz),
host clock around the synchronous call after warm-up, at least --min-seconds of calls each.  Prints one JSON line.  Run on a GPU box.

    python tools/bench_witness_check.py [--min-seconds 1.0] [--out profiles/witness_check_bench.json]
        host_ms / host_signed_ms:          TransactionMetadata.check of the host witness, without and with the signature test
        resident_ms / resident_signed_ms:  the same witness uploaded once, then checked where it lies (no upload, 1 KB down)
        validate_ms:                       TransactionExample.validate of the same witness (trace build and every constraint)
        prove_verify_ms:                   prove + verify of the same witness, example options
        ratios:                            each of the above over resident_ms
    python tools/bench_witness_check.py --trace-run 5
        five checks of the host witness and five cstark_account_check_paths calls of 4 * 1024 paths with values at depth 15 (the
        witness's own sender and receiver paths, twice: depth + 1 permutations per chain, as many chains) and nothing else: the program
        to put behind `rocprofv3 --kernel-trace --output-format csv -d DIR --`
    python tools/bench_witness_check.py --kernel-trace DIR/.../*_kernel_trace.csv [--merge FILE] [--out ...]
        folds such a trace into device time: k_witness_check over k_path_check; --merge: added to the JSON of a timing run"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


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


def golden():
    from certificate_stark_amd.prover import TransactionMetadata
    return TransactionMetadata.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))


def bench(backend, min_seconds):
    from certificate_stark_amd.prover import TransactionExample, get_example_options
    w = golden()
    first = w.check(backend, check_signatures=True)
    assert first.ok and np.array_equal(first.final_root, w.final_root), str(first)
    out = {"n_tx": w.n_tx, "depth": w.depth}
    out["host_ms"] = timed(lambda: w.check(backend), min_seconds)
    out["host_signed_ms"] = timed(lambda: w.check(backend, check_signatures=True), min_seconds)
    backend.upload_witness(w)
    report, verdicts = backend.tx_witness_check(final_root=w.final_root, check_signatures=True)
    assert report.first_bad == -1 and not verdicts.any()
    out["resident_ms"] = timed(lambda: backend.tx_witness_check(final_root=w.final_root), min_seconds)
    out["resident_signed_ms"] = timed(lambda: backend.tx_witness_check(final_root=w.final_root, check_signatures=True), min_seconds)
    ex = TransactionExample(get_example_options(), w, backend)
    assert ex.validate().ok
    out["validate_ms"] = timed(ex.validate, min_seconds)

    def prove_verify():
        ex.verify(ex.prove())
    out["prove_verify_ms"] = timed(prove_verify, min_seconds)
    base = out["resident_ms"]["median"]
    out["ratios_over_resident"] = {k[:-3]: round(out[k]["median"] / base, 2)
                                   for k in ("host_ms", "host_signed_ms", "resident_signed_ms", "validate_ms", "prove_verify_ms")}
    return out


def trace_run(backend, repeats):
    w = golden()
    indices = np.concatenate([w.s_indices, w.s_indices, w.r_indices, w.r_indices])
    values = np.concatenate([w.s_old_values, w.s_old_values, w.r_old_values, w.r_old_values])
    paths = np.concatenate([w.s_paths, w.s_paths, w.r_paths, w.r_paths])
    roots = np.concatenate([w.initial_roots] * 4)
    assert len(indices) == 4 * w.n_tx
    for _ in range(repeats):
        w.check(backend)
        backend.account_check_paths(indices, paths, roots, values=values)


def fold_trace(path):
    rows = {"k_witness_check": [], "k_path_check": []}
    with open(path) as f:
        for r in csv.DictReader(f):
            for name in rows:
                if name in r.get("Kernel_Name", ""):
                    rows[name].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {name: {"launches": len(v), "median_us": round(statistics.median(v) / 1e3, 2), "min_us": round(min(v) / 1e3, 2),
                  "last_us": round(v[-1] / 1e3, 2)} for name, v in rows.items()}
    out["witness_check_over_path_check"] = round(out["k_witness_check"]["median_us"] / out["k_path_check"]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_trace:
        result = {}
        if args.merge:
            with open(args.merge) as f:
                result = json.loads(f.read())
        result["kernel_trace_1024_d15"] = fold_trace(args.kernel_trace)
    else:
        from certificate_stark_amd.backend import Backend
        b = Backend()
        if args.trace_run:
            trace_run(b, args.trace_run)
            result = {"trace_run": args.trace_run}
        else:
            result = {"config": "cstark_tx_witness_check on the committed 1024-transfer depth-15 witness, MI355X; host clock around the synchronous calls"}
            result.update(bench(b, args.min_seconds))
        b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
