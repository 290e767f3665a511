"""The signature check at the workload's size: cstark_schnorr_check_signatures against the SchnorrAir trace of the same signatures (the
same ladders plus 56 stored columns), the checked ledger apply against the unchecked one, and the same check on this machine's CPU.
Prints one JSON line.  Run on a GPU box.

    python tools/bench_sigcheck.py [--min-seconds 1.0] [--out profiles/sig_check_bench.json]
        check_ms[count]:      host clock around Backend.schnorr_check (synchronous: upload, three launches, verdicts back) at 1, 64, 1024
                              and 8192 signatures; warm-up first, then at least --min-seconds of calls
        trace_1024_ms:        the yardstick, in the same run: cstark_schnorr_build_trace of the same 1024 signatures (resident witness,
                              no copies) followed by a synchronise
        apply_ms / apply_checked_ms: Ledger.apply without and with check_signatures, 1024 transfers at depth 15 (the committed
                              witness), witness left on the device; the ledger is reset outside the timed region
        host_check_s:         verify_signature for the same 1024 transfers with the host arithmetic of hostgadgets.h
                              (tests/cpp/ledger_messages_check.cpp --time, g++ -O2), one signature after the other
    python tools/bench_sigcheck.py --trace-run 5
        five checks and five traces of 1024 signatures and nothing else: the program to put behind
        `rocprofv3 --kernel-trace --output-format csv -d DIR --`
    python tools/bench_sigcheck.py --kernel-trace DIR/.../*_kernel_trace.csv [--out ...]
        folds such a trace into device time per kernel (the last launch of each: everything warm)"""
import argparse
import csv
import functools
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

COUNTS = (1, 64, 1024, 8192)


@functools.lru_cache(maxsize=None)
def _generated_1024():
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample
    ex = SchnorrExample.build_random(ProofOptions(), 1024, seed=1, backend=object())
    return ex.messages, ex.sig_rx, ex.sig_s


def signatures(count):
    """`count` valid signatures: the first of 1024 generated ones, repeated beyond that"""
    reps = (count + 1023) // 1024
    return tuple(np.ascontiguousarray(np.concatenate([a] * reps)[:count]) for a in _generated_1024())


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


def trace_fn(backend, sigs):
    backend.upload_schnorr_witness(*sigs)

    def run():
        backend.schnorr_build_trace()
        backend.synchronize()
    return run


def bench_check(backend, min_seconds):
    out = {"check_ms": {}}
    for count in COUNTS:
        sigs = signatures(count)
        assert not backend.schnorr_check(*sigs).any()
        out["check_ms"][str(count)] = timed(lambda: backend.schnorr_check(*sigs), min_seconds)
    out["trace_1024_ms"] = timed(trace_fn(backend, signatures(1024)), min_seconds)
    out["check_over_trace_1024"] = round(out["check_ms"]["1024"]["median"] / out["trace_1024_ms"]["median"], 3)
    return out


def bench_apply(backend, min_seconds):
    import ledger_cases as LC
    from certificate_stark_amd.prover import Ledger
    w = LC.golden_1024()
    indices, initial = LC.initial_accounts(w)
    tr = tuple(getattr(w, f) for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))
    led = Ledger(w.depth, backend)
    out = {"n_tx": int(w.n_tx), "depth": int(w.depth)}
    for name, flag in (("apply_ms", False), ("apply_checked_ms", True)):
        samples = []
        t_end = None
        while t_end is None or time.perf_counter() < t_end or len(samples) < 5:
            led.set_accounts(indices, initial)
            t0 = time.perf_counter()
            led.apply(tr, want_witness=False, check_signatures=flag)
            dt = time.perf_counter() - t0
            if t_end is None:                       # the first apply is the warm-up
                t_end = time.perf_counter() + min_seconds
            else:
                samples.append(dt)
        out[name] = {"median": round(1e3 * statistics.median(samples), 4), "min": round(1e3 * min(samples), 4), "max": round(1e3 * max(samples), 4),
                     "repeats": len(samples)}
    led.close()
    return out


def host_check_seconds(tmp):
    import ledger_cases as LC
    import sig_cases as SC
    w = LC.golden_1024()
    exe, path = SC.build_messages_checker(tmp, sanitize=False), os.path.join(tmp, "case.bin")
    SC.write_messages_case(path, w)
    res = subprocess.run([exe, path, "--time"], capture_output=True, text=True)
    if res.returncode != 0 or "%d signatures valid" % w.n_tx not in res.stdout:
        raise RuntimeError("host check failed: " + res.stdout + res.stderr)
    return float(res.stdout.split("seconds=")[1].split()[0])


def fold_trace(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for key in ("k_sig_hash", "k_sig_ladder", "k_sig_final", "k_trace_schnorr_hash", "k_trace_schnorr_ec", "k_trace_schnorr_final", "k_trace_schnorr_bits"):
                if key in name:
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for key, v in rows.items():
        v.sort()
        out[key] = {"launches": len(v), "last_us": round((v[-1][1] - v[-1][0]) / 1e3, 2), "median_us": round(statistics.median(e - s for s, e in v) / 1e3, 2)}
    for name, keys in (("check_device_us", ("k_sig_hash", "k_sig_ladder", "k_sig_final")),
                       ("trace_device_us", ("k_trace_schnorr_hash", "k_trace_schnorr_ec", "k_trace_schnorr_final", "k_trace_schnorr_bits"))):
        if all(k in out for k in keys):
            out[name] = round(sum(out[k]["median_us"] for k in keys), 2)
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
        result = {"kernel_trace_1024": fold_trace(args.kernel_trace)}
    else:
        from certificate_stark_amd.backend import Backend
        b = Backend()
        if args.trace_run:
            sigs = signatures(1024)
            run_trace = trace_fn(b, sigs)
            for _ in range(args.trace_run):
                b.schnorr_check(*sigs)
                run_trace()
            result = {"trace_run": args.trace_run}
        else:
            result = {"config": "cstark_schnorr_check_signatures and cstark_ledger_apply_checked, MI355X; host clock around the synchronous calls"}
            result.update(bench_check(b, args.min_seconds))
            result["ledger_1024_d15"] = bench_apply(b, args.min_seconds)
            if not args.no_baseline:
                with tempfile.TemporaryDirectory() as tmp:
                    s = host_check_seconds(tmp)
                result["host_check_s"] = round(s, 4)
                result["host_us_per_signature"] = round(1e6 * s / 1024, 1)
                result["speedup_vs_host_1024"] = round(1e3 * s / result["check_ms"]["1024"]["median"], 1)
        b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
