"""Trace validation at the workload's size: cstark_air_validate_trace against the two other ways to learn whether a witness is good.
Prints one JSON line.  Run on a GPU box.

    python tools/bench_validate.py [--min-seconds 1.0] [--out profiles/validate_bench.json]
        tx_1024_d15:     the committed 1024-transfer witness (tests/golden/witness_1024_d15.npz), 94 x 2^20 rows, with its 14 public
                         words: validate_ms = host clock around the synchronous call on a resident device trace; warm-up first, then at
                         least --min-seconds of calls.  Beside it, in the same run:
                           prove_verify_ms  (a) cstark_tx_prove + cstark_tx_verify of the same witness: the only way to learn the same
                                            fact without this call
                           host_route_ms    (b) the device-to-host copy of the trace + oracle.tx_check_trace with 16 threads
        schnorr_512:     the 512-signature SchnorrAir trace (56 x 2^18) against the resident statement
        merkle_512:      the 512-transfer MerkleAir trace (65 x 2^18) of the first 512 transfers of the same witness
    python tools/bench_validate.py --trace-run 5
        five validations of each case and nothing else: the program to put behind `rocprofv3 --kernel-trace --output-format csv -d DIR --`
    python tools/bench_validate.py --kernel-trace DIR/.../*_kernel_trace.csv [--out ...]
        folds such a trace into device time per validation kernel"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz")


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


def cases(b):
    """name -> (air, device trace, depth, public inputs, metadata); the Schnorr statement is left resident last"""
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample, TransactionMetadata
    full = TransactionMetadata.load(FIXTURE)
    m512 = TransactionMetadata(*[getattr(full, f) if f == "final_root" else getattr(full, f)[:512] for f in TransactionMetadata.FIELDS])
    out = {}
    b.upload_witness(m512)
    mt = b.merkle_build_trace()
    out["merkle_512"] = (b.AIR_MERKLE, mt, 15, None, m512)     # the 512-transfer prefix ends at another root than the stated one: transitions only
    b.upload_witness(full)
    out["tx_1024_d15"] = (b.AIR_TRANSACTION, b.build_trace(), 15, np.concatenate([full.initial_roots[0], full.final_root]), full)
    sx = SchnorrExample.build_random(ProofOptions(), 512, backend=b)
    b.upload_schnorr_witness(sx.messages, sx.sig_rx, sx.sig_s)
    out["schnorr_512"] = (b.AIR_SCHNORR, b.schnorr_build_trace(), 0, True, None)
    b.synchronize()
    return out


def bench(min_seconds):
    from certificate_stark_amd.backend import Backend, to_numpy_u64
    from certificate_stark_amd.prover import get_example_options
    from oracle import oracle as O
    b = Backend()
    cs = cases(b)
    res = {}
    for name in ("merkle_512", "schnorr_512", "tx_1024_d15"):
        air, trace, depth, pub, _ = cs[name]
        rep = b.air_validate_trace(air, trace, depth, pub)
        assert rep.ok, "%s: %s" % (name, rep)
        res[name] = {"rows": int(trace.shape[1]), "width": int(trace.shape[0]),
                     "validate_ms": timed(lambda: b.air_validate_trace(air, trace, depth, pub), min_seconds)}
    air, trace, depth, pub, full = cs["tx_1024_d15"]
    b.upload_witness(full)
    opts = get_example_options()

    def prove_verify():
        proof = b.prove(opts)
        assert int(b.tx_verify([proof], full.initial_roots[0], full.final_root)[0]) == 0
    res["tx_1024_d15"]["prove_verify_ms"] = timed(prove_verify, min_seconds)
    O.build()
    O.set_num_threads(16)

    def host_route():
        assert O.tx_check_trace(to_numpy_u64(trace), 1024, 15) == -1
    res["tx_1024_d15"]["host_route_ms"] = timed(host_route, min_seconds, warmup=1)
    res["tx_1024_d15"]["host_threads"] = O.num_threads()
    v, a = res["tx_1024_d15"]["validate_ms"]["median"], res["tx_1024_d15"]["prove_verify_ms"]["median"]
    res["tx_1024_d15"]["validate_below_prove_verify"] = bool(v < a)
    b.close()
    return res


def trace_run(count):
    from certificate_stark_amd.backend import Backend
    b = Backend()
    for name, (air, trace, depth, pub, _) in cases(b).items():
        for _ in range(count):
            b.air_validate_trace(air, trace, depth, pub)
    b.close()


def kernel_trace(path):
    """device time per kernel name of the validation, from a rocprofv3 kernel trace: calls, total and mean microseconds"""
    per = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("KernelName") or ""
            if "k_validate" not in name and "k_eval_frames" not in name:
                continue
            dt = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            e = per.setdefault(name.split("(")[0], [0, 0.0])
            e[0] += 1; e[1] += dt
    return {k: {"calls": c, "total_us": round(t, 1), "mean_us": round(t / c, 2)} for k, (c, t) in sorted(per.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.trace_run:
        trace_run(a.trace_run)
        return
    res = {"kernels": kernel_trace(a.kernel_trace)} if a.kernel_trace else bench(a.min_seconds)
    if a.out and os.path.exists(a.out) and a.kernel_trace:     # the kernel times join the timings of an earlier run
        with open(a.out) as f:
            old = json.load(f)
        old.update(res); res = old
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
