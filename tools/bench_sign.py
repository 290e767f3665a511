"""The device signer at the workload's size: cstark_schnorr_public_keys + cstark_schnorr_sign of 1024 messages against the host signer
that cstark_schnorr_witness_generate runs for the same number of signatures, and against the check of the signatures it made.
Prints one JSON line.  Run on a GPU box.

    python tools/bench_sign.py [--min-seconds 1.0] [--out profiles/sign_bench.json]
        sign_ms[keys]:        host clock around Backend.schnorr_public_keys + Backend.schnorr_sign (synchronous: uploads, the rounds of
                              launches, results back) of 1024 messages, with keys 1..8 in turn and with key 255; warm-up first (the
                              fixed-base table is built by it), then at least --min-seconds of calls.  rounds / attempts_run: what the
                              schedule of csrc/sign_plan.h ran for the accepted attempts the call reports; ms_per_round follows
        host_generate_1024_ms: the path that existed before, in the same run: cstark_schnorr_witness_generate(1024), keys 1..8, the same
                              key derivation and signing on one host thread; sign_speedup_vs_host is the ratio
        check_1024_ms:        Backend.schnorr_check of the 1024 signatures just made (keys 1..8), and sign_over_check
    python tools/bench_sign.py --trace-run 5
        five calls of schnorr_sign_nonces with 2048 nonces uniform below 2^264 (every one of the 66 digits in use) and five checks of 1024
        signatures (2048 ladders), and nothing else: the program to put behind `rocprofv3 --kernel-trace --output-format csv -d DIR --`
    python tools/bench_sign.py --kernel-trace DIR/.../*_kernel_trace.csv [--out ...]
        folds such a trace into device time per kernel (added to the JSON of --out where that file exists); comb_over_ladder is the one
        condition the table has to meet (below 1)"""
import argparse
import csv
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

P = 2**62 + 2**56 + 2**55 + 1
N = 1024


def timed(fn, min_seconds, warmup=3, at_least=5):
    for _ in range(warmup):
        fn()
    samples = []
    t_end = time.perf_counter() + min_seconds
    while time.perf_counter() < t_end or len(samples) < at_least:
        t0 = time.perf_counter()
        fn()
        samples.append(time.perf_counter() - t0)
    return {"median": round(1e3 * statistics.median(samples), 4), "min": round(1e3 * min(samples), 4), "max": round(1e3 * max(samples), 4),
            "repeats": len(samples)}


def batch(backend, secrets, seed):
    """messages [n][28]: the device's public key of every secret, then 16 reduced words"""
    rng = random.Random(seed)
    sk = np.asarray(secrets, np.uint64)
    m = np.zeros((sk.size, 28), np.uint64)
    m[:, :12] = backend.schnorr_public_keys(sk)
    m[:, 12:] = np.array([[rng.randrange(P) for _ in range(16)] for _ in range(sk.size)], np.uint64)
    return m, sk


def schedule(attempts, secrets, max_attempts):
    """rounds and attempts run by the schedule of csrc/sign_plan.h, (sk + 2) / 2 attempts per pending signature and round, for the
    accepted attempts the call reported"""
    per_round = (np.asarray(secrets, np.int64) + 2) // 2
    rounds = -(-np.asarray(attempts, np.int64) // per_round)
    return int(rounds.max()), int(np.minimum(rounds * per_round, max_attempts).sum())


def bench_sign(backend, min_seconds):
    out = {"n": N, "sign_ms": {}}
    kept = None
    for name, secrets, max_attempts in (("1..8", [1 + i % 8 for i in range(N)], 256), ("255", [255] * N, 4096)):
        m, sk = batch(backend, secrets, 0xBE7C4)
        payload = m[:, 12:].copy()

        def run():
            msg = np.zeros((N, 28), np.uint64)
            msg[:, :12] = backend.schnorr_public_keys(sk)
            msg[:, 12:] = payload
            return msg, backend.schnorr_sign(msg, sk, seed=1, max_attempts=max_attempts)
        msg, (rx, s, attempts, status) = run()
        assert not status.any() and not backend.schnorr_check(msg, rx, s).any()
        entry = timed(run, min_seconds)
        entry["rounds"], entry["attempts_run"] = schedule(attempts, sk, max_attempts)
        entry["attempts_accepted_mean"] = round(float(attempts.mean()), 2)
        entry["ms_per_round"] = round(entry["median"] / entry["rounds"], 4)
        out["sign_ms"][name] = entry
        if kept is None:
            kept = (msg, rx, s)
    out["check_1024_ms"] = timed(lambda: backend.schnorr_check(*kept), min_seconds)
    out["sign_over_check"] = round(out["sign_ms"]["1..8"]["median"] / out["check_1024_ms"]["median"], 3)
    return out


def bench_host(min_seconds):
    from certificate_stark_amd import _lib
    lib = _lib.load()
    msg, rx, s = np.zeros((N, 28), np.uint64), np.zeros((N, 6), np.uint64), np.zeros((N, 32), np.uint8)

    def run():
        _lib.check(lib.cstark_schnorr_witness_generate(C.c_uint32(N), C.c_uint64(1), msg.ctypes.data_as(_lib.u64p), rx.ctypes.data_as(_lib.u64p),
                                                       s.ctypes.data_as(_lib.u8p)))
    return timed(run, min_seconds, warmup=0, at_least=2)


def trace_run(backend, repeats):
    rng = random.Random(0x7ACE)
    halves = [batch(backend, [1 + i % 8 for i in range(N)], 0x7ACE + h) for h in (0, 1)]   # keys by launches of 1024: only the timed comb has 2048
    m, sk = np.concatenate([h[0] for h in halves]), np.concatenate([h[1] for h in halves])
    nonces = np.array([[rng.getrandbits(64) for _ in range(4)] + [rng.getrandbits(8)] for _ in range(2 * N)], np.uint64)
    rx, s, _, status = backend.schnorr_sign(m[:N], sk[:N], seed=1, max_attempts=256)
    assert not status.any()
    for _ in range(repeats):
        backend.schnorr_sign_nonces(m, sk, nonces)
        backend.schnorr_check(m[:N], rx, s)


def fold_trace(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for key in ("k_sign_table", "k_sign_comb", "k_sign_gather", "k_sign_scalar", "k_sig_hash", "k_sig_ladder", "k_sig_final"):
                if key in name:
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)))
    out = {}
    for key, v in rows.items():
        v.sort()
        if key == "k_sign_comb":        # the launches of 2048 nonces only: the seeded signer's rounds ahead of them have other sizes
            v = [x for x in v if x[2] in (0, 2 * N * 64)] or v
        out[key] = {"launches": len(v), "last_us": round((v[-1][1] - v[-1][0]) / 1e3, 2), "median_us": round(statistics.median(e - s for s, e, _ in v) / 1e3, 2),
                    "min_us": round(min(e - s for s, e, _ in v) / 1e3, 2)}
    if "k_sign_comb" in out and "k_sig_ladder" in out:
        out["comb_over_ladder"] = round(out["k_sign_comb"]["median_us"] / out["k_sig_ladder"]["median_us"], 3)
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
        result = {}
        if args.out and os.path.exists(args.out):       # beside the host-clock figures of the same build, where they are there
            with open(args.out) as f:
                result = json.load(f)
        result["kernel_trace_2048"] = fold_trace(args.kernel_trace)
    else:
        from certificate_stark_amd.backend import Backend
        b = Backend()
        if args.trace_run:
            trace_run(b, args.trace_run)
            result = {"trace_run": args.trace_run}
        else:
            result = {"config": "cstark_schnorr_public_keys + cstark_schnorr_sign, 1024 messages, MI355X; host clock around the synchronous calls"}
            result.update(bench_sign(b, args.min_seconds))
            if not args.no_baseline:
                result["host_generate_1024_ms"] = bench_host(args.min_seconds)
                result["sign_speedup_vs_host"] = round(result["host_generate_1024_ms"]["median"] / result["sign_ms"]["1..8"]["median"], 1)
        b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
