"""Ledger.select at the workload's size against what an operator had before it, in one process on one box.  Prints one JSON line.  Run on a
GPU box.

    python tools/bench_ledger_select.py [--min-seconds 1.0] [--out profiles/ledger_select_bench.json]

The pool is the committed 1,024-transfer depth-15 witness (tests/golden/witness_1024_d15.npz) re-signed with Ledger.sign (the senders'
secrets recovered by matching their keys against public_keys(1..255)):
    clean                  the 1,024 signed transfers, want 1,024
    corrupt_1 / 10 / 50    1 %, 10 % and 50 % of the candidates (seeded choice) with one scalar bit flipped
    pool_2048 / pool_8192  every signed transfer followed by 1 or 7 forged candidates (a sender that only receives in the batch, delta 0,
                           seeded signature words), want 1,024
Per case: select alone (read-only) and select with apply (the witness left on the device, as in the checked apply it is compared with)
with the ledger put back by a checkpoint's revert outside the clock; n_selected, n_sig_checked, n_chunks.  Against them, in the same run: apply(check_signatures=True) on the clean pool, and for the corrupted pools
the retry loop of apply(check_signatures=True) that drops the refused transfer each time (total time, number of calls, transfers left).
The host clock is taken around the synchronous calls after warm-up, for at least --min-seconds: median and minimum in milliseconds."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

P = 2**62 + 2**56 + 2**55 + 1
SEED = 0x5E1EC7


def timed(fn, min_seconds, after=None, warmup=2, least=5):
    for _ in range(warmup):
        fn()
        if after:
            after()
    samples = []
    t_end = time.perf_counter() + min_seconds
    while time.perf_counter() < t_end or len(samples) < least:
        t0 = time.perf_counter()
        fn()
        samples.append(time.perf_counter() - t0)
        if after:
            after()
    return {"median": round(1e3 * statistics.median(samples), 4), "min": round(1e3 * min(samples), 4), "max": round(1e3 * max(samples), 4),
            "repeats": len(samples)}


def corrupted(pool, percent, rng):
    s, r, d, rx, ss = (a.copy() for a in pool)
    bad = rng.choice(len(s), len(s) * percent // 100, replace=False)
    ss[bad, 7] ^= 0x20
    return s, r, d, rx, ss


def extended(pool, junk_per_real, rng):
    """every signed transfer followed by forged candidates whose senders only receive in the batch"""
    s, r, d, rx, ss = pool
    only_receive = np.setdiff1d(r, s)
    n, k = len(s), junk_per_real + 1
    S, R, D = np.zeros(n * k, np.uint64), np.zeros(n * k, np.uint64), np.zeros(n * k, np.uint64)
    RX, SS = rng.integers(0, P, (n * k, 6), dtype=np.uint64), rng.integers(0, 128, (n * k, 32), dtype=np.uint8)
    S[:], R[:] = rng.choice(only_receive, n * k), np.repeat(r, k)
    S[::k], R[::k], D[::k], RX[::k], SS[::k] = s, r, d, rx, ss
    return S, R, D, RX, SS


def retry_loop(led, pool):
    """what the parent commit offers for a pool with bad candidates: the checked apply, dropping the refused transfer each time"""
    from certificate_stark_amd.prover import TransferRefused
    keep = np.ones(len(pool[0]), bool)
    where = np.arange(len(keep))
    calls = 0
    while keep.any():
        calls += 1
        try:
            led.apply(tuple(a[keep] for a in pool), want_witness=False, check_signatures=True)
            break
        except TransferRefused as e:
            keep[where[keep][e.index]] = False
    return calls, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ledger_cases as LC
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import Ledger, public_keys
    b = Backend()
    w = LC.golden_1024()
    indices, initial = LC.initial_accounts(w)
    initial = np.asarray(initial, np.uint64).reshape(-1, 14)
    led = Ledger(w.depth, b)
    led.set_accounts(indices, initial)
    keys = public_keys(np.arange(1, 256, dtype=np.uint64), b)
    secret_of = {keys[k].tobytes(): k + 1 for k in range(255)}
    key_at = {int(i): v[:12].tobytes() for i, v in zip(indices, initial)}
    secrets = np.array([secret_of[key_at[int(i)]] for i in w.s_indices], np.uint64)
    clean = led.sign((w.s_indices, w.r_indices, w.deltas), secrets, seed=SEED)
    cp = led.checkpoint()
    back = lambda: led.revert(cp)
    rng = np.random.default_rng(SEED)
    pools = {"clean": clean, "corrupt_1": corrupted(clean, 1, rng), "corrupt_10": corrupted(clean, 10, rng), "corrupt_50": corrupted(clean, 50, rng),
             "pool_2048": extended(clean, 1, rng), "pool_8192": extended(clean, 7, rng)}
    result = {"config": "Ledger.select on the committed 1024-transfer depth-15 witness re-signed with Ledger.sign, want 1024, pow2 off, MI355X; "
                        "host clock around the synchronous calls, milliseconds", "cases": {}}
    result["apply_checked_clean_ms"] = timed(lambda: led.apply(clean, want_witness=False, check_signatures=True), args.min_seconds, after=back)
    for name, pool in pools.items():
        sel = led.select(pool, 1024, pow2=False)
        out = {"candidates": len(pool[0]), "n_selected": len(sel), "n_sig_checked": sel.report.n_sig_checked, "n_chunks": sel.report.n_chunks,
               "counts": sel.counts}
        out["select_ms"] = timed(lambda: led.select(pool, 1024, pow2=False), args.min_seconds)
        # as the checked apply it is compared with: the witness stays on the device (Backend.ledger_select, want_witness=False)
        flags = b.SELECT_CHECK_SIGNATURES | b.SELECT_APPLY
        out["select_apply_ms"] = timed(lambda: b.ledger_select(led._led, led.depth, *pool, 1024, flags=flags, want_witness=False), args.min_seconds, after=back)
        if name == "clean":
            out["select_apply_minus_apply_checked_ms"] = round(out["select_apply_ms"]["median"] - result["apply_checked_clean_ms"]["median"], 4)
        if name.startswith("corrupt"):
            calls, left = retry_loop(led, pool)
            back()
            loop = timed(lambda: retry_loop(led, pool), 0.0, after=back, warmup=0, least=3)
            out["retry_loop"] = {"calls": calls, "transfers_left": left, "ms": loop,
                                 "over_select_apply": round(loop["median"] / out["select_apply_ms"]["median"], 2)}
        result["cases"][name] = out
    led.close()
    b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
