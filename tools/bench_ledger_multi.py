"""Multi-openings against per-account paths, on the same accounts in the same process: cstark_ledger_open_multi against
cstark_ledger_open_accounts, cstark_account_check_multiproof against cstark_account_check_paths.  Prints one JSON line.  Run on a GPU box.

    python tools/bench_ledger_multi.py [--min-seconds 1.0] [--out profiles/ledger_multi_bench.json] [--no-dense-paths]
        golden_1024_d15:    the 1,996 accounts of the committed witness (tests/golden/witness_1024_d15.npz) in a ledger of depth 15: a
                            sparse set, the check is a latency chain of depth + 1 launches against k_path_check's one
        dense_65536_d31:    65,536 consecutive accounts (seeded reduced words) from leaf 2^30 + 2^16 of a ledger of depth 31: a chunk
                            of state, 15 proof nodes and one subtree rebuild
    Per case and per form: bytes that travel (indices, values, presence flags, digests, root), merges of the check (leaf hashes apart),
    and the host clock around the synchronous calls (values and presence given: the leaf hashes run in both forms): warm-up first,
    then at least --min-seconds of calls, median and minimum in milliseconds.  Both forms are checked VALID before anything is timed.
    --no-dense-paths: the path form of the dense case (117 MB of digests) is not built; its byte and merge counts are reported alone."""
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


def timed(fn, min_seconds, warmup=3):
    for _ in range(warmup):
        fn()
    samples = []
    t_end = time.perf_counter() + min_seconds
    while time.perf_counter() < t_end or len(samples) < 5:
        t0 = time.perf_counter()
        fn()
        samples.append(time.perf_counter() - t0)
    return {"median": round(1e3 * statistics.median(samples), 4), "min": round(1e3 * min(samples), 4), "repeats": len(samples)}


def bench_case(backend, led, indices, min_seconds, with_paths=True):
    """indices: ascending and distinct, so both forms open exactly the same accounts"""
    n, d = len(indices), led.depth
    account_bytes = 8 * n + 112 * n + n + 56       # indices, values, presence flags, root: the same in both forms
    multi = led.open_multi(indices)
    got = multi.check()
    assert got.verdict == backend.MULTI_VALID and np.array_equal(got.root, led.root()) and multi.nbytes == account_bytes + multi.nodes.nbytes
    n_nodes, n_merges = backend.account_multiproof_shape(d, indices)
    assert (n_nodes, n_merges) == (len(multi.nodes), got.n_merges)
    out = {"accounts": n, "depth": d, "leaf_hashes": n,
           "multiproof": {"digests": n_nodes, "bytes": multi.nbytes, "merges": n_merges, "launches": d + 1},
           "paths": {"digests": n * (d + 1), "bytes": account_bytes + 56 * n * (d + 1), "merges": n * d, "launches": 1}}
    out["multiproof"]["open_ms"] = timed(lambda: led.open_multi(indices), min_seconds)
    out["multiproof"]["check_ms"] = timed(multi.check, min_seconds)
    if with_paths:
        paths = led.open(indices)
        assert not paths.check().any() and np.array_equal(paths.root, multi.root) and np.array_equal(paths.values, multi.values)
        out["paths"]["open_ms"] = timed(lambda: led.open(indices), min_seconds)
        out["paths"]["check_ms"] = timed(paths.check, min_seconds)
        for call in ("open_ms", "check_ms"):
            out["paths_over_multiproof_" + call[:-3]] = round(out["paths"][call]["median"] / out["multiproof"][call]["median"], 3)
    else:
        out["paths"]["measured"] = False
    return out


def golden(backend, min_seconds):
    import ledger_cases as LC
    from certificate_stark_amd.prover import Ledger
    w = LC.golden_1024()
    indices, initial = LC.initial_accounts(w)
    led = Ledger(w.depth, backend)
    led.set_accounts(indices, initial)
    out = bench_case(backend, led, np.unique(np.asarray(indices, np.uint64)), min_seconds)
    led.close()
    return out


def dense(backend, min_seconds, with_paths):
    from certificate_stark_amd.prover import Ledger
    count, first = 1 << 16, (1 << 30) + (1 << 16)
    indices = np.arange(first, first + count, dtype=np.uint64)
    values = np.random.default_rng(0x5EED31).integers(0, P, (count, 14), dtype=np.uint64)
    led = Ledger(31, backend)
    led.set_accounts(indices, values)
    out = bench_case(backend, led, indices, min_seconds, with_paths)
    led.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--no-dense-paths", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from certificate_stark_amd.backend import Backend
    b = Backend()
    result = {"config": "cstark_ledger_open_multi / cstark_account_check_multiproof against cstark_ledger_open_accounts / "
                        "cstark_account_check_paths, MI355X; host clock around the synchronous calls, milliseconds"}
    result["golden_1024_d15"] = golden(b, args.min_seconds)
    result["dense_65536_d31"] = dense(b, args.min_seconds, not args.no_dense_paths)
    b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
