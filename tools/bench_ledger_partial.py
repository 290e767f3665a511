"""The partial ledger and the update check against what they replace, on the same opening in the same process.  Prints one JSON line.
Run on a GPU box.

    python tools/bench_ledger_partial.py [--min-seconds 1.0] [--out profiles/ledger_partial_bench.json]
        golden_1024_d15:    the 1,996 accounts of the committed witness (tests/golden/witness_1024_d15.npz) in a ledger of depth 15, opened
                            before the batch; the batch is the witness's 1024 transfers
        dense_65536_d31:    65,536 consecutive accounts (seeded reduced words) from leaf 2^30 + 2^16 of a ledger of depth 31; the new state
                            of the update check is other seeded words for every account, the batch is 1024 transfers of delta 0 between
                            neighbours
    Per case, the host clock around the synchronous calls, warm-up first, then at least --min-seconds of calls, median and minimum in
    milliseconds:
        from_opening_ms against check_plus_create_ms (AccountMultiOpening.check() of the same opening plus Ledger(depth) creation and
        destruction; from_opening is timed with its destruction too), with check_ms and create_ms apart;
        apply_full_ms against apply_partial_ms: the same batch on the full ledger F and on P = from_opening, each under a checkpoint
        that is reverted outside the timed span, so every repeat applies to the same state;
        pair_ms (two back-to-back checks, old values and new values) against update_ms (cstark_account_check_update of the whole change
        against the stated new root), update_compute_only_ms, update_one_changed_ms and update_no_change_ms.
    Every form is checked VALID, the roots against each other, before anything is timed."""
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


def timed_apply(led, batch, min_seconds, warmup=3):
    """apply under a checkpoint, reverted outside the timed span"""
    cp = led.checkpoint()
    samples = []
    t_end = None
    k = 0
    while t_end is None or time.perf_counter() < t_end or len(samples) < 5:
        t0 = time.perf_counter()
        led.apply(batch, want_witness=False)
        dt = time.perf_counter() - t0
        led.revert(cp)
        k += 1
        if k == warmup:
            t_end = time.perf_counter() + min_seconds
        elif k > warmup:
            samples.append(dt)
    led.release(cp)
    return {"median": round(1e3 * statistics.median(samples), 4), "min": round(1e3 * min(samples), 4), "repeats": len(samples)}


def bench_partial(backend, full, opening, batch, min_seconds):
    """full: the ledger the opening was taken from, in the state of the opening; batch: transfers among the opened accounts"""
    from certificate_stark_amd.prover import Ledger
    d = opening.depth
    part = Ledger.from_opening(opening)
    assert part.partial and np.array_equal(part.root(), full.root())
    out = {"from_opening_ms": timed(lambda: Ledger.from_opening(opening).close(), min_seconds),
           "check_plus_create_ms": timed(lambda: (opening.check(), Ledger(d, backend).close()), min_seconds),
           "check_ms": timed(opening.check, min_seconds), "create_ms": timed(lambda: Ledger(d, backend).close(), min_seconds)}
    out["from_opening_over_check_plus_create"] = round(out["from_opening_ms"]["median"] / out["check_plus_create_ms"]["median"], 3)
    out["apply_full_ms"] = timed_apply(full, batch, min_seconds)
    out["apply_partial_ms"] = timed_apply(part, batch, min_seconds)
    out["apply_partial_over_full"] = round(out["apply_partial_ms"]["median"] / out["apply_full_ms"]["median"], 3)
    full.apply(batch, want_witness=False)
    part.apply(batch, want_witness=False)
    assert np.array_equal(part.root(), full.root()) and part.audit().consistent == 1
    out["partial_info"] = dict(zip(("is_partial", "n_known", "n_opaque"), part.partial_info()))
    part.close()
    return out


def bench_case(backend, old, new_values, new_present, min_seconds):
    """old: the AccountMultiOpening before the change; (new_values, new_present): the same accounts after it"""
    from certificate_stark_amd.prover import AccountMultiOpening
    n, d = len(old.indices), old.depth
    assert old.check().verdict == backend.MULTI_VALID
    computed = old.check_update(new_values, new_present)
    assert computed.verdict == backend.UPDATE_VALID and computed.n_changed > 0
    new = AccountMultiOpening(d, old.indices, new_values, new_present, old.nodes, computed.new_root, old.inverse, backend=backend)
    assert new.check().verdict == backend.MULTI_VALID          # the one-pass fold of the new state is the root a plain check accepts
    stated = old.check_update(new_values, new_present, new.root)
    assert stated.verdict == backend.UPDATE_VALID and np.array_equal(stated.new_root, new.root)
    k = int(np.flatnonzero((old.values != new_values).any(axis=1) | (old.present != new_present))[0])
    one_values, one_present = old.values.copy(), old.present.copy()
    one_values[k], one_present[k] = new_values[k], new_present[k]
    one = old.check_update(one_values, one_present)
    assert one.verdict == backend.UPDATE_VALID and one.n_changed == 1
    none = old.check_update(old.values, old.present, old.root)
    assert none.verdict == backend.UPDATE_VALID and none.n_changed == 0
    n_nodes, n_merges = backend.account_multiproof_shape(d, old.indices)
    out = {"accounts": n, "depth": d, "proof_nodes": n_nodes, "merges": n_merges, "changed": computed.n_changed,
           "launches": {"check": d + 1, "pair": 2 * (d + 1), "update": d + 1}}
    out["check_ms"] = timed(old.check, min_seconds)
    out["pair_ms"] = timed(lambda: (old.check(), new.check()), min_seconds)
    out["update_ms"] = timed(lambda: old.check_update(new_values, new_present, new.root), min_seconds)
    out["update_compute_only_ms"] = timed(lambda: old.check_update(new_values, new_present), min_seconds)
    out["update_one_changed_ms"] = timed(lambda: old.check_update(one_values, one_present), min_seconds)
    out["update_no_change_ms"] = timed(lambda: old.check_update(old.values, old.present, old.root), min_seconds)
    out["pair_over_update"] = round(out["pair_ms"]["median"] / out["update_ms"]["median"], 3)
    out["update_over_check"] = round(out["update_ms"]["median"] / out["check_ms"]["median"], 3)
    return out


def golden(backend, min_seconds):
    import ledger_cases as LC
    from certificate_stark_amd.prover import Ledger
    w = LC.golden_1024()
    indices, initial = LC.initial_accounts(w)
    led = Ledger(w.depth, backend)
    led.set_accounts(indices, initial)
    old = led.open_multi(indices)
    partial = bench_partial(backend, led, old, w, min_seconds)          # leaves the batch applied
    new_values, new_present = led.accounts(old.indices)
    out = bench_case(backend, old, new_values, new_present, min_seconds)
    out.update(partial)
    assert np.array_equal(old.check_update(new_values, new_present).new_root, led.root())
    led.close()
    return out


def dense(backend, min_seconds):
    from certificate_stark_amd.prover import Ledger
    count, first = 1 << 16, (1 << 30) + (1 << 16)
    indices = np.arange(first, first + count, dtype=np.uint64)
    rng = np.random.default_rng(0x5EED31)
    values, new_values = (rng.integers(0, P, (count, 14), dtype=np.uint64) for _ in range(2))
    led = Ledger(31, backend)
    led.set_accounts(indices, values)
    old = led.open_multi(indices)
    out = bench_case(backend, old, new_values, np.ones(count, bool), min_seconds)
    n_tx = 1024
    t = np.arange(n_tx, dtype=np.uint64)
    batch = (indices[2 * t], indices[2 * t + 1], np.zeros(n_tx, np.uint64), np.ones((n_tx, 6), np.uint64), np.zeros((n_tx, 32), np.uint8))
    cp = led.checkpoint()
    out.update(bench_partial(backend, led, old, batch, min_seconds))
    led.revert(cp)
    led.release(cp)
    led.set_accounts(indices, new_values)
    assert np.array_equal(old.check_update(new_values).new_root, led.root())
    led.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from certificate_stark_amd.backend import Backend
    b = Backend()
    result = {"config": "Ledger.from_opening against check() plus Ledger(depth); apply on the partial against the full ledger; "
                        "cstark_account_check_update against two cstark_account_check_multiproof calls; MI355X, host clock around the "
                        "synchronous calls, milliseconds"}
    result["golden_1024_d15"] = golden(b, args.min_seconds)
    result["dense_65536_d31"] = dense(b, args.min_seconds)
    b.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
