"""Ledger checkpoints and the audit at the workload's size: the committed 1,024-transfer depth-15 witness (1,996 accounts).  Prints one
JSON line.  Run on a GPU box.

    python tools/bench_ledger_checkpoints.py [--min-seconds 1.0] [--parent-lib PATH] [--runs 3] [--out profiles/ledger_checkpoint_bench.json]
        Host clock around the synchronous call after warm-up, at least --min-seconds of calls, as tools/bench_ledger.py measures.
        apply_ms            Ledger.apply of the batch with no live checkpoint, witness left on the device (the ledger is reset by
                            set_accounts outside the timed region)
        apply_ab            with --parent-lib (the parent commit's libcstark_hip.so): that apply measured in fresh child processes,
                            parent and this build alternating, --runs each; is this build inside the parent's own spread?
        apply_checkpoint_ms the same apply with one live checkpoint (taken after the reset, released after the apply), and the slots
                            that apply consumed
        open_head_ms / open_at_ms   Ledger.open of the 1,996 accounts at the head and at a checkpoint three batches back
        revert_ms / release_ms      of a checkpoint with one 1,024-transfer batch behind it
        audit_ms            Ledger.audit of that ledger; audit_host_s: the same jobs with the host merge (hostgadgets.h, g++ -O2)
    python tools/bench_ledger_checkpoints.py --apply-only
        apply_ms alone; needs nothing the parent commit lacks (run with CSTARK_LIB=<the parent's library>)
    python tools/bench_ledger_checkpoints.py --trace-run 5
        the program to put behind `rocprofv3 --kernel-trace --output-format csv -d DIR --`: applies without and with a live checkpoint,
        audits, and one k_ledger_merge launch of the audit's job count (the leaf launch of a set_accounts of as many accounts)
    python tools/bench_ledger_checkpoints.py --kernel-trace DIR/.../*_kernel_trace.csv --trace-jobs N [--out ...]
        folds such a trace: launches per apply without and with a checkpoint, k_ledger_audit against k_ledger_merge at N jobs"""
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

FIELDS = ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s")


def stats(seconds):
    return {"median": round(1e3 * statistics.median(seconds), 4), "min": round(1e3 * min(seconds), 4), "max": round(1e3 * max(seconds), 4),
            "repeats": len(seconds)}


def timed(min_seconds, body, before=None, after=None, warm=3):
    """seconds of body() per call: `warm` calls, then at least min_seconds and five calls; before() / after() run outside the clock"""
    out = []
    t_end = None
    while True:
        if before:
            before()
        t0 = time.perf_counter()
        body()
        t1 = time.perf_counter()
        if after:
            after()
        if warm > 0:
            warm -= 1
            continue
        t_end = t_end or t0 + min_seconds
        out.append(t1 - t0)
        if t1 >= t_end and len(out) >= 5:
            return out


class Case:
    def __init__(self, backend):
        import ledger_cases as LC
        from certificate_stark_amd.prover import Ledger
        self.w = LC.golden_1024()
        self.indices, self.initial = LC.initial_accounts(self.w)
        self.tr = tuple(getattr(self.w, f) for f in FIELDS)
        self.led = Ledger(self.w.depth, backend)

    def reset(self):
        self.led.set_accounts(self.indices, self.initial)

    def apply(self):
        self.led.apply(self.tr, want_witness=False)


def apply_only(backend, min_seconds):
    c = Case(backend)
    c.reset()
    m = c.led.apply(c.tr)
    assert np.array_equal(m.s_paths, c.w.s_paths) and np.array_equal(m.final_root, c.w.final_root)
    out = stats(timed(min_seconds, c.apply, before=c.reset))
    c.led.close()
    return out


def alternate(parent_lib, runs, min_seconds):
    """apply_only in fresh child processes, the parent's library and this one alternating"""
    got = {"parent": [], "this_build": []}
    for _ in range(runs):
        for name in ("parent", "this_build"):
            env = dict(os.environ)
            env.pop("CSTARK_LIB", None)
            if name == "parent":
                env["CSTARK_LIB"] = os.path.abspath(parent_lib)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--apply-only", "--min-seconds", str(min_seconds)], env=env, capture_output=True,
                                 text=True, timeout=600)
            if res.returncode != 0:
                raise RuntimeError("child failed: " + res.stdout[-2000:] + res.stderr[-2000:])
            got[name].append(json.loads(res.stdout.strip().splitlines()[-1])["apply_ms"])
    p, t = [r["median"] for r in got["parent"]], [r["median"] for r in got["this_build"]]
    return {"order": "parent, this build, parent, ... in fresh processes", "parent_runs": got["parent"], "this_build_runs": got["this_build"],
            "parent_medians_ms": p, "this_build_medians_ms": t, "parent_spread_ms": [min(p), max(p)],
            "this_build_inside_parent_spread": [min(p) <= x <= max(p) for x in t],
            "this_build_above_parent_slowest_ms": round(max(0.0, max(t) - max(p)), 4)}


def full(backend, args):
    c = Case(backend)
    led = c.led
    out = {"n_tx": int(c.w.n_tx), "depth": int(c.w.depth), "accounts": int(len(c.indices))}
    out["apply_ms"] = stats(timed(args.min_seconds, c.apply, before=c.reset))
    # one live checkpoint: taken after the reset, released after the apply, both outside the clock
    cps, consumed = [], []

    def take():
        c.reset()
        cps.append((led.checkpoint(), led.audit()))

    def drop():
        cp, before = cps.pop()
        after = led.audit()
        consumed.append(int(after.slots_held - before.slots_held))
        led.release(cp)

    out["apply_checkpoint_ms"] = stats(timed(args.min_seconds, c.apply, before=take, after=drop))
    out["apply_checkpoint_slots_consumed"] = sorted(set(consumed))
    r = led.audit()
    out["slots_after_releases"] = {"live": int(r.slots_live), "held": int(r.slots_held), "free": int(r.slots_free)}
    # openings three batches back: the 1,024 transfers applied three times behind the checkpoint, the accounts set back to their
    # initial values between two applies (an overwriting set_accounts, so that the balances allow the batch again)
    # A checkpoint is taken ahead of every batch, as an operator who proves every batch would: the lookup at the oldest walks three logs.
    c.reset()
    taken = []
    for k in range(3):
        if k:
            c.reset()
        taken.append(led.checkpoint())
        c.apply()
    cp = taken[0]
    out["open_at_batches_back"], out["open_at_logs_walked"] = 3, 3
    head = timed(args.min_seconds, lambda: led.open(c.indices))
    past = timed(args.min_seconds, lambda: led.open(c.indices, at=cp))
    o = led.open(c.indices, at=cp)
    assert np.array_equal(o.root, c.w.initial_roots[0]) and np.array_equal(o.values, c.initial)
    out["open_head_ms"], out["open_at_ms"] = stats(head), stats(past)
    out["open_at_log_walk_share"] = round(1 - out["open_head_ms"]["median"] / out["open_at_ms"]["median"], 3)
    for t in taken:
        led.release(t)
    # revert and release of one 1,024-transfer batch
    marks = []

    def batch_behind_a_checkpoint():
        c.reset()
        marks.append(led.checkpoint())
        c.apply()

    out["revert_ms"] = stats(timed(args.min_seconds / 2, lambda: led.revert(marks[-1]), before=batch_behind_a_checkpoint, after=lambda: led.release(marks.pop())))
    out["release_ms"] = stats(timed(args.min_seconds / 2, lambda: led.release(marks.pop()), before=batch_behind_a_checkpoint))
    # the audit of that ledger
    c.reset()
    r = led.audit()
    assert r.consistent == 1
    out["audit_jobs"] = int(c.w.depth + r.n_nodes)
    out["audit_ms"] = stats(timed(args.min_seconds, led.audit))
    if not args.no_baseline:
        out["audit_host_s"] = round(host_audit_seconds(c), 4)
        out["audit_host_us_per_merge"] = round(1e6 * out["audit_host_s"] / out["audit_jobs"], 2)
        out["audit_speedup_vs_host"] = round(1e3 * out["audit_host_s"] / out["audit_ms"]["median"], 1)
    led.close()
    return out


def host_audit_seconds(c):
    with tempfile.TemporaryDirectory() as tmp:
        exe, path = os.path.join(tmp, "ledger_checkpoint_check"), os.path.join(tmp, "ledger.bin")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_checkpoint_check.cpp")])
        with open(path, "wb") as f:
            for a in (np.array([c.w.depth, len(c.indices)], np.uint64), c.indices, c.initial):
                f.write(np.ascontiguousarray(a, "<u8").tobytes())
        res = subprocess.run([exe, "--time", path], capture_output=True, text=True)
        if res.returncode != 0 or "seconds=" not in res.stdout:
            raise RuntimeError("host audit failed: " + res.stdout + res.stderr)
        return float(res.stdout.split("seconds=")[1].split()[0])


def trace_run(backend, repeats):
    from certificate_stark_amd.prover import Ledger
    c = Case(backend)
    led = c.led
    c.reset()
    jobs = int(c.w.depth + led.audit().n_nodes)      # the first audit of the trace: fold_trace's segment 0 ends here
    twin = Ledger(15, backend)                      # its set_accounts of `jobs` accounts: one k_ledger_merge launch of `jobs` merges
    values = np.tile(c.initial[0], (jobs, 1))
    for _ in range(repeats):                        # the audits are the marks fold_trace cuts the trace at: six segments per repeat
        c.reset()                                   # 1: (the twin's creation or set_accounts and) the reset
        led.audit()
        c.apply()                                   # 2: an apply with no live checkpoint
        led.audit()
        c.reset()                                   # 3: the reset
        led.audit()
        cp = led.checkpoint()                       # 4: checkpoint
        led.audit()
        c.apply()                                   # 5: the same apply with one live checkpoint
        led.audit()
        led.revert(cp)                              # 6: revert and release
        led.release(cp)
        led.audit()
        twin.set_accounts(np.arange(jobs, dtype=np.uint64), values)
    twin.close()
    led.close()
    return {"trace_jobs": jobs, "repeats": repeats}


def fold_trace(path, jobs):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_ledger_" in name:
                kind = "audit" if "k_ledger_audit" in name else "merge" if "k_ledger_merge" in name else "gather"
                rows.append((kind, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)))
    rows.sort(key=lambda x: x[1])
    grid = 64 * ((jobs + 3) // 4)
    audits = [(x[2] - x[1]) / 1e3 for x in rows if x[0] == "audit" and x[3] == grid]
    merges = [(x[2] - x[1]) / 1e3 for x in rows if x[0] == "merge" and x[3] == grid]
    # the ledger's launches between two audits: six segments per repeat of --trace-run (see trace_run)
    segments, cur = [], []
    for x in rows:
        if x[0] == "audit":
            segments.append(cur)
            cur = []
        else:
            cur.append(x[0])

    def shapes(position):
        found = {}
        for s in segments[position::6]:
            key = "%d k_ledger_merge + %d k_ledger_gather" % (s.count("merge"), s.count("gather"))
            found[key] = found.get(key, 0) + 1
        return found

    out = {"trace_jobs": jobs, "launches_apply_no_checkpoint": shapes(2), "launches_checkpoint": shapes(4), "launches_apply_one_live_checkpoint": shapes(5),
           "launches_revert_and_release": shapes(6),
           "k_ledger_audit_us": {"launches": len(audits), "median": round(statistics.median(audits), 2), "min": round(min(audits), 2), "max": round(max(audits), 2)},
           "k_ledger_merge_same_jobs_us": {"launches": len(merges), "median": round(statistics.median(merges), 2), "min": round(min(merges), 2),
                                           "max": round(max(merges), 2)}}
    out["audit_over_merge"] = round(out["k_ledger_audit_us"]["median"] / out["k_ledger_merge_same_jobs_us"]["median"], 3)
    out["merge_spread"] = round(out["k_ledger_merge_same_jobs_us"]["max"] / out["k_ledger_merge_same_jobs_us"]["min"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--apply-only", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-jobs", type=int, default=0)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_trace:
        result = {"kernel_trace": fold_trace(args.kernel_trace, args.trace_jobs)}
    else:
        from certificate_stark_amd.backend import Backend
        b = Backend()
        if args.apply_only:
            result = {"apply_ms": apply_only(b, args.min_seconds)}
        elif args.trace_run:
            result = trace_run(b, args.trace_run)
        else:
            result = {"config": "ledger checkpoints and audit, the committed 1024-transfer depth-15 witness, MI355X; host clock around the synchronous calls"}
            result.update(full(b, args))
        b.close()
        if args.parent_lib and not args.apply_only and not args.trace_run:
            result["apply_ab"] = alternate(args.parent_lib, args.runs, args.min_seconds)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
