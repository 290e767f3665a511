"""Conversion of proofs between the plain and the compact form (cstark_tx_convert) against the verification it contains.  Run on a GPU
box; prints one JSON line (kept as profiles/convert_bench.json).

    python tools/bench_convert.py [--rounds 5] [--seconds 0.4] [--parent parent.json --alone alone.json]
    CSTARK_LIB=<library of the parent commit> python tools/bench_convert.py --verify-only > parent.json
    python tools/bench_convert.py --verify-only > alone.json

The headline statement (1024 transfers, 2^20 rows, 96 queries), 1 and 64 proofs per call, one process: the turns -- tx_verify of the
plain proofs, tx_verify of the compact ones, tx_convert to compact, tx_convert to plain -- alternate in rounds, each turn warmed up and
timed for --seconds of synchronous calls; per turn the median over the rounds and the spread (max - min).  Every call goes straight to
the C ABI with its arguments and output buffers made once, so a turn times the library, not the binding.  After the rounds one more
call per turn reads cstark_verify_stage_ms.  The bytes copied back are what the call's one copy spans: every changing proof's path
sections in the plain form (to the compact form the selected nodes are found inside that span) and, to the compact form, one count
word per tree.  --verify-only runs the two verify turns alone, for a library from before the convert calls; --parent merges its output.
The verify call of this build is compared with the parent's in a process of the same turns (--alone: this build's own --verify-only
run): beside convert turns, which write 64 proofs into 64 buffers between its calls, its host staging copy finds colder caches."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from certificate_stark_amd.backend import Backend  # noqa: E402
from certificate_stark_amd.prover import ProofOptions, TransactionExample, TransactionMetadata  # noqa: E402
from tools.bench_compact import path_digests  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SELECT_MS = 0.21   # select_multiproof per headline proof on the host
u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


def timed(call, seconds):
    for _ in range(2):
        call()
    calls, t0 = 0, time.perf_counter()
    while True:
        call()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / calls * 1e3


def alternate(turns, rounds, seconds):
    got = {k: [] for k in turns}
    for _ in range(rounds):
        for k, call in turns.items():
            got[k].append(timed(call, seconds))
    return {k: {"ms": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v], "spread": round(max(v) - min(v), 4)} for k, v in got.items()}


class Call:
    """one verify or convert call over `count` copies of `proof`, its arguments made once"""

    def __init__(self, b, proof, count, roots, form=None):
        self.b, self.count, self.form, self.proof = b, count, form, proof
        self.ptrs, self.lens = (C.POINTER(C.c_uint8) * count)(), (C.c_size_t * count)()
        for i in range(count):
            self.ptrs[i], self.lens[i] = C.cast(C.c_char_p(proof), C.POINTER(C.c_uint8)), len(proof)
        self.ir = np.ascontiguousarray(np.broadcast_to(np.asarray(roots[0], np.uint64), (count, 7)))
        self.fr = np.ascontiguousarray(np.broadcast_to(np.asarray(roots[1], np.uint64), (count, 7)))
        self.verdicts = np.zeros(count, np.int32)
        if form is not None:
            from certificate_stark_amd.verify import convert_bound
            cap = convert_bound(proof, form)
            self.bufs = [(C.c_uint8 * cap)() for _ in range(count)]
            self.out, self.caps, self.out_lens = (C.POINTER(C.c_uint8) * count)(), (C.c_size_t * count)(), (C.c_size_t * count)()
            for i, buf in enumerate(self.bufs):
                self.out[i], self.caps[i] = C.cast(buf, C.POINTER(C.c_uint8)), cap

    def __call__(self):
        b, head = self.b, (self.b.ctx, C.c_uint32(self.count), self.ptrs, self.lens, self.ir.ctypes.data_as(u64p), self.fr.ctypes.data_as(u64p), None)
        if self.form is None:
            rc = b.lib.cstark_tx_verify(*head, self.verdicts.ctypes.data_as(i32p))
        else:
            rc = b.lib.cstark_tx_convert(*head, C.c_uint32(b.PROOF_FORMS.index(self.form)), self.out, self.caps, self.out_lens,
                                         self.verdicts.ctypes.data_as(i32p))
        assert rc == 0 and not self.verdicts.any()

    def result(self, i=0):
        return bytes(memoryview(self.bufs[i])[:self.out_lens[i]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--verify-only", action="store_true")
    ap.add_argument("--parent", help="JSON printed by a --verify-only run on the parent commit's library")
    ap.add_argument("--alone", help="JSON printed by a --verify-only run on this build")
    args = ap.parse_args()
    b = Backend()
    meta = TransactionMetadata.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))
    head = ProofOptions(96, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)
    tx = TransactionExample(head, meta, b)
    plain, compact = tx.prove(), tx.prove(compact=True)
    roots = tx.pub_inputs()
    trees = len(path_digests(plain))
    out = {"device": "MI355X", "rounds": args.rounds, "seconds_per_turn": args.seconds, "library": os.environ.get("CSTARK_LIB", "this build"),
           "plain_bytes": len(plain), "compact_bytes": len(compact), "plain_digests": sum(path_digests(plain)),
           "compact_digests": sum(path_digests(compact)), "counts": {}}
    for count in (1, 64):
        turns = {"verify_plain": Call(b, plain, count, roots), "verify_compact": Call(b, compact, count, roots)}
        if not args.verify_only:
            turns["convert_to_compact"] = Call(b, plain, count, roots, "compact")
            turns["convert_to_plain"] = Call(b, compact, count, roots, "plain")
        res = alternate(turns, args.rounds, args.seconds)
        for name, call in turns.items():
            call()
            res[name]["stage_ms"] = {k: round(v, 4) for k, v in b.verify_stage_ms().items()}
            res[name]["h2d_bytes"] = b.verify_h2d_bytes()
        if not args.verify_only:
            assert turns["convert_to_compact"].result(count - 1) == compact and turns["convert_to_plain"].result(count - 1) == plain
            span = 32 * sum(path_digests(plain))
            res["convert_to_compact"]["d2h_bytes"] = count * (span + 4 * trees)
            res["convert_to_plain"]["d2h_bytes"] = count * span
            for conv, ver in (("convert_to_compact", "verify_plain"), ("convert_to_plain", "verify_compact")):
                res[conv]["over_its_verify_ms"] = round(res[conv]["ms"] - res[ver]["ms"], 4)
                res[conv]["over_its_verify_stage_ms"] = {k: round(res[conv]["stage_ms"][k] - res[ver]["stage_ms"][k], 4) for k in res[ver]["stage_ms"]}
            res["host_selection_ms"] = round(HOST_SELECT_MS * count, 2)
        out["counts"][str(count)] = res
    if args.parent and args.alone:
        with open(args.parent) as f:
            parent = json.loads(f.read().strip().splitlines()[-1])
        with open(args.alone) as f:
            alone = json.loads(f.read().strip().splitlines()[-1])
        for count, res in out["counts"].items():
            for name in ("verify_plain", "verify_compact"):
                p, a = parent["counts"][count][name], alone["counts"][count][name]
                res[name]["parent"] = {k: p[k] for k in ("ms", "spread", "rounds", "stage_ms")}
                res[name]["alone"] = {k: a[k] for k in ("ms", "spread", "rounds", "stage_ms")}
                res[name]["alone_inside_parent_spread"] = abs(a["ms"] - p["ms"]) <= p["spread"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
