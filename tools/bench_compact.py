"""The compact proof form (include/cstark.h, "Proof layout") against the plain form: sizes, verify time, prove time.  Run on a GPU box;
prints one JSON line (kept as profiles/compact_proof.json).

    python tools/bench_compact.py [--rounds 5] [--seconds 0.4] [--skip-sizes] [--plain-only]

Sizes are exact, not timed: the length of both forms and the digests in every tree's path section, for the 1024-transfer headline
options, the Sha3 / quadratic / cubic option sets, a SchnorrAir proof of 512 signatures (2^18 rows) and a range proof over 2^16 rows.

Times: both forms of the SAME statement in one process, alternating in rounds (plain, compact, plain, ...), each turn warmed up and
timed for --seconds of synchronous calls; per form the median over the rounds and the spread (max - min) of the rounds.  A difference
inside the spread of the plain form's own rounds is reported as "no difference".  cstark_tx_verify at counts 1 and 64 with
cstark_verify_h2d_bytes of both forms; cstark_tx_prove at the headline options with the channel it reports (the compact form must
stay on the device channel: it adds no host wait).

--plain-only: for a library built from the commit before the form existed (CSTARK_LIB=...): the plain turns alone, same rounds."""
import argparse
import json
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from certificate_stark_amd.backend import Backend  # noqa: E402
from certificate_stark_amd.prover import ProofOptions, SchnorrExample, TransactionExample, TransactionMetadata  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE = {0: 8, 1: 4, 2: 8, 3: 2, 4: 4}  # composition columns per AIR id


def path_digests(proof):
    """digests in the path section of every tree (trace, composition, the layers), read from the counts the proof states"""
    b = bytes(proof)
    compact = b[:4] == b"CSTC"
    air, width, log_n, _ = struct.unpack_from("<4I", b, 8)
    nq, blowup, _, _, ext, folding, _ = struct.unpack_from("<7I", b, 24)
    em, log_N, log_f = ext + 1, log_n + blowup.bit_length() - 1, folding.bit_length() - 1
    nl = struct.unpack_from("<I", b, 116)[0]
    o = 120 + 32 * nl + 32 + 8 * (2 * width + CE[air]) * em + 8
    out = []

    def tree(o, count, row_bytes, depth):
        o += count * row_bytes
        n = struct.unpack_from("<I", b, o)[0] if compact else count * depth
        out.append(n)
        return o + (4 if compact else 0) + 32 * n

    o = tree(o, nq, 8 * width, log_N)
    o = tree(o, nq, 8 * CE[air] * em, log_N)
    lg = log_N
    for _ in range(nl):
        npos = struct.unpack_from("<I", b, o)[0]
        lg -= log_f
        o = tree(o + 4, npos, 8 * folding * em, lg)
    return out


def both_forms(b, prove, plain_only):
    b.proof_form = "plain"
    plain = prove()
    if plain_only:
        return plain, None
    b.proof_form = "compact"
    try:
        return plain, prove()
    finally:
        b.proof_form = "plain"


def size_row(name, plain, compact):
    row = {"config": name, "plain_bytes": len(plain), "plain_digests": path_digests(plain)}
    if compact is not None:
        row.update(compact_bytes=len(compact), compact_digests=path_digests(compact))
    return row


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
    """turns: {name: call}; -> {name: {"ms": median, "rounds": [...], "spread": max - min}}"""
    got = {k: [] for k in turns}
    for _ in range(rounds):
        for k, call in turns.items():
            got[k].append(timed(call, seconds))
    return {k: {"ms": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v], "spread": round(max(v) - min(v), 4)} for k, v in got.items()}


def judge(res):
    if "compact" not in res:
        return None
    d, spread = res["compact"]["ms"] - res["plain"]["ms"], res["plain"]["spread"]
    return "no difference" if abs(d) <= spread else "%+.4f ms" % d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--skip-sizes", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    b = Backend()
    if args.plain_only:
        type(b).proof_form = "plain"   # a library from before the form: nothing to set
    meta = TransactionMetadata.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))
    out = {"device": "MI355X", "rounds": args.rounds, "seconds_per_turn": args.seconds, "sizes": [], "verify": {}, "prove": {}}
    head = ProofOptions(96, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)
    tx = TransactionExample(head, meta, b)
    plain, compact = both_forms(b, tx.prove, args.plain_only)
    out["sizes"].append(size_row("state_transition 1024 tx (2^20 rows), (96, 8, 0, Blake3, None, 4, 256)", plain, compact))
    if not args.skip_sizes:
        for name, o in (("Sha3", (96, 8, 0, 1, 0, 4, 256)), ("quadratic", (96, 8, 0, 0, 1, 4, 256)), ("cubic", (96, 8, 0, 0, 2, 4, 256))):
            po = ProofOptions(*o)
            out["sizes"].append(size_row("state_transition 1024 tx, %s %r" % (name, o), *both_forms(b, lambda: b.prove(po), args.plain_only)))
        po = ProofOptions(42, 8, 0, 0, 0, 4, 256)
        words = (np.arange(1, 1025, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.array([0] * 1023 + [1], np.uint64)
        out["sizes"].append(size_row("range 2^16 rows, (42, 8, 0, Blake3, None, 4, 256)", *both_forms(b, lambda: b.range_prove_bits(po, words, 16), args.plain_only)))
        sex = SchnorrExample.build_random(po, 512, backend=b)
        out["sizes"].append(size_row("schnorr 512 signatures (2^18 rows), (42, 8, 0, Blake3, None, 4, 256)", *both_forms(b, sex.prove, args.plain_only)))
        b.upload_witness(meta)         # the headline witness again for the timed proofs
    r0, r1 = tx.pub_inputs()
    for count in (1, 64):
        turns, h2d = {}, {}
        for form, proof in (("plain", plain), ("compact", compact)):
            if proof is None:
                continue
            proofs = [proof] * count
            assert not b.tx_verify(proofs, r0, r1, head).any()
            h2d[form] = b.verify_h2d_bytes()
            turns[form] = (lambda ps: lambda: b.tx_verify(ps, r0, r1, head))(proofs)
        res = alternate(turns, args.rounds, args.seconds)
        res["h2d_bytes"] = h2d
        res["compact_vs_plain"] = judge(res)
        out["verify"][str(count)] = res

    def prove_in(form):
        def run():
            b.proof_form = form
            b.prove(head)
        return run
    turns = {"plain": prove_in("plain")} if args.plain_only else {"plain": prove_in("plain"), "compact": prove_in("compact")}
    res = alternate(turns, args.rounds, args.seconds * 2)
    channels = {}
    for form, run in turns.items():
        run()
        channels[form] = b.prove_channel()
    b.proof_form = "plain"
    res["channel"] = channels
    res["compact_vs_plain"] = judge(res)
    out["prove"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
