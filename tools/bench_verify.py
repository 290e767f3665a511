"""Verification throughput at the headline configuration (1024 transfers = 2^20 rows, depth 15; 96 queries, blowup 8, folding 4,
remainder 256): single-proof latency, proofs/s at batch sizes 16, 64 and 256, bytes copied per call (proof bytes and the whole copy)
and the achieved host-to-device rate of the whole copy, and cstark_verify_stage_ms.  Prints one JSON line.  Run on a GPU box.

    python tools/bench_verify.py [--counts 1,64] [--min-seconds 1.0] [--air transaction|merkle|range|schnorr] [--signatures 1]

--air merkle: a MerkleAir proof of 512 transfers (2^18 rows, depth 15, 96 queries); --air range: the reference's 64-row range proof
(42 queries); both through cstark_air_verify.  --air schnorr: a SchnorrAir proof of --signatures signatures (1: 2^9 rows, counts 1, 64, 1024;
512: 2^18 rows, count 1; 42 queries) through cstark_schnorr_verify; its statement (304 bytes per signature) is part of the copy.

The verify calls are synchronous (verdicts are on the host when they return), so wall time around the call is the latency; every
configuration is warmed up first and timed over at least --min-seconds of calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from certificate_stark_amd.backend import Backend  # noqa: E402
from certificate_stark_amd.prover import (MerkleExample, ProofOptions, RangeProofExample, SchnorrExample, TransactionExample,  # noqa: E402
                                           TransactionMetadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCIE_GEN5_X16_GBPS = 63.0  # per direction, MI355X spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,16,64,256")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--air", default="transaction", choices=("transaction", "merkle", "range", "schnorr"))
    ap.add_argument("--signatures", type=int, default=1)
    args = ap.parse_args()
    b = Backend()
    meta = None if args.air in ("range", "schnorr") else TransactionMetadata.load(os.path.join(ROOT, "tests", "golden", "witness_1024_d15.npz"))
    if args.air == "transaction":
        opt = ProofOptions(96, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)
        tx = TransactionExample(opt, meta, b)
        proof = tx.prove()
        r0, r1 = tx.pub_inputs()
        config = "state_transition 1024 tx (2^20 rows), depth 15, options (96, 8, 0, Blake3, None, 4, 256)"

        def verify(proofs):
            return b.tx_verify(proofs, r0, r1, opt)
    elif args.air == "merkle":
        opt = ProofOptions(96, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)
        half = TransactionMetadata(*[getattr(meta, f) if f == "final_root" else getattr(meta, f)[:512] for f in TransactionMetadata.FIELDS])
        proof = MerkleExample(opt, half, b).prove()
        pub = np.concatenate([meta.initial_roots[0], meta.initial_roots[512]])  # the tree's root before and after the first 512 transfers
        config = "merkle_update 512 tx (2^18 rows), depth 15, options (96, 8, 0, Blake3, None, 4, 256)"

        def verify(proofs):
            return b.air_verify(proofs, Backend.AIR_MERKLE, pub, opt)
    elif args.air == "schnorr":
        opt = ProofOptions(42, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)
        ex = SchnorrExample.build_random(opt, args.signatures, backend=b)
        proof = ex.prove()
        config = "schnorr %d signatures (%d rows), options (42, 8, 0, Blake3, None, 4, 256)" % (args.signatures, 512 * args.signatures)

        def verify(proofs):
            return b.schnorr_verify(proofs, [ex] * len(proofs), opt)
    else:
        opt = ProofOptions(42, 8, 0, ProofOptions.BLAKE3_256, ProofOptions.EXT_NONE, 4, 256)
        p = (1 << 62) + (1 << 56) + (1 << 55) + 1
        number = 12345678901234567 * pow(2, 64, p) % p   # memory form
        proof = RangeProofExample(opt, number, b).prove()
        config = "range 64 rows, options (42, 8, 0, Blake3, None, 4, 256)"

        def verify(proofs):
            return b.air_verify(proofs, Backend.AIR_RANGE, options=opt, numbers=number)
    out = {"config": config, "proof_bytes": len(proof), "device": "MI355X", "results": {}}
    for count in [int(c) for c in args.counts.split(",")]:
        proofs = [proof] * count
        for _ in range(3):  # warm-up: staging buffers, periodic coefficients, code objects
            v = verify(proofs)
        assert not v.any(), v
        calls, t0 = 0, time.perf_counter()
        while True:
            verify(proofs)
            calls += 1
            dt = time.perf_counter() - t0
            if dt >= args.min_seconds:
                break
        per_call = dt / calls
        st = b.verify_stage_ms()
        nbytes = count * len(proof)
        copied = b.verify_h2d_bytes()   # the one host-to-device copy: proof bytes + descriptors + opening records
        out["results"][str(count)] = {
            "calls": calls, "ms_per_call": round(per_call * 1e3, 4), "proofs_per_s": round(count / per_call, 1),
            "proof_bytes_per_call": nbytes, "h2d_bytes_per_call": copied,
            "h2d_gbps": round(copied / (st["h2d"] * 1e-3) / 1e9, 2) if st["h2d"] > 0 else None,
            "link_share": round(copied / (st["h2d"] * 1e-3) / 1e9 / PCIE_GEN5_X16_GBPS, 3) if st["h2d"] > 0 else None,
            "stage_ms": {k: round(v, 4) for k, v in st.items()},
        }
    if "1" in out["results"]:
        out["single_proof_latency_ms"] = out["results"]["1"]["ms_per_call"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
