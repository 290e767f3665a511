"""cstark_proof_inspect (the verifier's host parser) and the verdict table, on the CPU: no GPU, no context."""
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "proof_2tx_d3.npz")
MALFORMED = 1


@pytest.fixture(scope="module")
def golden():
    return bytes(np.load(GOLDEN)["proof"].tobytes())


def _inspect(p):
    from certificate_stark_amd import inspect_proof
    return inspect_proof(p)


def _sections(p):
    """byte offsets of every section boundary (restated here from the layout in include/cstark.h)"""
    info = _inspect(p)
    nq, blowup, _, _, ext, fold, _ = info.options
    m, W, ce = ext + 1, 94, 8
    log_N, log_f = info.log_n + blowup.bit_length() - 1, fold.bit_length() - 1
    nl = struct.unpack_from("<I", p, 116)[0]
    o, cuts, counts = 52, [0, 4, 8, 12, 16, 20, 24, 52], {}
    o += 64; cuts.append(o)
    counts["n_layers"] = o
    o += 4 + 32 * nl + 32; cuts.append(o)
    o += 8 * (2 * W + ce) * m; cuts.append(o)
    o += 8; cuts.append(o)
    for words in (nq * W, nq * log_N * 4, nq * ce * m, nq * log_N * 4):
        o += 8 * words; cuts.append(o)
    lg = log_N
    for l in range(nl):
        counts["n_positions_%d" % l] = o
        npos = struct.unpack_from("<I", p, o)[0]
        o += 4; cuts.append(o)
        o += 8 * npos * fold * m; cuts.append(o)
        o += 32 * npos * (lg - log_f); cuts.append(o)
        lg -= log_f
    counts["remainder_len"] = o
    rem_len = struct.unpack_from("<I", p, o)[0]
    o += 4; cuts.append(o)
    o += 8 * rem_len * m
    assert o == len(p)
    cuts.append(o)
    return cuts, counts


def test_golden_proof_header(golden):
    info = _inspect(golden)
    assert info.verdict == 0
    assert info.options == [42, 8, 0, 0, 0, 4, 256]
    assert info.log_n == 11 and info.depth == 3 and info.air == 0 and info.trace_width == 94


@pytest.mark.parametrize("options", [
    (16, 8, 0, 1, 0, 4, 256),    # Sha3_256
    (8, 8, 0, 0, 1, 4, 256),     # Quadratic
    (8, 16, 0, 0, 2, 4, 256),    # Cubic, blowup 16
    (8, 8, 0, 0, 0, 8, 128),     # folding 8, remainder 128
    (8, 8, 0, 0, 0, 16, 1024),   # folding 16, remainder 1024
    (8, 8, 6, 1, 2, 16, 512),    # grinding, Sha3, Cubic
])
def test_cpu_prover_proofs_read_back(oracle, witness_d3, options):
    from oracle import prover as OP
    p = OP.prove(witness_d3, options)
    info = _inspect(p)
    assert info.verdict == 0
    assert info.options == list(options)
    assert info.log_n == 11 and info.depth == 3 and info.air == 0
    # every section boundary was derived from the header and the counts alone
    cuts, _ = _sections(p)
    assert cuts[-1] == len(p)


def test_other_airs_read_back(oracle, witness_d3):
    from oracle import prover as OP
    merkle = OP.prove_air(oracle.AIR_MERKLE, witness_d3, (8, 8, 0, 0, 0, 4, 128))
    info = _inspect(merkle)
    assert (info.verdict, info.air, info.trace_width, info.header_word) == (0, 1, 65, 3)
    rng = OP.prove_air(oracle.AIR_RANGE, 12345, (8, 8, 0, 0, 0, 4, 128))
    info = _inspect(rng)
    assert (info.verdict, info.air, info.trace_width, info.log_n) == (0, 3, 2, 6)
    assert info.options == [8, 8, 0, 0, 0, 4, 128]


def test_writer_and_parser_share_one_layout(golden, tmp_path):
    """csrc/proof_layout.h alone (g++, host code only): write_proof -> parse_layout round trips over the five AIRs, the three extension
    degrees and folding factors, with and without FRI layers; a pinned proof, parsed and written again from its sections, is the same
    bytes; a buffer one byte short stays untouched and the needed length is reported (tests/cpp/proof_layout_check.cpp)."""
    import subprocess
    exe, dump = str(tmp_path / "proof_layout_check"), str(tmp_path / "proof.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "proof_layout_check.cpp")])
    with open(dump, "wb") as f:
        f.write(golden)
    out = subprocess.run([exe, dump], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok") and "golden proof rewritten byte for byte" in out.stdout, out.stdout + out.stderr


def test_air_groups_match_the_shapes(tmp_path):
    """csrc/air_groups.h alone (g++, host code only): the degree and divisor groups and the per-coset powers that the generic merge of
    the sub-AIRs works from, against each AIR's shape stated directly; shapes with too many groups are refused
    (tests/cpp/air_groups_check.cpp)."""
    import subprocess
    exe = str(tmp_path / "air_groups_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "air_groups_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: 18 groupings checked"), out.stdout + out.stderr


@pytest.fixture(scope="module")
def transcript_check(tmp_path_factory):
    """tests/cpp/transcript_check.cpp: csrc/transcript.h and csrc/proof_layout.h alone under g++ (host code only)"""
    import subprocess
    exe = str(tmp_path_factory.mktemp("transcript") / "transcript_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "transcript_check.cpp")])
    return exe


def _transcript_case(name, oracle, witness_d3):
    """proof, the AIR as the restated verifier sees it, and the call that verifies the proof with a probe"""
    from oracle import prover as OP
    from oracle import verifier as V
    if name == "golden":   # TransactionAir, Blake3, base field
        z = np.load(GOLDEN)
        proof, r0, r1 = bytes(z["proof"].tobytes()), z["initial_root"], z["final_root"]
        return proof, V._TxAir(V.parse(proof), r0, r1), lambda probe: V.verify(proof, r0, r1, probe=probe)
    options = {"range_sha3_pow": (30, 8, 3, 1, 0, 4, 128),        # Sha3, 3 bits of proof of work, one FRI layer
               "range_quadratic": (20, 8, 0, 0, 1, 4, 1024)}[name]   # quadratic extension, no layer
    number = int(oracle.to_mont(np.array([0x1234567890ABCDEF], np.uint64))[0])
    proof = OP.prove_air(oracle.AIR_RANGE, number, options)
    return proof, V._RangeAir(V.parse(proof), number), lambda probe: V.verify_range(proof, number, options=list(options), probe=probe)


@pytest.mark.parametrize("case", ["golden", "range_sha3_pow", "range_quadratic"])
def test_host_transcript_draws_what_the_restated_verifier_draws(oracle, witness_d3, transcript_check, tmp_path, case):
    """csrc/transcript.h, the steps every host-channel prover calls, replayed from a proof's own roots, frame, layer roots, remainder
    and nonce: EVERY value drawn -- coefficients, z, DEEP coefficients, FRI folding points, query positions and each layer's folded
    positions -- equals what oracle/verifier.py draws for the same proof.  The values, not only the positions: every reseed resets the
    draw counter, so a step with a wrong number of draws leaves no trace in what is drawn after it."""
    import subprocess
    from oracle import verifier as V
    proof, air, verify = _transcript_case(case, oracle, witness_d3)
    probe = {}
    assert verify(probe)
    dump = str(tmp_path / "proof.bin")
    with open(dump, "wb") as f:
        f.write(proof)
    pub = [str(int(v)) for v in oracle.to_mont(np.array(air.pub, np.uint64))]
    out = subprocess.run([transcript_check, dump, str(air.nc), str(air.na)] + pub, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {}
    for ln in out.stdout.splitlines():
        name, *vals = ln.split()
        got[name] = [int(v) for v in vals]

    d = V.parse(proof)
    m, nq, n_layers = d["options"][4] + 1, d["options"][0], len(d["layer_roots"])
    flat = lambda elems: [int(w) for e in elems for w in (e if isinstance(e, tuple) else (e,))]
    ta, tb, ba, bb = probe["coefficients"]
    d_alpha, d_beta, d_delta, deg_a, deg_b = probe["deep"]
    want = {"t_alpha": flat(ta), "t_beta": flat(tb), "b_alpha": flat(ba), "b_beta": flat(bb), "z": flat([probe["z"]]),
            "deep_alpha": flat(d_alpha), "deep_beta": flat(d_beta), "deep_delta": flat(d_delta), "deg_a": flat([deg_a]), "deg_b": flat([deg_b]),
            "layer_points": flat(probe["layer_points"]), "positions": list(probe["positions"])}
    assert len(want["t_alpha"]) == m * air.nc and len(want["b_beta"]) == m * air.na and len(want["deep_alpha"]) == m * air.width
    assert len(want["deep_delta"]) == m * air.ce and len(want["layer_points"]) == m * n_layers and len(want["positions"]) == nq
    log_N, log_f = d["log_n"] + d["options"][1].bit_length() - 1, d["options"][5].bit_length() - 1
    cur, counts = want["positions"], []
    for l in range(n_layers):
        cur = V.fold_positions(cur, 1 << (log_N - (l + 1) * log_f))
        want["folded_%d" % l] = cur
        counts.append(len(cur))
        assert len(d["layers"][l][0]) == len(cur)
    want["folded_counts"] = counts
    assert {"golden": 2, "range_sha3_pow": 1, "range_quadratic": 0}[case] <= n_layers and (case != "range_quadratic" or n_layers == 0)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_truncations_are_malformed(golden):
    cuts, _ = _sections(golden)
    lengths = set()
    for c in cuts:
        lengths.update((c - 1, c, c + 1))
    rng = np.random.default_rng(7)
    lengths.update(int(v) for v in rng.integers(0, len(golden), 500))
    for n in sorted(lengths):
        if 0 <= n < len(golden):
            assert _inspect(golden[:n]).verdict == MALFORMED, n
    assert _inspect(golden + b"\0").verdict == MALFORMED


def test_count_words_are_checked_before_use(golden):
    nq = 42
    _, counts = _sections(golden)
    assert len(counts) >= 3
    for name, off in counts.items():
        for v in (0, nq + 1, 1 << 31, (1 << 32) - 1):
            bad = bytearray(golden)
            struct.pack_into("<I", bad, off, v)
            assert _inspect(bytes(bad)).verdict == MALFORMED, (name, v)


@pytest.mark.parametrize("off,value", [
    (0, 0x4B545344),        # magic
    (4, 2),                 # version
    (8, 5),                 # air id
    (12, 93),               # trace width
    (24 + 4 * 5, 2),        # folding factor
    (24 + 4 * 5, 32),
    (24 + 4 * 1, 4),        # blowup below the AIR's constraint-evaluation blowup
    (24 + 4 * 1, 3),
    (24 + 4 * 0, 0),        # no queries
    (24 + 4 * 4, 3),        # field extension
    (24 + 4 * 2, 33),       # grinding
    (20, 4),                # Merkle depth the prover refuses
])
def test_bad_header_words_are_malformed(golden, off, value):
    bad = bytearray(golden)
    struct.pack_into("<I", bad, off, value)
    assert _inspect(bytes(bad)).verdict == MALFORMED


def test_empty_and_tiny_inputs(golden):
    assert _inspect(b"").verdict == MALFORMED
    assert _inspect(b"CSTK").verdict == MALFORMED
    assert _inspect(golden[:52]).verdict == MALFORMED


def test_verdict_table_matches_the_header():
    from certificate_stark_amd import VERDICTS
    hdr = open(os.path.join(ROOT, "include", "cstark.h")).read()
    body = hdr[hdr.index("typedef enum cstark_verdict"):]
    body = body[:body.index("} cstark_verdict;")]
    pairs = re.findall(r"CSTARK_PROOF_([A-Z_]+)\s*=\s*(\d+)", body)
    assert len(pairs) == 14
    assert [int(v) for _, v in pairs] == list(range(14))
    assert tuple(n for n, _ in pairs) == VERDICTS


def test_verifier_error_carries_verdict_and_reason():
    from certificate_stark_amd import VerifierError
    e = VerifierError(4)
    assert e.verdict == 4 and e.reason == "OOD"
