"""CPU: the compact proof form against Python references (tests/compact_cases.py) and the host parser (cstark_proof_inspect,
cstark_proof_form); csrc/proof_layout.h's writer and parser on their own (tests/cpp/proof_compact_check.cpp, g++).

Inputs: the CPU oracle's proofs of two transfers (depth 3) at four option sets -- Blake3 and Sha3, base field, quadratic and cubic,
folding 4, 8 and 16 -- and of RangeProofAir at five: two without any FRI layer, and 128 queries into a 64-leaf layer tree.  The
positions are the CPU verifier's.  Path digests, plain -> compact, of the range proofs: 672 -> 174, 1008 -> 294, 896 -> 94,
2414 -> 181, 2896 -> 626 (asserted below)."""
import os
import struct
import subprocess

import pytest

import compact_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("tx",) + (o,) for o in CC.TX_OPTS] + [("range",) + (o,) for o in CC.RANGE_OPTS]
RANGE_DIGESTS = {CC.RANGE_OPTS[0]: (672, 174), CC.RANGE_OPTS[1]: (1008, 294), CC.RANGE_OPTS[2]: (896, 94), CC.RANGE_OPTS[3]: (2414, 181),
                 CC.RANGE_OPTS[4]: (2896, 626)}


def case(kind, opts):
    return CC.tx_case(2, 3, opts) if kind == "tx" else CC.range_case(opts)


def oracle_accepts(oracle, kind, proof, opts):
    from oracle import verifier as V
    if kind == "tx":
        w = CC.witness(2, 3)
        return V.verify(proof, w.initial_roots[0], w.final_root, options=list(opts))
    return V.verify_range(proof, CC.range_number(), options=list(opts))


def test_multiproof_nodes_by_hand():
    # depth 3, leaves 2 and 3 are siblings, 6 is alone: level 3 gives (3, 7); level 2: parents 1 and 3 -> (2, 0), (2, 2); level 1: 0, 1 paired
    assert CC.multiproof_nodes(3, [6, 2, 3]) == [(3, 7), (2, 0), (2, 2)]
    assert CC.multiproof_nodes(3, [5]) == [(3, 4), (2, 3), (1, 0)]               # one position: its path
    assert CC.multiproof_nodes(2, [0, 1, 2, 3]) == []                            # every leaf: nothing to add
    assert CC.multiproof_nodes(3, [1, 1, 1]) == CC.multiproof_nodes(3, [1])      # over the distinct positions


@pytest.mark.parametrize("kind,opts", CASES)
def test_compact_round_trip_and_length(oracle, kind, opts):
    plain, positions = case(kind, opts)
    assert len(set(positions)) == len(positions) == opts[0]
    compact = CC.compact(plain, positions)
    assert compact[:4] == b"CSTC" and compact[4:52] == plain[4:52]
    back = CC.expand(compact, positions, opts[3])
    assert back == plain
    assert oracle_accepts(oracle, kind, back, opts)
    form, trees, _ = CC.walk(plain)
    n_plain, n_multi = CC.path_digests(plain), CC.path_digests(compact)
    assert n_multi == sum(len(CC.multiproof_nodes(t.depth, pos)) for t, pos in zip(trees, CC.tree_positions(plain, positions)))
    assert len(compact) == len(plain) - 32 * (n_plain - n_multi) + 4 * len(trees)
    if kind == "range":
        assert (n_plain, n_multi) == RANGE_DIGESTS[opts]


def test_the_edge_cases_these_shapes_contain(oracle):
    # no FRI layer at all: two trees
    for opts in (CC.RANGE_OPTS[0], CC.RANGE_OPTS[2]):
        assert len(CC.walk(CC.range_case(opts)[0])[1]) == 2
    # 128 queries at blowup 4, folding 4: the layer tree has 64 leaves, 61 of them opened, 3 proof nodes
    plain, positions = CC.range_case(CC.RANGE_OPTS[3])
    trees = CC.walk(plain)[1]
    layer, lpos = trees[2], CC.tree_positions(plain, positions)[2]
    assert (layer.depth, layer.count, len(CC.multiproof_nodes(layer.depth, lpos))) == (6, 61, 3)
    # trees with levels that contribute no node
    for t, pos in zip(trees, CC.tree_positions(plain, positions)):
        levels = {l for l, _ in CC.multiproof_nodes(t.depth, pos)}
        assert len(levels) < t.depth, t.name


@pytest.mark.parametrize("kind,opts", CASES)
def test_host_parser_reads_the_compact_form(oracle, kind, opts):
    from certificate_stark_amd.verify import inspect_proof, proof_form
    plain, positions = case(kind, opts)
    compact = CC.compact(plain, positions)
    assert proof_form(plain) == "plain" and proof_form(compact) == "compact"
    a, b = inspect_proof(plain), inspect_proof(compact)
    assert a.ok and b.ok
    assert (b.air, b.trace_width, b.log_n, b.header_word, b.options) == (a.air, a.trace_width, a.log_n, a.header_word, a.options)
    assert b.options == list(opts) and b.air == (0 if kind == "tx" else 3)
    assert not inspect_proof(compact + b"\0").ok                                 # one trailing byte
    # each body under the other magic.  For every shape here the two forms differ in length (the multiproofs save more than the
    # 4 bytes per tree they add), so neither body has the length the other form's walk arrives at: MALFORMED
    assert len(compact) != len(plain)
    assert not inspect_proof(b"CSTK" + compact[4:]).ok
    assert not inspect_proof(b"CSTC" + plain[4:]).ok
    # an n_nodes word above n_positions * depth, in every tree
    for t in CC.walk(compact)[1]:
        bad = bytearray(compact)
        struct.pack_into("<I", bad, t.paths - 4, t.count * t.depth + 1)
        assert not inspect_proof(bytes(bad)).ok, t.name
    with pytest.raises(ValueError):
        proof_form(b"CSTX" + plain[4:])
    with pytest.raises(ValueError):
        proof_form(b"CS")


@pytest.mark.parametrize("kind,opts", [("range", CC.RANGE_OPTS[2]), ("range", CC.RANGE_OPTS[3]), ("tx", CC.TX_OPTS[2])])
def test_host_parser_refuses_every_truncation(oracle, kind, opts):
    """every length below the proof's: no FRI layer (Blake3), one layer (Sha3, cubic), and a TransactionAir proof with layers"""
    from certificate_stark_amd.verify import inspect_proof
    compact = CC.compact(*case(kind, opts))
    step = 1 if len(compact) < 40000 else 7      # (the TransactionAir proof: every 7th length and the last 600)
    cuts = list(range(0, len(compact), step)) + list(range(max(0, len(compact) - 600), len(compact)))
    assert all(not inspect_proof(compact[:n]).ok for n in cuts)


def test_writer_and_parser_of_the_compact_form(tmp_path):
    """tests/cpp/proof_compact_check.cpp: write_proof's selection against an independent walk, parse_layout's offsets against the
    writer's, the refusals of the parser; positions that repeat and single queries included"""
    exe = str(tmp_path / "proof_compact_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "proof_compact_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok 162 shapes"), out.stdout + out.stderr
