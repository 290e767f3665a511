"""csrc/ledger_plan.h on steered batches (ledger_scenarios.py) against the plain model (ledger_model.py): first the model itself against
every generated case, then every scenario and every refusal through tests/cpp/ledger_plan_check.cpp (built with AddressSanitizer and
UBSan, as test_ledger_cpu.py builds it), with the model's arrays as the expectation."""
import os
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import ledger_scenarios as LS

ROOT = LC.ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ledger_steered") / "ledger_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_plan_check.cpp")])
    return exe


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_model_reproduces_the_generator(case):
    """before any steered expectation is trusted: the model gives the generator's eleven arrays, bit for bit"""
    w = LC.generated(case)
    indices, initial = LC.initial_accounts(w)
    m = LM.LedgerModel(w.depth)
    m.set_accounts(indices, initial)
    assert np.array_equal(m.root(), w.initial_roots[0])
    got = m.apply(w.s_indices, w.r_indices, w.deltas, w.sig_rx, w.sig_s)
    assert (got.n_tx, got.depth) == (w.n_tx, w.depth)
    for f in w.FIELDS:
        assert np.array_equal(getattr(got, f), getattr(w, f)), f
    assert np.array_equal(m.root(), w.final_root)
    assert np.array_equal(m.accounts(indices), LC.final_accounts(w, indices))


def test_model_refusals_leave_it_unchanged():
    for sc, at, reason in LS.REFUSALS:
        m = LS.model(sc)
        root, values = m.root(), m.accounts(sc.indices())
        assert m.apply(*LS.transfers(sc)) == (at, reason), sc.name
        assert np.array_equal(m.root(), root) and np.array_equal(m.accounts(sc.indices()), values), sc.name
        if at:
            assert not isinstance(m.apply(*LS.transfers(sc, 0, at)), tuple), sc.name


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_model_witness_satisfies_the_merkle_update_constraints(sc):
    """the model's arrays are a valid MerkleAir witness (the oracle's prover and restated verifier, src/merkle/update/air.rs:104-126), for
    its own roots and for no other scenario's"""
    from oracle import oracle as O, prover as OP, verifier as Vf
    options = (8, 4, 0, 0, 0, 4, 128)
    e = LS.expected(sc.proof_form())
    other = LS.expected(LS.SCENARIOS[(LS.SCENARIOS.index(sc) + 1) % len(LS.SCENARIOS)].proof_form())
    proof = OP.prove_air(O.AIR_MERKLE, e.witness, options)
    assert Vf.verify_merkle(proof, e.initial_root, e.final_root, options=list(options))
    for wrong in ((e.initial_root, other.final_root), (other.initial_root, e.final_root)):
        with pytest.raises(Vf.VerifierError):
            Vf.verify_merkle(proof, *wrong, options=list(options))


def _run(checker, path):
    return subprocess.run([checker, path], capture_output=True, text=True)


def _write_applied(path, sc, witness=None):
    e = LS.expected(sc)
    assert e.refusal is None, sc.name
    LC.write_case(path, witness or e.witness, accounts=(sc.indices(), LS.values(sc), e.final_values))


@pytest.mark.parametrize("sc", LS.SCENARIOS + LS.ACCEPTED, ids=lambda sc: sc.name)
def test_plan_reproduces_the_model(checker, sc, tmp_path):
    path = str(tmp_path / "case.bin")
    _write_applied(path, sc)
    out = _run(checker, path)
    assert out.returncode == 0 and out.stdout.startswith("ok: depth %d, %d accounts, %d transfers," % (sc.depth, len(sc.accounts), sc.n_tx)), out.stdout + out.stderr


@pytest.mark.parametrize("sc,at,reason", LS.REFUSALS, ids=lambda v: getattr(v, "name", None))
def test_plan_refuses_where_the_model_does(checker, sc, at, reason, tmp_path):
    assert LS.expected(sc).refusal == (at, reason), "the model disagrees with the scenario's stated refusal"
    # the arrays of the valid prefix, in a witness of the whole batch's shape
    O = LM._oracle()
    w = O.TxWitness(sc.n_tx, sc.depth)
    w.s_indices[:], w.r_indices[:], w.deltas[:] = LS.transfers(sc)[:3]
    w.initial_roots[0] = LS.expected(sc).initial_root
    final = LS.values(sc)
    if at:
        e = LS.expected(sc.prefix(at))
        for f in ("initial_roots", "s_old_values", "r_old_values", "s_paths", "r_paths"):
            getattr(w, f)[:at] = getattr(e.witness, f)
        w.initial_roots[at] = e.final_root
        final = e.final_values
    path = str(tmp_path / "case.bin")
    LC.write_case(path, w, accounts=(sc.indices(), LS.values(sc), final), refusal=(at, reason))
    out = _run(checker, path)
    assert out.returncode == 0 and "refused at %d of %d (reason %d)" % (at, sc.n_tx, reason) in out.stdout, out.stdout + out.stderr
    # the comparison is live: another position or another reason fails it
    other = (at, reason % 4 + 1) if at == 0 else (at - 1, reason)
    LC.write_case(path, w, accounts=(sc.indices(), LS.values(sc), final), refusal=other)
    out = _run(checker, path)
    assert out.returncode == 1 and "the steered batch: refused_at %d reason %d" % (at, reason) in out.stdout, out.stdout + out.stderr


def test_checker_notices_a_wrong_steered_witness(checker, tmp_path):
    """the comparison is live: one flipped word of a bystander's digest, read as a sibling, fails the check"""
    sc = LS.BY_NAME["bystander_siblings"]
    w = LS.expected(sc).witness.copy()
    assert sc.transfers[0][0] == 10 and 8 in sc.bystanders() and 9 in sc.bystanders()
    w.s_paths[0, 2, 4] ^= np.uint64(1)      # path[2]: the sibling of leaf 10 at level depth - 1, the parent of the bystanders 8 and 9
    path = str(tmp_path / "case.bin")
    _write_applied(path, sc, witness=w)
    out = _run(checker, path)
    assert out.returncode == 1 and "s_paths differ" in out.stdout, out.stdout + out.stderr
