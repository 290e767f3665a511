"""The CPU half of the sub-AIR cheating prover (cheating_sub_airs.py): every proof it builds is rejected by the restated verifier
(oracle/verifier.py) at exactly the check the deviation was aimed at.  test_gpu_air_verify.py gives the same proofs to
cstark_air_verify."""
import pytest

import cheating_sub_airs as CS


def test_honest_sub_air_proofs_are_accepted():
    for air in (CS.MERKLE, CS.RANGE, CS.RESCUE):
        proof, pub = CS.honest(air, CS.OPTIONS[air])
        assert CS.verify(air, proof, pub, options=list(CS.OPTIONS[air]))


def test_every_cheat_is_rejected_by_its_own_check():
    from oracle import verifier as V
    cases = CS.isolating_cases()
    assert sum(name.startswith("invalid_trace") for name in cases) == 10 and sum(name.startswith("lying") for name in cases) == 3
    for name, (air, proof, pub, verdict, part) in cases.items():
        with pytest.raises(V.VerifierError) as e:
            CS.verify(air, proof, pub)
        assert part in str(e.value), (name, str(e.value))


def test_lying_statement_is_consistent_but_for_the_boundary_terms():
    """against the statement the trace really holds the transcript differs (another seed): the lie is in the proof, not only in the call"""
    from oracle import verifier as V
    for air in (CS.MERKLE, CS.RANGE, CS.RESCUE):
        _, truth = CS.honest(air, CS.OPTIONS[air])
        proof, lie = CS.lying_statement(air, CS.OPTIONS[air])
        word = 0 if air == CS.RANGE else 7
        assert (int(lie[word]) - int(truth[word])) % CS.P == CS._one() and all(int(a) == int(b) for k, (a, b) in enumerate(zip(lie, truth)) if k != word)
        for pub in (lie, truth):
            with pytest.raises(V.VerifierError, match="out-of-domain"):
                CS.verify(air, proof, pub)


def test_byte_view_covers_every_section():
    proof, _ = CS.honest(CS.RANGE, (8, 8, 0, 1, 2, 8, 128))
    L = CS.layout(proof)
    assert L["n_layers"] == 1 and L["m"] == 3
    offs = CS.tamper_offsets(proof)
    assert len(set(offs.values())) == len(offs) and all(52 < o < len(proof) for o in offs.values())
    for sec in CS.element_sections(proof):
        assert not CS.words_canonical(CS.noncanonical(proof, sec))
    proof, _ = CS.honest(CS.RANGE, (8, 2, 0, 0, 1, 4, 128))
    assert CS.layout(proof)["n_layers"] == 0 and CS.layout(proof)["rem_len"] == 128
