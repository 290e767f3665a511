"""The cheating SchnorrAir prover of cheating_schnorr.py against the restated verifier (oracle/verifier.py, verify_schnorr), on the CPU:
the honest control is accepted and every deviation is rejected by the one check it isolates, with the reason test_gpu_schnorr_verify.py
expects of the product verifier."""
import pytest

import cheating_schnorr as CS


def test_control_is_accepted(oracle):
    proof, w = CS.honest()
    assert CS.verify(proof, w, options=list(CS.OPTIONS))
    assert CS.oracle_verdict(proof, w) == "OK"


def test_every_deviation_is_rejected_for_its_own_reason(oracle):
    from oracle import verifier as V
    for name, (proof, w, verdict, message) in CS.isolating_cases().items():
        with pytest.raises(V.VerifierError) as e:
            CS.verify(proof, w)
        assert message in str(e.value), (name, str(e.value))
        assert CS.oracle_verdict(proof, w) == verdict, name


def test_lie_is_what_is_rejected(oracle):
    """the proof of a lying prover is rejected against the lie (above) and against the truth alike: its seed is the lie's"""
    proof, lie = CS.lying_statement("rx")
    assert CS.oracle_verdict(proof, CS.witness()) != "OK" and CS.oracle_verdict(proof, lie) == "OOD"


def test_another_number_of_signatures(oracle):
    proof, w = CS.honest()
    with pytest.raises(Exception) as e:
        CS.verify(proof, CS.witness(2))
    assert "different number of signatures" in str(e.value) and CS.oracle_verdict(proof, CS.witness(2)) == "OOD"
