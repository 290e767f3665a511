"""cstark_schnorr_sign (Backend.schnorr_sign) against the reference signer's first-accepted result (sign_cases.Signed): signatures,
attempts_out and exhaustion, whatever max_attempts lets the device run together; proofs made after a signing call are the proofs made
without it; SchnorrExample.sign gives an example that proves and verifies."""
import random

import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC
import sign_cases as SG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _assert_signed(got, ref):
    rx, s, attempts, status = got
    assert np.array_equal(status, ref.status), (status, ref.status)
    assert np.array_equal(attempts, ref.attempts), (attempts, ref.attempts)
    assert np.array_equal(rx, ref.sig_rx) and np.array_equal(s, ref.sig_s)


@pytest.mark.parametrize("max_attempts", [64, 4096])
def test_seeded_signer_equals_the_first_accepted_attempt(backend, max_attempts):
    messages, secrets = SG.small_batch()
    ref = SG.small_signed(64)
    assert (ref.status == SG.OK).all() and int(ref.attempts.max()) > 1     # some signature needed a second round
    got = backend.schnorr_sign(messages, secrets, seed=SG.SEED, max_attempts=max_attempts)
    _assert_signed(got, ref)
    assert not backend.schnorr_check(messages, got[0], got[1]).any()


def test_a_cap_of_two_exhausts_what_the_reference_names(backend):
    messages, secrets = SG.small_batch()
    ref = SG.small_signed(2)
    exhausted = ref.status == SG.EXHAUSTED
    assert exhausted.any() and not exhausted.all()
    got = backend.schnorr_sign(messages, secrets, seed=SG.SEED, max_attempts=2)
    _assert_signed(got, ref)
    assert not got[0][exhausted].any() and not got[1][exhausted].any() and (got[2][exhausted] == 2).all()


def test_the_largest_key(backend):
    """about 128 attempts per signature: every round runs 128 of them per pending signature"""
    secrets = np.full(3, SG.MAX_SECRET, np.uint64)
    messages = SG.payload_messages(secrets, 0xF1F7)
    ref = SG.Signed(messages, secrets, 0x255, 1024)
    assert (ref.status == SG.OK).all()
    got = backend.schnorr_sign(messages, secrets, seed=0x255, max_attempts=1024)
    _assert_signed(got, ref)
    assert not backend.schnorr_check(messages, got[0], got[1]).any()


def test_another_seed_gives_other_signatures(backend):
    messages, secrets = SG.small_batch()
    a = backend.schnorr_sign(messages[:4], secrets[:4], seed=1, max_attempts=64)
    b = backend.schnorr_sign(messages[:4], secrets[:4], seed=2, max_attempts=64)
    assert not np.array_equal(a[0], b[0])
    assert not backend.schnorr_check(messages[:4], b[0], b[1]).any()


def test_proofs_after_a_signing_call_are_the_proofs_without_it(backend):
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample, get_example_options
    messages, secrets = SG.small_batch()
    backend.upload_witness(LC.generated((2, 3, 2)))
    before = backend.prove(get_example_options())
    backend.schnorr_sign(messages, secrets, seed=SG.SEED, max_attempts=64)
    backend.schnorr_public_keys(secrets)
    assert backend.prove(get_example_options()) == before
    example = SchnorrExample(ProofOptions(), *(a.copy() for a in SC.generated(2, seed=7)), backend=backend)
    before = example.prove()
    backend.schnorr_sign(messages, secrets, seed=SG.SEED, max_attempts=64)
    backend.schnorr_sign_nonces(messages[:3], secrets[:3], SG.nonce_array([0, 1, 2**255]))
    assert example.prove() == before
    example.verify(before)


def test_signing_and_checking_share_a_long_lived_context(backend):
    """the signing calls run in the device block of the signature check, and every context has a table of its own: small and large
    requests of both kinds in turn, on two contexts, give what each gives alone"""
    from certificate_stark_amd.backend import Backend
    messages, secrets = SG.small_batch()
    ref = SG.small_signed(64)
    big_secrets = np.full(3, SG.MAX_SECRET, np.uint64)
    big_messages = SG.payload_messages(big_secrets, 0xF1F7)
    big_ref = SG.Signed(big_messages, big_secrets, 0x255, 1024)
    checked = SC.generated(65)
    other = Backend()
    try:
        for b in (backend, other, backend):
            assert not b.schnorr_check(*SC.generated(5)).any()
            _assert_signed(b.schnorr_sign(messages, secrets, seed=SG.SEED, max_attempts=64), ref)
            assert not b.schnorr_check(*checked).any()                                                   # the block grows under the check
            _assert_signed(b.schnorr_sign(big_messages, big_secrets, seed=0x255, max_attempts=1024), big_ref)   # and under the signer
            assert list(b.schnorr_check(*SC.perturbed(SC.generated(5), 1, "msg26"))) == [0, SC.MISMATCH, 0, 0, 0]
            _assert_signed(b.schnorr_sign(messages, secrets, seed=SG.SEED, max_attempts=64), ref)
            assert np.array_equal(b.schnorr_public_keys(secrets), messages[:, :12])
    finally:
        other.close()


def test_signed_example_proves_and_verifies(backend):
    from certificate_stark_amd.prover import SchnorrExample
    rng = random.Random(8)
    secrets = [1, 2, 3, 4, 5, 6, 7, 200]
    payloads = SC._oracle().to_mont(np.array([[rng.randrange(SC.P) for _ in range(16)] for _ in secrets], np.uint64)).reshape(8, 16)
    example = SchnorrExample.sign(secrets, payloads, seed=3, backend=backend)
    assert np.array_equal(example.messages[:, :12], SG.public_keys(secrets)) and np.array_equal(example.messages[:, 12:], payloads)
    assert not example.check().any()
    ref = SG.Signed(example.messages, secrets, 3, 256)
    assert np.array_equal(example.sig_rx, ref.sig_rx) and np.array_equal(example.sig_s, ref.sig_s)
    proof = example.prove()
    example.verify(proof)
