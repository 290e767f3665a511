"""The reference signer of sign_cases.py, pinned on the CPU before any GPU run: its accepted signatures are VALID under the oracle's
SchnorrAir trace (sig_cases.reference, which shares nothing with the signer) and its rejected attempts are not; the caps the GPU tests
rely on hold for their seed; the built library exports the new entry points; and csrc/sign_plan.h -- the nonce stream, the round schedule
and the first-accepted selection -- equals a plain scan of the attempts in order (tests/cpp/sign_plan_check.cpp, a stand-alone program
built with AddressSanitizer and UBSan and run directly)."""
import os
import subprocess

import numpy as np
import pytest

import sig_cases as SC
import sign_cases as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_pinned(signed, messages):
    """every accepted signature is VALID; no rejected attempt is (a rejected attempt with 0 <= s < 2^255 would have been accepted)"""
    ok = np.flatnonzero(signed.status == SG.OK)
    verdicts, x = SC.reference(messages[ok], signed.sig_rx[ok], signed.sig_s[ok])
    assert (verdicts == SC.VALID).all() and np.array_equal(x, signed.sig_rx[ok])
    if signed.rejected:
        t = [r[0] for r in signed.rejected]
        verdicts, _ = SC.reference(messages[t], np.array([r[1] for r in signed.rejected]), np.array([r[2] for r in signed.rejected]))
        assert (verdicts != SC.VALID).all()
        assert all(r[3] in (SG.NEGATIVE, SG.RANGE) for r in signed.rejected)


def test_accepted_signatures_are_valid_and_rejected_attempts_are_not():
    messages, secrets = SG.small_batch()
    signed = SG.small_signed(64)
    assert sorted(set(int(k) for k in secrets)) == list(range(1, 9))
    _assert_pinned(signed, messages)
    statuses = set(r[3] for r in signed.rejected)
    assert statuses == {SG.NEGATIVE, SG.RANGE}, "the batch's rejected attempts show both ways to miss the window"


def test_the_largest_key_signs_too():
    secrets = np.full(4, SG.MAX_SECRET, np.uint64)
    messages = SG.payload_messages(secrets, 0xF1F7)
    signed = SG.Signed(messages, secrets, 0x255, 1024)
    assert (signed.status == SG.OK).all() and signed.total_attempts > 40   # about 128 attempts each are expected
    _assert_pinned(signed, messages)


def test_one_attempt_defines_every_output():
    """r = 0 is INFINITY with a zero R.x; r = 1 is R = G; the scalar is the low 256 bits of r - sk*h whatever the status"""
    messages, secrets = SG.small_batch()
    rx, s, status = SG.attempt(messages[0], secrets[0], 0)
    assert status == SG.INFINITY and not rx.any()
    h0 = SG.hash_to_int(np.zeros(6, np.uint64), messages[0])
    assert int.from_bytes(s.tobytes(), "little") == (-int(secrets[0]) * h0) % 2**256
    rx, s, status = SG.attempt(messages[0], secrets[0], 1)
    assert status == SG.NEGATIVE and np.array_equal(rx, np.array(SG.GEN_RAW[:6], np.uint64))
    assert all(SG.on_curve(k) for k in SG.public_keys([1, 2, 255]))


def test_caps_of_the_gpu_tests():
    """with the GPU tests' seed, 64 attempts exhaust no signature of the small batch, 2 attempts exhaust some and not all"""
    full, capped = SG.small_signed(64), SG.small_signed(2)
    assert (full.status == SG.OK).all() and int(full.attempts.max()) <= 64
    exhausted = capped.status == SG.EXHAUSTED
    assert exhausted.any() and not exhausted.all()
    assert np.array_equal(exhausted, full.attempts > 2)
    assert np.array_equal(capped.sig_rx[~exhausted], full.sig_rx[~exhausted]) and not capped.sig_rx[exhausted].any()
    assert (capped.attempts[exhausted] == 2).all()


def test_the_library_exports_the_signing_entry_points():
    from certificate_stark_amd import _lib
    lib = _lib.load()
    for name in ("cstark_schnorr_public_keys", "cstark_schnorr_sign_nonces", "cstark_schnorr_sign", "cstark_ledger_messages", "cstark_ledger_sign"):
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def plan_checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sign_plan") / "sign_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "sign_plan_check.cpp")])
    return exe


def test_rounds_and_selection_equal_a_scan_in_order(plan_checker):
    out = subprocess.run([plan_checker], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "ok: round sizes 0 1 3 64" in out.stdout, out.stdout


def test_the_stream_of_sign_plan_is_the_reference_stream(plan_checker):
    """the program prints the first nonces of a few signatures; the Python restatement gives the same"""
    out = subprocess.run([plan_checker, "nonces"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("nonce ")]
    assert len(lines) >= 12
    for _, seed, t, sk, a, value in lines:
        stream = SG.nonce_stream(int(seed, 16), int(t), int(sk))
        for _ in range(int(a)):
            next(stream)
        assert next(stream) == int(value, 16), (seed, t, sk, a)
