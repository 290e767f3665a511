"""cstark_schnorr_sign_nonces and cstark_schnorr_public_keys against the reference signer of sign_cases.py, bit for bit in sig_rx, sig_s
and status: one nonce per entry of the fixed-base table (the only place a wrong entry is visible one at a time), the extremes of the
nonce, random nonces that show every status, the counts around the kernels' groupings, the validity of every accepted output under the
existing signature check, the public keys of every secret, and the refusals that launch nothing.  Outputs of the raw calls start as 0xA5
and are compared whole."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import sig_cases as SC
import sign_cases as SG

pytestmark = pytest.mark.gpu

u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
FILL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _assert_reference(backend, messages, secrets, nonces, expected_status=None):
    """nonces: Python integers.  -> (sig_rx, sig_s, status) of the device, equal to the reference's"""
    ref_rx, ref_s, ref_status = SG.attempts(messages, secrets, nonces)
    if expected_status is not None:
        assert list(ref_status) == list(expected_status), "the reference itself disagrees with the case"
    rx, s, status = backend.schnorr_sign_nonces(messages, secrets, SG.nonce_array(nonces))
    assert np.array_equal(status, ref_status), (status, ref_status)
    assert np.array_equal(rx, ref_rx), np.flatnonzero((rx != ref_rx).any(axis=1))
    assert np.array_equal(s, ref_s), np.flatnonzero((s != ref_s).any(axis=1))
    return rx, s, status


def _assert_accepted_are_valid(backend, messages, rx, s, status):
    ok = np.flatnonzero(status == SG.OK)
    if not len(ok):
        return
    verdicts, x = backend.schnorr_check(messages[ok], rx[ok], s[ok], want_rx=True)
    assert not verdicts.any() and np.array_equal(x, rx[ok])


def test_every_table_entry(backend):
    """r = d * 16^w reads exactly one entry, T[w][d]: 990 nonces, one per entry"""
    nonces = [d << (4 * w) for w in range(66) for d in range(1, 16)]
    secrets = np.ones(len(nonces), np.uint64)
    messages = np.repeat(SG.payload_messages([1], 0x7AB1E), len(nonces), axis=0)
    rx, _, _ = _assert_reference(backend, messages, secrets, nonces)
    assert len(set(rx[:, 0].tolist())) == 990


@pytest.mark.parametrize("sk", [1, 255])
def test_extremes(backend, sk):
    nonces = [0, 1, 2**264 - 1, 2**255, 2**256, 2**263]
    secrets = np.full(len(nonces), sk, np.uint64)
    messages = SG.payload_messages(secrets, 0xE87 + sk)
    expected = None
    if sk == 1:     # 1 < h < 2^255 (four limbs below p): 2^255 lies in [h, h + 2^255), 1 below it, 2^256 and more above it
        expected = [SG.INFINITY, SG.NEGATIVE, SG.RANGE, SG.OK, SG.RANGE, SG.RANGE]
    rx, s, status = _assert_reference(backend, messages, secrets, nonces, expected)
    assert status[0] == SG.INFINITY and not rx[0].any()
    assert status[1] == SG.NEGATIVE and np.array_equal(rx[1], np.array(SG.GEN_RAW[:6], np.uint64))
    assert status[2] == SG.RANGE     # 2^264 - 1, every digit 15: above 255 * h + 2^255 too
    if sk == 1:
        verdicts, x = backend.schnorr_check(messages[3:4], rx[3:4], s[3:4], want_rx=True)
        assert list(verdicts) == [SC.VALID] and np.array_equal(x, rx[3:4])
    _assert_accepted_are_valid(backend, messages, rx, s, status)


@functools.lru_cache(maxsize=None)
def _random_case():
    """300 nonces across keys 1..8, drawn as the seeded signer draws them: uniform below (sk + 2) * 2^254"""
    rng = random.Random(0x300)
    secrets = np.array([1 + i % 8 for i in range(300)], np.uint64)
    messages = SG.payload_messages(secrets, 0x3001)
    nonces = tuple(rng.randrange((int(sk) + 2) << 254) for sk in secrets)
    ref = SG.attempts(messages, secrets, nonces)
    for a in (secrets, messages) + ref:
        a.flags.writeable = False
    return messages, secrets, nonces, ref


def test_random_nonces_show_every_status(backend):
    messages, secrets, nonces, ref = _random_case()
    assert set(ref[2].tolist()) == {SG.OK, SG.NEGATIVE, SG.RANGE}
    rx, s, status = _assert_reference(backend, messages, secrets, nonces)
    _assert_accepted_are_valid(backend, messages, rx, s, status)


# 1, 3, 5: partial groups of the hash kernel (four hashes per wave); 64, 257: whole blocks of the scalar kernel and one attempt behind them
@pytest.mark.parametrize("count", [1, 3, 5, 64, 257])
def test_counts(backend, count):
    messages, secrets, nonces, ref = _random_case()
    rx, s, status = backend.schnorr_sign_nonces(messages[:count], secrets[:count], SG.nonce_array(nonces[:count]))
    assert np.array_equal(status, ref[2][:count]) and np.array_equal(rx, ref[0][:count]) and np.array_equal(s, ref[1][:count])


def test_a_message_with_someone_elses_key_is_signed_as_given(backend):
    """the key inside the message is hashed, not compared with sk*G: the signature is one the check calls MISMATCH"""
    rng = random.Random(0x0DD)
    secrets = np.array([3, 5] * 8, np.uint64)
    messages = SG.payload_messages(secrets[::-1], 0x0DD)
    nonces = [rng.randrange((int(sk) + 2) << 254) for sk in secrets]
    rx, s, status = _assert_reference(backend, messages, secrets, nonces)
    ok = np.flatnonzero(status == SG.OK)
    assert len(ok) >= 2 and (backend.schnorr_check(messages[ok], rx[ok], s[ok]) == SC.MISMATCH).all()


def test_public_keys(backend):
    secrets = np.arange(1, 256, dtype=np.uint64)
    keys = backend.schnorr_public_keys(secrets)
    assert keys.shape == (255, 12) and np.array_equal(keys, SG.public_keys(secrets))
    assert all(SG.on_curve(k) for k in keys)
    assert np.array_equal(keys[0], np.array(SG.GEN_RAW, np.uint64))
    from certificate_stark_amd.prover import public_keys
    assert np.array_equal(public_keys([7, 7, 200], backend=backend), keys[[6, 6, 199]])


def _raw(backend, name, count, inputs, outputs, null=None):
    """the C call `name` on 0xA5-filled outputs -> (status, outputs)"""
    outs = [np.full(shape, FILL if dtype == np.uint64 else 0xA5A5A5A5 if dtype == np.uint32 else 0xA5, dtype) for shape, dtype in outputs]
    args = [a if isinstance(a, (C.c_uint64, C.c_uint32)) else a.ctypes.data_as(u8p if a.dtype == np.uint8 else u64p) for a in inputs]
    args += [a.ctypes.data_as(u8p if a.dtype == np.uint8 else C.POINTER(C.c_uint32) if a.dtype == np.uint32 else u64p) for a in outs]
    if null is not None:
        args[null] = None
    rc = getattr(backend.lib, name)(backend.ctx, C.c_uint32(count), *args)
    return rc, outs


def test_refusals_launch_nothing_and_leave_the_outputs(backend):
    n = 5
    secrets = np.array([1, 2, 3, 4, 255], np.uint64)
    messages = SG.payload_messages(secrets, 0xBAD)
    nonces = SG.nonce_array([2**255 + i for i in range(n)])
    shapes = {"keys": ((n, 12), np.uint64), "rx": ((n, 6), np.uint64), "s": ((n, 32), np.uint8), "status": ((n,), np.uint8),
              "attempts": ((n,), np.uint32)}

    def refused(name, inputs, outputs, count=n, null=None):
        rc, outs = _raw(backend, name, count, inputs, [shapes[o] for o in outputs], null)
        assert rc == -1, (name, rc)
        for o in outs:
            assert (o == (FILL if o.dtype == np.uint64 else 0xA5A5A5A5 if o.dtype == np.uint32 else 0xA5)).all(), name
        return backend.lib.cstark_last_error().decode()

    def each_call(messages=messages, secrets=secrets, nonces=nonces, count=n, max_attempts=64, only=None):
        calls = {"cstark_schnorr_public_keys": ([secrets], ["keys"]),
                 "cstark_schnorr_sign_nonces": ([messages, secrets, nonces], ["rx", "s", "status"]),
                 "cstark_schnorr_sign": ([messages, secrets, C.c_uint64(7), C.c_uint32(max_attempts)], ["rx", "s", "attempts", "status"])}
        return [refused(name, ins, outs, count) for name, (ins, outs) in calls.items() if only is None or name in only]

    each_call(count=0)
    each_call(count=(1 << 20) + 1)
    # a null pointer, every argument of every call (attempts_out, which may be null, apart)
    for null in (0, 1):
        refused("cstark_schnorr_public_keys", [secrets], ["keys"], null=null)
    for null in range(6):
        refused("cstark_schnorr_sign_nonces", [messages, secrets, nonces], ["rx", "s", "status"], null=null)
    for null in (0, 1, 4, 5, 7):
        refused("cstark_schnorr_sign", [messages, secrets, C.c_uint64(7), C.c_uint32(64)], ["rx", "s", "attempts", "status"], null=null)
    for bad_secret in (0, 256, 2**64 - 1):
        bad = secrets.copy()
        bad[3] = bad_secret
        bad[4] = 0
        assert all("secrets[3]" in text for text in each_call(secrets=bad))
    bad = nonces.copy()
    bad[2, 4] = 0x100
    bad[4, 4] = 2**63
    assert "nonces[2]" in each_call(nonces=bad, only=["cstark_schnorr_sign_nonces"])[0]
    bad = messages.copy()
    bad[1, 27] = SC.P
    bad[3, 0] = 2**64 - 1
    assert all("messages[1][27]" in text for text in each_call(messages=bad, only=["cstark_schnorr_sign_nonces", "cstark_schnorr_sign"]))
    for max_attempts in (0, 4097):
        assert "max_attempts" in each_call(max_attempts=max_attempts, only=["cstark_schnorr_sign"])[0]
    # the largest legal values are no refusal: a nonce of 2^264 - 1, a null attempts_out
    edge = nonces.copy()
    edge[0] = SG.limbs(2**264 - 1)
    rc, _ = _raw(backend, "cstark_schnorr_sign_nonces", n, [messages, secrets, edge], [shapes[o] for o in ("rx", "s", "status")])
    assert rc == 0, backend.lib.cstark_last_error()
    rc, outs = _raw(backend, "cstark_schnorr_sign", 4, [messages, secrets, C.c_uint64(7), C.c_uint32(64)],
                    [shapes[o] for o in ("rx", "s", "attempts", "status")], null=6)
    assert rc == 0 and not outs[3][:4].any() and (outs[2] == 0xA5A5A5A5).all()


def test_python_layer_refuses_ragged_arrays(backend):
    messages, secrets, nonces, _ = _random_case()
    with pytest.raises(ValueError):
        backend.schnorr_sign_nonces(messages[:4], secrets[:3], SG.nonce_array(nonces[:4]))
    with pytest.raises(ValueError):
        backend.schnorr_sign_nonces(messages[:4], secrets[:4], SG.nonce_array(nonces[:3]))
    from certificate_stark_amd import CstarkError
    with pytest.raises(CstarkError):
        backend.schnorr_public_keys([0])
