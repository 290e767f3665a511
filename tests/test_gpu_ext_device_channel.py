"""GPU: quadratic and cubic proofs on the device-side Fiat-Shamir channel (csrc/channel.hip, prove_core_dev in csrc/prove.hip).

With the Blake3 coin and no proof of work, extension-field proofs are enqueued whole and waited for once, like base-field proofs: the
channel draws m-word elements on the device, and the out-of-domain frame, the DEEP stage and the FRI folds read them there.  The bytes
stay those of the host channel and of the CPU prover (oracle/prover.py); Backend.prove_channel() tells which channel a proof took.

The sizes are the smallest at which each piece can go wrong: a cubic TransactionAir proof draws 3 * 2 * (115 + 4) = 714 coefficient
words (two passes of the channel's draw loop and more), its frame absorbs 2 * 3 * 94 = 564 words (five Blake3 chunks: the chunk tree),
and folding factors 4, 8 and 16 each have at least one FRI layer on the 2^14-point domain of two transfers."""
import hashlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (transfers, Merkle depth, options); options = (queries, blowup, grinding, hash, extension, folding, max remainder)
TX_CASES = []
for _ext in (1, 2):
    TX_CASES += [(1, 3, (42, 8, 0, 0, _ext, 4, 256)),     # 2^10 rows: the smallest trace
                 (2, 3, (42, 8, 0, 0, _ext, 4, 256)),
                 (2, 3, (20, 8, 0, 0, _ext, 8, 128)),
                 # (the issue's (20, 16, 0, 0, ext, 16, 64) is refused by oracle/prover.py -- fri_max_remainder must be 128 .. 1024 -- and by
                 # the library: dropped.  Folding factor 16 is kept in the suite by the same options at the smallest remainder both accept.)
                 (2, 3, (20, 16, 0, 0, _ext, 16, 128)),
                 (2, 3, (28, 8, 0, 0, _ext, 4, 1024))]
TX_CASES.append((8, 15, (96, 8, 0, 0, 2, 4, 256)))
SUB_AIR_OPTS = (42, 8, 0, 0, None, 4, 256)  # the options of test_gpu_prove_small_airs.py::test_sub_air_proofs_over_extension_fields

_witnesses, _references = {}, {}


def witness(n_tx, depth):
    from oracle import oracle as O
    key = (n_tx, depth)
    if key not in _witnesses:
        _witnesses[key] = O.TxWitness.generate(n_tx, depth, seed=900 + n_tx)
    return _witnesses[key]


def reference(n_tx, depth, opts):
    """the CPU prover's proof of witness(n_tx, depth): computed once, shared by the tests below, never changed"""
    from oracle import prover as OP
    key = (n_tx, depth, tuple(opts))
    if key not in _references:
        _references[key] = OP.prove(witness(n_tx, depth), tuple(opts))
    return _references[key]


def metadata(w):
    from certificate_stark_amd.prover import TransactionMetadata
    return TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS])


def options(opts):
    from certificate_stark_amd.prover import ProofOptions
    return ProofOptions(*opts)


@pytest.fixture(scope="module")
def backend(oracle):
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.mark.parametrize("ext", [1, 2])
def test_extension_proofs_take_the_device_channel(oracle, ext):
    """The test that fails without the feature: quadratic and cubic Blake3 proofs without proof of work report the device channel;
    the Sha3 coin and proof of work keep the host channel; a base-field Blake3 proof is on the device as before."""
    from certificate_stark_amd import CstarkError
    from certificate_stark_amd.backend import Backend
    b = Backend()
    try:
        with pytest.raises(CstarkError):   # no proof has been generated on this context
            b.prove_channel()
        b.upload_witness(metadata(witness(2, 3)))
        b.prove(options((42, 8, 0, 0, ext, 4, 256)))
        assert b.prove_channel() == "device"
        b.prove(options((42, 8, 0, 1, ext, 4, 256)))
        assert b.prove_channel() == "host"
        b.prove(options((42, 8, 8, 0, ext, 4, 256)))
        assert b.prove_channel() == "host"
        b.prove(options((42, 8, 0, 0, 0, 4, 256)))
        assert b.prove_channel() == "device"
    finally:
        b.close()


@pytest.mark.parametrize("n_tx,depth,opts", TX_CASES)
def test_device_channel_proof_bytes_equal_the_cpu_prover(oracle, backend, n_tx, depth, opts):
    from oracle import verifier as V
    w = witness(n_tx, depth)
    backend.upload_witness(metadata(w))
    proof = backend.prove(options(opts))
    assert backend.prove_channel() == "device"
    ref = reference(n_tx, depth, opts)
    assert len(proof) == len(ref)
    assert proof == ref
    assert V.verify(proof, w.initial_roots[0], w.final_root, options=list(opts))


@pytest.mark.parametrize("ext", [1, 2])
def test_sub_air_proofs_on_the_device_channel(oracle, backend, ext):
    """MerkleAir, SchnorrAir, RangeProofAir and RescueAir: one coefficient block per component, one merge per block.  A 64-row range
    proof at the reference tests' blowup 4 has no FRI layer (256 points, remainder 256) and stays on the host channel."""
    from oracle import prover as OP
    from oracle import verifier as V
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import MerkleExample, RangeProofExample, RescueExample, SchnorrExample
    opts = tuple(ext if v is None else v for v in SUB_AIR_OPTS)
    po = options(opts)

    w = witness(2, 3)
    mex = MerkleExample(po, metadata(w), backend)
    proof = mex.prove()
    assert backend.prove_channel() == "device"
    assert proof == OP.prove_air(oracle.AIR_MERKLE, w, opts)
    assert V.verify_merkle(proof, *mex.pub_inputs(), options=list(opts))

    sex = SchnorrExample.build_random(po, 1, seed=80 + ext, backend=backend)
    proof = sex.prove()
    assert backend.prove_channel() == "device"
    sw = oracle.SchnorrWitness(1)
    sw.messages[...], sw.sig_rx[...], sw.sig_s[...] = sex.messages, sex.sig_rx, sex.sig_s
    assert proof == OP.prove_air(oracle.AIR_SCHNORR, sw, opts)
    assert V.verify_schnorr(proof, sw, options=list(opts))

    number = int(oracle.to_mont([42])[0])
    proof = RangeProofExample(po, number, backend).prove()
    assert backend.prove_channel() == "device"
    assert proof == OP.prove_air(oracle.AIR_RANGE, number, opts)
    assert V.verify_range(proof, number, options=list(opts))
    no_layer = (42, 4, 0, 0, ext, 4, 256)     # build_options of src/range/tests.rs:87-98
    proof = RangeProofExample(options(no_layer), number, backend).prove()
    assert backend.prove_channel() == "host"
    assert proof == OP.prove_air(oracle.AIR_RANGE, number, no_layer)
    assert V.verify_range(proof, number, options=list(no_layer))

    rex = RescueExample(8, po, backend)       # the shortest chain of test_gpu_rescue_chain.py: 64 rows
    proof = rex.prove()
    assert backend.prove_channel() == "device"
    assert proof == OP.prove_air(oracle.AIR_RESCUE_CHAIN, (rex.seed, 8), opts)
    result = oracle.rescue_chain_build_trace(rex.seed, 8)[:7, -1].copy()
    assert V.verify_rescue(proof, rex.seed, result, options=list(opts))


def _channel_digests():
    """the channel of, then the sha256 of, the extension-field proofs of TX_CASES at two transfers, on a fresh backend: printed by the
    child process of the test below, computed in-process by the test itself"""
    from certificate_stark_amd.backend import Backend
    b = Backend()
    out = []
    try:
        b.upload_witness(metadata(witness(2, 3)))
        for n_tx, depth, opts in TX_CASES:
            if n_tx == 2:
                proof = b.prove(options(opts))
                out.append(b.prove_channel() + ":" + hashlib.sha256(proof).hexdigest())
    finally:
        b.close()
    return out


def test_host_and_device_channel_give_the_same_extension_proofs(oracle):
    """CSTARK_HOST_CHANNEL=1 -- read once per process -- keeps the host channel for the same proofs: same bytes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_gpu_ext_device_channel import _channel_digests\n"
            "print(' '.join(_channel_digests()))\n") % (root, os.path.join(root, "tests"))
    got = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CSTARK_HOST_CHANNEL="1"), capture_output=True, text=True, timeout=600)
    assert got.returncode == 0, got.stderr[-2000:]
    child = [v.split(":") for v in got.stdout.strip().splitlines()[-1].split()]
    mine = [v.split(":") for v in _channel_digests()]
    assert len(mine) == 8 and len(child) == len(mine)
    assert all(ch == "host" for ch, _ in child) and all(ch == "device" for ch, _ in mine)
    assert [d for _, d in child] == [d for _, d in mine]


def test_one_context_alternating_between_the_channels(oracle, backend):
    """cubic (device), Sha3 cubic (host), quadratic (device), base field (device), cubic again on ONE context: the two channels share the
    arena's per-proof buffers, and every proof must still equal the CPU prover's and leave all stage times behind."""
    w = witness(2, 3)
    backend.upload_witness(metadata(w))
    cubic = (42, 8, 0, 0, 2, 4, 256)
    proofs = []
    for opts, channel in ((cubic, "device"), ((42, 8, 0, 1, 2, 4, 256), "host"), ((42, 8, 0, 0, 1, 4, 256), "device"),
                          ((42, 8, 0, 0, 0, 4, 256), "device"), (cubic, "device")):
        proof = backend.prove(options(opts))
        assert backend.prove_channel() == channel, opts
        assert proof == reference(2, 3, opts), opts
        stages = backend.prove_stage_ms()
        assert set(stages) == set(backend.PROVE_STAGES) and all(v >= 0 and math.isfinite(v) for v in stages.values()), (opts, stages)
        proofs.append(proof)
    assert proofs[0] == proofs[-1]


def test_gpu_verifier_accepts_a_cubic_device_channel_proof(oracle):
    from certificate_stark_amd.prover import TransactionExample
    from certificate_stark_amd.verify import VerifierError
    w = witness(2, 3)
    tx = TransactionExample(options((42, 8, 0, 0, 2, 4, 256)), metadata(w))
    try:
        proof = tx.prove()
        assert tx.prover.backend.prove_channel() == "device"
        tx.verify(proof)                       # raises VerifierError on rejection
        bad = bytearray(proof)
        bad[len(bad) - 40] ^= 2                # (and is not vacuous: a flipped remainder bit is rejected)
        with pytest.raises(VerifierError):
            tx.verify(bytes(bad))
    finally:
        tx.prover.backend.close()
