"""cstark_air_validate_trace on the GPU against the CPU reference of validate_cases.py: clean traces, single-cell corruptions (step,
constraint, bad cycles, every cycle code and all frame values bit for bit), one frame on which two contributions to a slot cancel,
the boundary lists, validate() on steered witnesses, isolation from the prover and misuse.  Device traces are oracle-built numpy
traces uploaded with from_numpy_u64 unless the test is about validate() itself."""
import ctypes as C

import numpy as np
import pytest

import validate_cases as VC

pytestmark = pytest.mark.gpu
P = VC.P
OPTS = (8, 8, 0, 0, 0, 4, 128)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def seed(oracle):
    return oracle.to_mont(np.arange(42, 49, dtype=np.uint64))


@pytest.fixture(scope="module")
def tx2(oracle, witness_d3):
    return oracle.tx_build_trace(witness_d3)


@pytest.fixture(scope="module")
def schnorr2(oracle, backend):
    w = oracle.SchnorrWitness.generate(2, seed=9)
    return w, oracle.schnorr_build_trace(w)


def pub_of(w):
    return np.concatenate([w.initial_roots[0], w.final_root])


def run(backend, air, trace, depth=0, public=None):
    return backend.air_validate_trace(air, backend.from_numpy_u64(trace), depth, public, want_cycles=True, want_frame=True)


def assert_matches(rep, ref, boundary=None):
    """the report against the reference, bit for bit"""
    assert rep.step == ref.step and rep.constraint == ref.constraint and rep.bad_cycles == ref.bad_cycles
    assert np.array_equal(rep.cycle_codes, ref.codes)
    if ref.step is None:
        assert rep.frame_values is None
    else:
        assert np.array_equal(rep.frame_values, ref.frame_values)
    assert (rep.boundary, rep.boundary_register, rep.boundary_step) == (boundary or (None, None, None))
    assert rep.ok == (ref.step is None and boundary is None)


def assert_clean(rep, n_cycles):
    assert rep.ok and rep.step is None and rep.bad_cycles == 0 and rep.boundary is None and str(rep) == "clean"
    assert rep.cycle_codes.shape == (n_cycles,) and (rep.cycle_codes == VC.CLEAN).all()


# ---- 1. clean traces -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tx,depth", [(1, 3), (2, 3), (4, 7), (2, 15), (64, 15)])
def test_clean_transaction_traces(oracle, backend, n_tx, depth):
    w = oracle.TxWitness.generate(n_tx, depth, seed=0x5EED)
    assert_clean(run(backend, VC.TX, oracle.tx_build_trace(w), depth, pub_of(w)), n_tx)


@pytest.mark.parametrize("depth", [3, 15])
def test_clean_merkle_traces(oracle, backend, depth):
    w = oracle.TxWitness.generate(2, depth, seed=0x5EED)
    assert_clean(run(backend, VC.MERKLE, oracle.merkle_build_trace(w), depth, pub_of(w)), 2)


@pytest.mark.parametrize("n_sig", [1, 2, 4])
def test_clean_schnorr_traces(oracle, backend, n_sig):
    w = oracle.SchnorrWitness.generate(n_sig, seed=9)
    backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s)
    assert_clean(run(backend, VC.SCHNORR, oracle.schnorr_build_trace(w), 0, True), n_sig)


@pytest.mark.parametrize("number", [0, 1, P - 1])
def test_clean_range_traces(oracle, backend, number):
    assert_clean(run(backend, VC.RANGE, oracle.range_build_trace(number), 0, oracle.to_mont([number])), 1)


@pytest.mark.parametrize("chain", [2, 8, 16])
def test_clean_rescue_traces(oracle, backend, seed, chain):
    t = oracle.rescue_chain_build_trace(seed, chain)        # chain 2: 16 rows, less than one wave
    assert_clean(run(backend, VC.RESCUE, t, 0, np.concatenate([seed, t[:7, -1]])), chain)


# the lowest violated slot of the cells that are there for a particular slot: slot 0, the highest slot any cell can violate (R_KEY_RES + 11),
# PREV_ROOT under finish and under not_finish
TX_NAMED_SLOTS = {"slot-0": 0, "top-slot": 114, "prev-root-finish": 58, "prev-root-not-finish": 58}
# ... and of the sub-AIR cells on a slot with more than one contribution: MerkleAir's PREV_ROOT, RescueAir's slot 0 (round and copy)
SUB_NAMED_SLOTS = {(1, "two-contributions"): 58, (4, "two-contributions"): 0}


# ---- 2. single-cell corruption -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(VC.TX_CELLS))
def test_one_corrupted_transaction_cell(oracle, backend, tx2, name):
    bad = VC.bump(tx2, [VC.TX_CELLS[name]])
    ref = VC.reference(oracle, VC.TX, bad, 3, clean_trace=tx2)
    rep = run(backend, VC.TX, bad, 3)
    print(name, VC.TX_CELLS[name], "->", rep, "| reference step", ref.step, "constraint", ref.constraint)
    assert ref.step is not None
    if name in TX_NAMED_SLOTS:                             # the cases named for the slot they violate keep violating it
        assert ref.constraint == TX_NAMED_SLOTS[name]
    assert_matches(rep, ref)
    assert str(rep) == "transfer %d, row %d, constraint %d" % (ref.step // 1024, ref.step % 1024, ref.constraint)


def test_two_corrupted_transfers_are_two_bad_cycles(oracle, backend, tx2):
    bad = VC.bump(tx2, [(60, 100), (70, 1500)])
    ref = VC.reference(oracle, VC.TX, bad, 3, clean_trace=tx2)
    assert ref.bad_cycles == 2
    assert_matches(run(backend, VC.TX, bad, 3), ref)


# per sub-AIR: first row, last row, cycle boundary, a slot with more than one contribution
SUB_CELLS = {
    VC.MERKLE: {"first-row": (60, 0), "last-row": (60, 1023), "cycle-boundary": (60, 512), "two-contributions": (58, 31), "wave-boundary": (61, 64)},
    VC.RESCUE: {"first-row": (3, 0), "last-row": (3, 127), "cycle-boundary": (3, 8), "two-contributions": (2, 7), "wave-boundary": (9, 64)},
    VC.RANGE: {"first-row": (1, 0), "last-row": (1, 63), "bit": (0, 7), "accumulator": (1, 30)},
}


@pytest.mark.parametrize("air,name", [(a, k) for a in SUB_CELLS for k in sorted(SUB_CELLS[a])])
def test_one_corrupted_sub_air_cell(oracle, backend, witness_d3, seed, air, name):
    trace = {VC.MERKLE: lambda: oracle.merkle_build_trace(witness_d3), VC.RESCUE: lambda: oracle.rescue_chain_build_trace(seed, 16),
             VC.RANGE: lambda: oracle.range_build_trace(0x123456789ABCDEF)}[air]()
    bad = VC.bump(trace, [SUB_CELLS[air][name]])
    ref = VC.reference(oracle, air, bad, 3)
    rep = run(backend, air, bad, 3)
    print(air, name, SUB_CELLS[air][name], "->", rep)
    assert ref.step is not None
    if (air, name) in SUB_NAMED_SLOTS:
        assert ref.constraint == SUB_NAMED_SLOTS[(air, name)]
    assert_matches(rep, ref)


# SchnorrAir: row 510 of a block is where parts 0 / 1 (the last ladder step) hand over to part 3 (the final addition at row 510 -> 511)
@pytest.mark.parametrize("name,cell", [("first-row", (3, 0)), ("last-row", (3, 1023)), ("cycle-boundary", (3, 512)), ("parts-0-and-3", (7, 510)),
                                       ("final-addition", (7, 511)), ("hash", (45, 20)), ("limbs", (40, 600))])
def test_one_corrupted_schnorr_cell(oracle, backend, schnorr2, name, cell):
    w, trace = schnorr2
    backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s)
    bad = VC.bump(trace, [cell])
    ref = VC.reference(oracle, VC.SCHNORR, bad, statement=w)
    rep = run(backend, VC.SCHNORR, bad)
    print(name, cell, "->", rep)
    assert ref.step is not None
    assert_matches(rep, ref)


# ---- 3. cancellation -----------------------------------------------------------------------------------------------------------
def _sqrt_mod_p(a):
    """Tonelli-Shanks; None if a is no square"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 2, P) != 1:
        return None
    q, s = P - 1, 0
    while q % 2 == 0:
        q //= 2; s += 1
    z = 2
    while pow(z, (P - 1) // 2, P) == 1:
        z += 1
    m, c, t, r = s, pow(z, q, P), pow(a, q, P), pow(a, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % P; i += 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    return r


def test_contributions_that_cancel_are_not_reported(oracle, backend, tx2):
    """Row 0 of a transfer is a row of the trace domain where two flags of one slot are both set and weigh DIFFERENT values: slot 14
    takes setup * (first row of the S_UPD round gadget) and tx_hash * is_binary(next[14]).  On frame 1024 (row 0 of transfer 1) the
    round contribution is made D != 0 by changing next[S_UPD]; the bit next[14] is then set to a root of b^2 - b = -D, so both
    contributions are non-zero and the slot's sum is 0.  Slot 15 (the same gadget row under hash_flag) is violated, so the frame's
    lowest violated slot is 15: an evaluator that decides from single contributions says 14."""
    r, per = 1024, np.ascontiguousarray(oracle.tx_periodic_columns(3)[:, 0])
    rows = np.ascontiguousarray(tx2.T)
    for delta in range(1, 64):
        bad = tx2.copy()
        bad[15, r + 1] = np.uint64((int(bad[15, r + 1]) + delta * VC.one()) % P)
        ev = oracle.tx_evaluate_transition(rows[r], np.ascontiguousarray(bad[:, r + 1]), per)
        d = int(oracle.from_mont(ev[14:15])[0])            # the round contribution alone: the bit is still binary
        root = _sqrt_mod_p(1 - 4 * d)                      # b^2 - b + D = 0
        if d and root is not None:
            break
    else:
        pytest.fail("no delta gives a solvable bit")
    bit = (1 + root) * pow(2, P - 2, P) % P
    assert (bit * bit - bit + d) % P == 0 and bit not in (0, 1)
    bad[14, r + 1] = oracle.to_mont([bit])[0]
    only_bit = tx2.copy(); only_bit[14, r + 1] = bad[14, r + 1]
    ev_bit = oracle.tx_evaluate_transition(rows[r], np.ascontiguousarray(only_bit[:, r + 1]), per)
    ev_both = oracle.tx_evaluate_transition(rows[r], np.ascontiguousarray(bad[:, r + 1]), per)
    assert ev[14] != 0 and ev_bit[14] != 0 and ev_both[14] == 0 and ev_both[15] != 0      # each contribution alone, then their sum
    ref = VC.reference(oracle, VC.TX, bad, 3, clean_trace=tx2)
    assert ref.codes[1] == 0 * 115 + 15 and ref.codes[0] == VC.CLEAN
    rep = run(backend, VC.TX, bad, 3)
    assert_matches(rep, ref)
    assert rep.frame_values[14] == 0 and rep.constraint == 15 and rep.step == 1024


# ---- 4. boundary ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("air", [VC.TX, VC.MERKLE, VC.RESCUE])
def test_each_altered_public_word_is_named(oracle, backend, witness_d3, tx2, seed, air):
    if air == VC.RESCUE:
        trace = oracle.rescue_chain_build_trace(seed, 8)
        pub = np.concatenate([seed, trace[:7, -1]])
    else:
        trace = tx2 if air == VC.TX else oracle.merkle_build_trace(witness_d3)
        pub = pub_of(witness_d3)
    n = trace.shape[1]
    d_trace = backend.from_numpy_u64(trace)
    for k in range(14):
        p = VC.bump(pub.reshape(1, 14), [(0, k)])[0]
        rep = backend.air_validate_trace(air, d_trace, 3, p)
        want = VC.boundary_reference(oracle, air, trace, p)
        assert want == (k, (0 if air == VC.RESCUE else 58) + k % 7, 0 if k < 7 else n - 1)
        assert (rep.boundary, rep.boundary_register, rep.boundary_step) == want and rep.step is None and not rep.ok
        assert str(rep) == "boundary entry %d: register %d at step %d" % want
    assert backend.air_validate_trace(air, d_trace, 3, None).boundary is None


def test_wrong_range_number_is_entry_1(oracle, backend):
    trace = oracle.range_build_trace(77)
    rep = run(backend, VC.RANGE, trace, 0, oracle.to_mont([78]))
    assert (rep.boundary, rep.boundary_register, rep.boundary_step) == (1, 1, 63) and rep.step is None
    bad0 = VC.bump(trace, [(1, 0)])
    rep = run(backend, VC.RANGE, bad0, 0, oracle.to_mont([77]))
    assert (rep.boundary, rep.boundary_register, rep.boundary_step) == (0, 1, 0) and rep.step == 0


def test_altered_signature_word_is_the_sequence_entry_of_its_block(oracle, backend, schnorr2):
    w, trace = schnorr2
    rx = VC.bump(w.sig_rx, [(1, 2)])
    backend.upload_schnorr_witness(w.messages, rx, w.sig_s)
    stated = oracle.SchnorrWitness(2)
    stated.messages[...] = w.messages; stated.sig_rx[...] = rx; stated.sig_s[...] = w.sig_s
    want = VC.boundary_reference(oracle, VC.SCHNORR, trace, statement=stated)
    assert want == (42 + 2, 42 + 2, 512)                 # the step-0 sequence of R.x word 2, at the first row of block 1
    rep = run(backend, VC.SCHNORR, trace, 0, True)
    assert (rep.boundary, rep.boundary_register, rep.boundary_step) == want and rep.step is None
    rep = run(backend, VC.SCHNORR, trace, 0, None)       # no boundary check: whatever the trace holds
    assert rep.boundary is None and rep.ok
    backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s)
    assert run(backend, VC.SCHNORR, VC.bump(trace, [(30, 512)]), 0, None).boundary is None


# ---- 5. witness level ----------------------------------------------------------------------------------------------------------
def _steered(oracle, what):
    w = oracle.TxWitness.generate(2, 3, seed=0x5EED)
    if what == "sibling":
        w.s_paths[1, 2, 0] ^= np.uint64(1)
    elif what == "initial-root-1":
        w.initial_roots[1, 0] ^= np.uint64(1)
    elif what == "delta-above-balance":
        w.deltas[1] = oracle.to_mont([(1 << 62) + 12345])[0]
    elif what == "final-root":
        w.final_root[0] ^= np.uint64(1)
    elif what == "sig-s":
        w.sig_s[1, 3] ^= np.uint8(4)
    return w


@pytest.mark.parametrize("what", ["honest", "sibling", "initial-root-1", "delta-above-balance", "final-root", "sig-s"])
def test_validate_agrees_with_prove_and_verify(oracle, backend, what):
    from certificate_stark_amd.backend import to_numpy_u64
    from certificate_stark_amd.prover import ProofOptions, TransactionExample
    from certificate_stark_amd.verify import VerifierError
    w = _steered(oracle, what)
    ex = TransactionExample(ProofOptions(*OPTS), w, backend)
    rep = ex.validate()
    try:
        ex.verify(ex.prove())
        accepted = True
    except VerifierError:
        accepted = False
    trace = to_numpy_u64(ex.prover.build_trace(w))
    code = oracle.tx_check_trace(trace, 2, 3)
    print(what, "->", rep, "| accepted", accepted, "| tx_check_trace", code)
    assert rep.ok == accepted
    assert rep.ok == (what in ("honest", "sig-s"))          # TransactionAir does not bind the signature: the known quirk
    assert (rep.step, rep.constraint) == ((None, None) if code < 0 else (code // 115, code % 115))
    assert VC.boundary_reference(oracle, VC.TX, trace, pub_of(w)) == (None if rep.boundary is None else (rep.boundary, rep.boundary_register, rep.boundary_step))


def test_schnorr_example_names_the_forged_signature(oracle, backend):
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample
    from certificate_stark_amd.verify import VerifierError
    w = oracle.SchnorrWitness.generate(2, seed=9)
    good = SchnorrExample(ProofOptions(*OPTS), w.messages.copy(), w.sig_rx.copy(), w.sig_s.copy(), backend)
    assert good.validate().ok
    good.verify(good.prove())
    s = w.sig_s.copy(); s[1, 3] ^= np.uint8(4)
    forged = SchnorrExample(ProofOptions(*OPTS), w.messages.copy(), w.sig_rx.copy(), s, backend)
    rep = forged.validate()
    print("forged signature 1 ->", rep)
    assert not rep.ok and rep.step is None and rep.boundary >= 55 and rep.boundary_step == 1023 and rep.boundary_register == rep.boundary - 55
    with pytest.raises(VerifierError):
        forged.verify(forged.prove())


# ---- 6. isolation --------------------------------------------------------------------------------------------------------------
def test_a_proof_after_a_validation_is_the_proof_without_it(oracle, backend, witness_d3, tx2):
    from certificate_stark_amd.prover import ProofOptions, SchnorrExample
    backend.upload_witness(witness_d3)
    before = backend.prove(ProofOptions(*OPTS))
    rep = run(backend, VC.TX, VC.bump(tx2, [(60, 100)]), 3, pub_of(witness_d3))
    assert not rep.ok
    assert backend.prove(ProofOptions(*OPTS)) == before
    w = oracle.SchnorrWitness.generate(2, seed=9)
    ex = SchnorrExample(ProofOptions(*OPTS), w.messages, w.sig_rx, w.sig_s, backend)
    before = ex.prove()
    assert not run(backend, VC.SCHNORR, VC.bump(oracle.schnorr_build_trace(w), [(3, 100)]), 0, True).ok
    assert ex.prove() == before


def test_optional_outputs_do_not_change_the_report(backend, tx2, witness_d3):
    d = backend.from_numpy_u64(VC.bump(tx2, [(60, 100), (70, 1500)]))
    p = VC.bump(pub_of(witness_d3).reshape(1, 14), [(0, 9)])[0]
    a = backend.air_validate_trace(VC.TX, d, 3, p)
    b = backend.air_validate_trace(VC.TX, d, 3, p, want_cycles=True, want_frame=True)
    key = lambda r: (r.step, r.constraint, r.bad_cycles, r.boundary, r.boundary_register, r.boundary_step)
    assert key(a) == key(b) and a.cycle_codes is None and a.frame_values is None and b.frame_values is not None


# ---- 7. misuse -----------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_with_the_outputs_untouched(backend, tx2, witness_d3, schnorr2):
    from certificate_stark_amd import _lib
    lib = backend.lib
    d = backend.from_numpy_u64(tx2)
    ptr = backend._ptr(d)
    pub = pub_of(witness_d3).copy()
    big = pub.copy(); big[5] = np.uint64(P)
    rep = _lib.TraceReportStruct(step=77, constraint=78, bad_cycles=79, boundary=80, boundary_register=81, boundary_step=82)
    codes = np.full(2, 12345, np.uint32)
    frame = np.full(115, 54321, np.uint64)
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

    def call(ctx, air, trace, log_n, item, public, report):
        return lib.cstark_air_validate_trace(ctx, C.c_int(air), trace, C.c_uint32(log_n), C.c_uint32(item),
                                             None if public is None else public.ctypes.data_as(u64), report,
                                             codes.ctypes.data_as(u32), frame.ctypes.data_as(u64))
    sd = backend.from_numpy_u64(schnorr2[1])
    backend.upload_schnorr_witness(*[a[:1] for a in (schnorr2[0].messages, schnorr2[0].sig_rx, schnorr2[0].sig_s)])   # one signature resident, two in the trace
    cases = {
        "null ctx": (None, 0, ptr, 11, 3, pub, C.byref(rep)), "null trace": (backend.ctx, 0, None, 11, 3, pub, C.byref(rep)),
        "null report": (backend.ctx, 0, ptr, 11, 3, pub, None), "unknown air": (backend.ctx, 5, ptr, 11, 3, pub, C.byref(rep)),
        "negative air": (backend.ctx, -1, ptr, 11, 3, pub, C.byref(rep)), "short trace": (backend.ctx, 0, ptr, 9, 3, pub, C.byref(rep)),
        "long trace": (backend.ctx, 0, ptr, 25, 3, pub, C.byref(rep)), "bad depth": (backend.ctx, 0, ptr, 11, 4, pub, C.byref(rep)),
        "depth 0": (backend.ctx, 1, ptr, 11, 0, pub, C.byref(rep)), "public word >= p": (backend.ctx, 0, ptr, 11, 3, big, C.byref(rep)),
        "no statement of this length": (backend.ctx, 2, backend._ptr(sd), 10, 0, None, C.byref(rep)),
        "short rescue trace": (backend.ctx, 4, ptr, 2, 0, pub, C.byref(rep)),
    }
    for name, args in cases.items():
        assert call(*args) == -1, name
        assert (rep.step, rep.constraint, rep.bad_cycles, rep.boundary, rep.boundary_register, rep.boundary_step) == (77, 78, 79, 80, 81, 82), name
        assert (codes == 12345).all() and (frame == 54321).all(), name
    assert call(backend.ctx, 0, ptr, 11, 3, pub, C.byref(rep)) == 0 and rep.step == -1 and rep.boundary == -1 and (frame == 54321).all()
    assert (codes == VC.CLEAN).all()
