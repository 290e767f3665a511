"""cstark_tx_witness_check on the GPU against the plain model of witness_check_cases.py: verdicts, first_bad, n_bad, the four folds of
every transfer and the final root, compared whole (every output buffer starts as 0xA5 with spare room).  Honest witnesses at 1, 2, 3 and
8 transfers and depths 1, 3, 15 and 31; the steered batches (sibling and opposite-half pairs, bit 30 of an index, deltas of 0 and of the
balance, a nonce of p - 1, a receiver balance that wraps past p); single-word mutations of every field, each expected to give what the
model gives; both forms -- the host witness and the resident one after upload_witness and after Ledger.apply; signatures; misuse that
launches nothing; a proof after checks is the proof without them; the committed 1024-transfer witness in one launch."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC
import ledger_scenarios as LS
import witness_check_cases as WC

pytestmark = pytest.mark.gpu

u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
SPARE = 2
SIGNATURES = 1     # CSTARK_WITNESS_CHECK_SIGNATURES
UNSET = object()


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _error(backend):
    return backend.lib.cstark_last_error().decode()


def _call(backend, w=None, n=None, final_root=None, flags=0, report=UNSET, want_verdicts=True, want_folds=True, null_field=None):
    """the C call on 0xA5-filled outputs, SPARE rows longer than it needs -> (status, report, verdicts, folds).  w: a witness object (the
    host form) or None (the resident form, n its number of transfers)"""
    from certificate_stark_amd import _lib
    n = w.n_tx if w is not None else n
    rep = _lib.WitnessReportStruct()
    C.memset(C.byref(rep), WC.FILL8, C.sizeof(rep))
    verdicts = np.full(n + SPARE, WC.FILL8, np.uint8)
    folds = np.full((n + SPARE, 4, 7), WC.FILL64, np.uint64)
    arg = None
    if w is not None:
        s, keep = backend._witness_struct(w)
        if null_field:
            setattr(s, null_field, None)
        arg = C.byref(s)
    root = None if final_root is None else np.ascontiguousarray(final_root, np.uint64)
    rc = backend.lib.cstark_tx_witness_check(backend.ctx, arg, None if root is None else root.ctypes.data_as(u64p), C.c_uint32(flags),
                                             C.byref(rep) if report is UNSET else report, verdicts.ctypes.data_as(u8p) if want_verdicts else None,
                                             folds.ctypes.data_as(u64p) if want_folds else None)
    return rc, rep, verdicts, folds


def _untouched(rep, verdicts, folds):
    return bytes(rep) == bytes([WC.FILL8]) * C.sizeof(rep) and (verdicts == WC.FILL8).all() and (folds == WC.FILL64).all()


def _assert_is(backend, got, e, n, depth):
    """the outputs of one call are the model's, whole"""
    rc, rep, verdicts, folds = got
    assert rc == 0, _error(backend)
    assert list(verdicts[:n]) == list(e.verdicts), ([WC.NAMES[v] for v in verdicts[:n]], [WC.NAMES[v] for v in e.verdicts])
    assert np.array_equal(folds[:n], e.folds)
    assert (rep.n_tx, rep.merkle_depth, rep.first_bad, rep.first_verdict, rep.n_bad, rep.reserved) == (n, depth, e.first_bad, e.first_verdict, e.n_bad, 0)
    assert np.array_equal(np.array(list(rep.final_root), np.uint64), e.final_root)
    assert (verdicts[n:] == WC.FILL8).all() and (folds[n:] == WC.FILL64).all()


def _assert_host(backend, w, check_signatures=False, e=None):
    e = e or WC.check(w, check_signatures=check_signatures)
    _assert_is(backend, _call(backend, w, flags=SIGNATURES if check_signatures else 0), e, w.n_tx, w.depth)
    return e


# ---- 1. honest witnesses, host form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", WC.DEPTHS)
@pytest.mark.parametrize("n_tx", WC.SIZES)
def test_generated_witness_is_valid(backend, n_tx, depth):
    w = WC.generated(n_tx, depth)
    e = _assert_host(backend, w, check_signatures=True)
    assert not e.verdicts.any() and np.array_equal(e.final_root, w.final_root)


@pytest.mark.parametrize("case", WC.steered(), ids=lambda c: c[0])
def test_steered_witness_is_valid(backend, case):
    name, w = case
    e = _assert_host(backend, w)
    assert not e.verdicts.any()


def test_unsigned_steered_transfers_fail_the_signature_test_only(backend):
    name, w = WC.steered()[0]
    e = _assert_host(backend, w, check_signatures=True)
    assert list(e.verdicts) == [WC.SIGNATURE] * w.n_tx


# ---- 2. mutations: the verdict names the part that was changed ------------------------------------------------------------------------
@pytest.mark.parametrize("depth", WC.DEPTHS)
def test_every_mutation_gets_the_models_verdict(backend, depth):
    kinds = set()
    for name, m, e in WC.mutation_set(depth):
        got = _call(backend, m, flags=SIGNATURES)
        try:
            _assert_is(backend, got, e, 3, depth)
        except AssertionError as err:
            raise AssertionError("mutation %s: %s" % (name, err))
        kinds.update(int(v) for v in got[2][:3])
    assert kinds == set(range(10))


@pytest.mark.parametrize("depth", [3, 31])
def test_without_the_flag_a_bad_signature_is_no_finding(backend, depth):
    by_name = {name: (m, e) for name, m, e in WC.mutation_set(depth)}
    for name in ("sig_s_byte", "sig_rx", "sig_s_bit255"):
        m, e = by_name[name]
        assert list(e.verdicts) == [WC.VALID, WC.SIGNATURE, WC.VALID]
        plain = _assert_host(backend, m)
        assert not plain.verdicts.any()
    m, e = by_name["path_and_signature"]     # the order rule: the path is reported, with and without the flag
    assert e.verdicts[1] == WC.SENDER_PATH and _assert_host(backend, m).verdicts[1] == WC.SENDER_PATH


def test_several_bad_transfers_each_get_their_own_verdict(backend):
    m = WC._copy(WC.generated(8, 15))
    WC._bump(m.s_paths, (1, 9, 0))
    WC._bump(m.r_paths, (4, 0, 0))
    m.s_indices[6] = 1 << 15
    WC._bump(m.initial_roots, (7, 0))
    e = _assert_host(backend, m)
    assert list(e.verdicts) == [0, WC.SENDER_PATH, 0, 0, WC.RECEIVER_LEAF, 0, WC.INDEX_RANGE, WC.SENDER_PATH] and e.first_bad == 1 and e.n_bad == 4
    assert e.folds.shape == (8, 4, 7)


def test_optional_outputs_may_be_null(backend):
    w = WC.generated(3, 3)
    e = WC.check(w)
    rc, rep, verdicts, folds = _call(backend, w, want_verdicts=False, want_folds=False)
    assert rc == 0 and rep.first_bad == -1 and np.array_equal(np.array(list(rep.final_root), np.uint64), e.final_root)
    assert (verdicts == WC.FILL8).all() and (folds == WC.FILL64).all()


# ---- 3. the resident form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", WC.DEPTHS)
def test_resident_witness_after_upload(backend, depth):
    by_name = {name: (m, e) for name, m, e in WC.mutation_set(depth)}
    w = WC.generated(3, depth)
    backend.upload_witness(w)
    _assert_is(backend, _call(backend, n=3, final_root=w.final_root, flags=SIGNATURES), WC.check(w, check_signatures=True), 3, depth)
    _assert_is(backend, _call(backend, n=3), WC.check(w, final_root=None), 3, depth)
    wrong = w.final_root.copy()
    WC._bump(wrong, 4)
    e = WC.check(w, final_root=wrong)
    assert list(e.verdicts) == [WC.VALID, WC.VALID, WC.NEXT_ROOT]
    _assert_is(backend, _call(backend, n=3, final_root=wrong), e, 3, depth)
    # a mutated resident witness, its own final root mutated or not: without a stated root the last NEXT_ROOT test does not run
    for name in ("final_root", "next_initial_root", "receiver_leaf_and_signature", "r_index_bit63"):
        m, e = by_name[name]
        backend.upload_witness(m)
        _assert_is(backend, _call(backend, n=3, final_root=m.final_root, flags=SIGNATURES), e, 3, depth)
        _assert_is(backend, _call(backend, n=3), WC.check(m, final_root=None), 3, depth)
    assert not WC.check(by_name["final_root"][0], final_root=None).verdicts.any()


@pytest.mark.parametrize("sc", [LS.BY_NAME[n] for n in ("pingpong_siblings", "receiver_wraps_p", "depth31_edges", "depth1_busy", "single_deep")],
                         ids=lambda sc: sc.name)
def test_resident_witness_after_apply(backend, sc):
    from certificate_stark_amd.prover import Ledger
    led = Ledger(sc.depth, backend)
    led.set_accounts(sc.indices(), LS.values(sc))
    led.apply(LS.transfers(sc), want_witness=False)
    w = LS.expected(sc).witness
    report, verdicts = backend.tx_witness_check(final_root=led.root())
    assert report.first_bad == -1 and report.n_bad == 0 and not verdicts.any()
    assert np.array_equal(np.array(list(report.final_root), np.uint64), led.root())
    _assert_is(backend, _call(backend, n=sc.n_tx, final_root=led.root()), WC.check(w), sc.n_tx, sc.depth)
    wrong = led.root().copy()
    WC._bump(wrong, 0)
    report, verdicts = backend.tx_witness_check(final_root=wrong)
    assert list(verdicts) == [WC.VALID] * (sc.n_tx - 1) + [WC.NEXT_ROOT] and (report.first_bad, report.n_bad) == (sc.n_tx - 1, 1)
    assert np.array_equal(np.array(list(report.final_root), np.uint64), led.root())
    led.close()


def test_a_batch_signed_by_the_ledger_is_valid_and_a_flipped_byte_is_found(backend):
    from certificate_stark_amd.prover import TransactionMetadata
    from test_gpu_ledger_sign import SEED, case
    c = case(3)
    led = c.ledger(backend)
    signed = led.sign(c.batch, c.secrets, seed=SEED)
    m = led.apply(signed)
    n = m.n_tx
    report, verdicts = backend.tx_witness_check(final_root=led.root(), check_signatures=True)
    assert report.first_bad == -1 and not verdicts.any()
    checked = m.check(backend, check_signatures=True)
    assert checked.ok and checked.verdict == "VALID" and checked.first_bad is None and np.array_equal(checked.final_root, led.root())
    led.close()
    forged = TransactionMetadata(*[getattr(m, f).copy() for f in TransactionMetadata.FIELDS])
    forged.sig_s[5, 9] ^= 0x04
    assert not forged.check(backend).verdicts.any()
    found = forged.check(backend, check_signatures=True)
    assert list(found.verdicts) == [WC.VALID] * 5 + [WC.SIGNATURE] + [WC.VALID] * (n - 6)
    assert (found.ok, found.first_bad, found.verdict, found.n_bad) == (False, 5, "SIGNATURE", 1) and "transfer 5: SIGNATURE" in str(found)
    led = c.ledger(backend)                    # the unchecked apply copies the forged signature through: the resident form finds it too
    led.apply(tuple(getattr(forged, f) for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s")), want_witness=False)
    report, verdicts = backend.tx_witness_check(final_root=led.root(), check_signatures=True)
    assert (report.first_bad, report.first_verdict, report.n_bad) == (5, WC.SIGNATURE, 1)
    led.close()


def test_python_layers(backend):
    from certificate_stark_amd import prover
    from certificate_stark_amd.backend import Backend
    assert prover.WITNESS_VERDICTS == WC.NAMES
    assert [getattr(Backend, "WITNESS_" + name) for name in WC.NAMES] == list(range(10))
    name, m, e = WC.mutation_set(3)[0]
    md = prover.TransactionMetadata(*[getattr(m, f) for f in prover.TransactionMetadata.FIELDS])
    got = md.check(backend, want_folds=True)
    plain = WC.check(m)
    assert list(got.verdicts) == list(plain.verdicts) and np.array_equal(got.folds, plain.folds) and np.array_equal(got.final_root, plain.final_root)
    assert (got.first_bad, got.verdict, got.n_bad) == (plain.first_bad, WC.NAMES[plain.first_verdict], plain.n_bad)
    ex = prover.TransactionExample(prover.get_example_options(), md, backend)
    assert list(ex.check_witness(check_signatures=True).verdicts) == list(e.verdicts)
    with pytest.raises(ValueError):
        backend.tx_witness_check(md, final_root=md.final_root)


# ---- 4. misuse: nothing is launched, the outputs are untouched -------------------------------------------------------------------------
def test_misuse_leaves_the_outputs_untouched(backend):
    from certificate_stark_amd.backend import Backend
    w = WC.generated(3, 3)
    for field in ("initial_roots", "final_root", "s_old_values", "r_old_values", "s_paths", "r_paths", "deltas", "sig_rx"):
        m = WC._copy(w)
        a = getattr(m, field)
        at = (2,) + (0,) * (a.ndim - 2) + (min(a.shape[-1] - 1, 5),) if field not in ("final_root", "deltas") else (2,)
        a[at] = WC.P
        rc, *outputs = _call(backend, m)
        assert rc == -1 and _untouched(*outputs), field
        where = "%s[%s]" % (field, "][".join(str(k) for k in (at if field != "final_root" else (0,) + at) + ((0,) if field == "deltas" else ())))
        assert where in _error(backend), (where, _error(backend))
    for field in WC.generated(1, 3).FIELDS:
        rc, *outputs = _call(backend, w, null_field=field)
        assert rc == -1 and _untouched(*outputs), field
    rc, *outputs = _call(backend, w, final_root=w.final_root)
    assert rc == -1 and _untouched(*outputs) and "resident form" in _error(backend)
    rc, *outputs = _call(backend, w, flags=2)
    assert rc == -1 and _untouched(*outputs)
    rc, *outputs = _call(backend, w, report=None)
    assert rc == -1 and _untouched(*outputs)
    for n_tx, depth in ((0, 3), (3, 0), (3, 2), (3, 63)):
        m = WC._copy(w)
        m.n_tx, m.depth = n_tx, depth
        rc, *outputs = _call(backend, m, n=3)
        assert rc == -1 and _untouched(*outputs), (n_tx, depth)
    fresh = Backend()            # a context without a resident witness
    rc, *outputs = _call(fresh, n=3)
    assert rc == -1 and _untouched(*outputs) and "no transaction witness" in _error(fresh)
    fresh.close()
    backend.upload_witness(w)
    bad_root = w.final_root.copy()
    bad_root[6] = 2**64 - 1
    rc, *outputs = _call(backend, n=3, final_root=bad_root)
    assert rc == -1 and _untouched(*outputs) and "final_root[0][6]" in _error(backend)


# ---- 5. read-only: proofs and traces are what they are without a check ----------------------------------------------------------------
def test_a_proof_after_checks_is_the_proof_without_them(backend):
    from certificate_stark_amd.backend import Backend, to_numpy_u64
    from certificate_stark_amd.prover import get_example_options
    w, other = WC.generated(8, 3), WC.mutation_set(15)[0][1]
    plain = Backend()
    plain.upload_witness(w)
    trace_ref = to_numpy_u64(plain.build_trace())
    proof_ref = plain.prove(get_example_options())
    plain.close()
    backend.upload_witness(w)
    assert _call(backend, n=8, final_root=w.final_root, flags=SIGNATURES)[1].first_bad == -1
    assert _call(backend, other, flags=SIGNATURES)[0] == 0       # a host witness of another shape beside the resident one
    assert np.array_equal(to_numpy_u64(backend.build_trace()), trace_ref)
    assert _call(backend, n=8, flags=SIGNATURES)[1].first_bad == -1
    assert backend.prove(get_example_options()) == proof_ref
    _assert_is(backend, _call(backend, n=8, final_root=w.final_root), WC.check(w), 8, 3)


def test_the_call_block_grows_and_is_reused(backend):
    """a small, a large and the small request again on one fresh context, in both forms: the block the context keeps for the call is
    grown once and answers the same before and after"""
    from certificate_stark_amd.backend import Backend
    b = Backend()
    small, large = WC.generated(1, 1), WC.generated(8, 31)
    for w in (small, large, small, large):
        _assert_is(b, _call(b, w, flags=SIGNATURES), WC.check(w, check_signatures=True), w.n_tx, w.depth)
        b.upload_witness(small)
        _assert_is(b, _call(b, n=1, final_root=small.final_root), WC.check(small), 1, 1)
    b.close()


# ---- 6. the committed 1024-transfer witness: one launch, needs no model ---------------------------------------------------------------
def test_the_committed_1024_transfer_witness_is_valid(backend):
    w = LC.golden_1024()
    rc, rep, verdicts, folds = _call(backend, w, flags=SIGNATURES)
    assert rc == 0, _error(backend)
    assert (rep.n_tx, rep.merkle_depth, rep.first_bad, rep.first_verdict, rep.n_bad) == (1024, 15, -1, 0, 0) and not verdicts[:1024].any()
    assert np.array_equal(np.array(list(rep.final_root), np.uint64), w.final_root)
    assert np.array_equal(folds[:1024, 0], w.initial_roots) and np.array_equal(folds[:1023, 3], w.initial_roots[1:])
    assert np.array_equal(folds[:1024, 1], folds[:1024, 2])
    assert (verdicts[1024:] == WC.FILL8).all() and (folds[1024:] == WC.FILL64).all()
