"""Ledger checkpoints on the GPU (cstark_ledger_checkpoint, _revert, _release, _root_at, _open_accounts_at) against copies of the plain
model (ledger_model.LedgerModel.copy()) taken at the moment of each checkpoint: openings under past roots, reverts, releases in every
order, no cost when unused, witness and proof unchanged under a live checkpoint, misuse, and a pool growth while a checkpoint is live.
Every state these tests reach is also audited (ledger_checkpoint_cases.assert_state): clean at id 0 and at every live id."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ledger_cases as LC
import ledger_checkpoint_cases as CC
import ledger_model as LM
import ledger_paths_cases as PC
import sig_cases as SC
from test_gpu_ledger import _assert_batch

pytestmark = pytest.mark.gpu

u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
DEPTHS = [1, 3, 15, 31]
INVALID_ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _applied(pair, n, among):
    got, want = pair.apply(n, among)
    _assert_batch(got, want)


def _started(backend, depth, seed=1):
    """accounts set, one batch applied: the state the first checkpoint names"""
    p = CC.Pair(backend, depth, seed)
    p.set_accounts(CC.ACCOUNTS[depth][0])
    _applied(p, 3, CC.ACCOUNTS[depth][0])
    return p


# ---- 1. openings under a past root --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_openings_under_past_roots(backend, depth):
    first, later = CC.ACCOUNTS[depth]
    p = _started(backend, depth)
    cp1 = p.checkpoint()
    assert cp1 == 1
    p.assert_all()
    # with id 0 and at=None the outputs are those of open / root
    plain, zero = p.led.open(p.ask), p.led.open(p.ask, at=0)
    for f in ("values", "present", "paths", "root"):
        assert np.array_equal(getattr(plain, f), getattr(zero, f)), f
    assert np.array_equal(p.led.root(), p.led.root(at=0))
    _applied(p, 2, first)                      # one further apply: accounts changed since, accounts untouched
    p.assert_all()
    _applied(p, 8, first)                      # two
    p.assert_all()
    if later:                                  # accounts created after the checkpoint, and one overwritten: absent at cp1, old siblings
        p.set_accounts(later + [first[1]])
        p.assert_all()
        assert not p.led.open(np.array(later, np.uint64), at=cp1).present.any() and p.led.open(np.array(later, np.uint64)).present.all()
    cp2 = p.checkpoint()
    assert cp2 == 2
    _applied(p, 5, first + later)              # three
    p.assert_all()
    assert not np.array_equal(p.led.root(at=cp1), p.led.root(at=cp2)) and not np.array_equal(p.led.root(at=cp2), p.led.root())
    p.close()


# ---- 2. revert ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_revert_restores_the_state_and_work_goes_on(backend, depth):
    from certificate_stark_amd import CstarkError
    first, later = CC.ACCOUNTS[depth]
    p = _started(backend, depth, seed=2)
    cp = p.checkpoint()
    before = p.m.copy()
    _applied(p, 4, first)
    if later:
        p.set_accounts(later + [first[0]])
    newer = p.checkpoint()
    _applied(p, 3, first + later)
    p.assert_all()
    p.revert(cp)                               # to the older of two: the newer id is gone
    assert np.array_equal(p.led.root(), before.root())
    values, present = p.led.accounts(np.array(first + later, np.uint64))
    assert list(present) == [i in before.value for i in first + later]
    assert np.array_equal(values[:len(first)], before.accounts(first)) and not values[len(first):].any()
    r = p.assert_all()
    assert (r.slots_held, r.n_nodes) == (0, before.n_nodes())
    for call in (lambda: p.led.root(at=newer), lambda: p.led.open(p.ask, at=newer), lambda: p.led.audit(at=newer), lambda: p.led.revert(newer),
                 lambda: p.led.release(newer)):
        with pytest.raises(CstarkError) as e:
            call()
        assert e.value.code == INVALID_ARG
    _applied(p, 6, first)                      # the next apply returns the eleven arrays the model returns
    p.assert_all()
    third = p.checkpoint()
    assert third == 3                          # ids are never reused
    _applied(p, 2, first)
    p.revert(cp)                               # cp itself a second time, after more applies
    assert np.array_equal(p.led.root(), before.root())
    r = p.assert_all()
    assert r.slots_held == 0
    _applied(p, 2, first)
    p.assert_all()
    p.close()


# ---- 3. release in every order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(itertools.permutations(range(3))), ids=lambda o: "".join(map(str, o)))
def test_release_in_every_order(backend, order):
    depth = 3
    first, later = CC.ACCOUNTS[depth]
    p = _started(backend, depth, seed=3)
    cps = [p.checkpoint()]
    _applied(p, 4, first)
    cps.append(p.checkpoint())
    p.set_accounts(later + [first[2]])
    _applied(p, 3, first + later)
    cps.append(p.checkpoint())
    _applied(p, 8, first + later)
    r = p.assert_all()
    assert r.slots_held > 0
    for k in order:
        p.release(cps[k])                      # the remaining checkpoints' openings are unchanged
        r = p.assert_all()
    assert (r.slots_held, r.slots_live) == (0, p.m.n_nodes())
    _applied(p, 2, first + later)
    r2 = p.assert_all()
    assert (r2.slots_held, r2.slots_free) == (0, r.slots_free)      # in place again: nothing taken, nothing freed
    p.close()


def test_release_at_depth_15_frees_what_only_the_checkpoint_kept(backend):
    depth = 15
    first, later = CC.ACCOUNTS[depth]
    p = _started(backend, depth, seed=4)
    a = p.checkpoint()
    _applied(p, 4, first)
    b = p.checkpoint()
    _applied(p, 4, first)
    held = p.assert_all().slots_held
    p.release(b)                               # the newest: its slots merge into its predecessor's log or go free
    assert 0 < p.assert_all().slots_held <= held
    p.release(a)
    r = p.assert_all()
    assert (r.slots_held, r.slots_live) == (0, p.m.n_nodes()) and r.slots_free >= held
    p.close()


# ---- 4. no cost when unused -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_a_ledger_without_checkpoints_holds_its_nodes_only(backend, depth):
    first, later = CC.ACCOUNTS[depth]
    p = CC.Pair(backend, depth, seed=5)
    p.set_accounts(first + later)
    for n in (2, 8, 5):
        _applied(p, n, first + later)
    r = p.assert_all()
    assert (r.slots_held, r.slots_free, r.slots_live) == (0, 0, p.m.n_nodes())
    p.close()


def test_a_refused_batch_under_a_live_checkpoint_changes_nothing(backend, oracle):
    from certificate_stark_amd.prover import Ledger, TransferRefused
    w = LC.generated((2, 3, 2))
    indices, initial = LC.initial_accounts(w)
    absent = LC.absent_index(w, indices)
    assert absent is not None
    led = Ledger(3, backend)
    led.set_accounts(indices, initial)
    cp = led.checkpoint()
    m = led.apply(SC.transfers(w, 0, 1), check_signatures=True)        # one applied transfer, so that the checkpoint's log is not empty
    assert np.array_equal(m.final_root, w.initial_roots[1])
    root, root_cp, report = led.root(), led.root(at=cp), CC.report_tuple(led.audit())
    assert report[7] > 0

    def refused(transfers, reason, at=0, **kw):
        with pytest.raises(TransferRefused) as e:
            led.apply(transfers, **kw)
        assert (e.value.index, e.value.reason) == (at, reason)
        assert CC.report_tuple(led.audit()) == report and CC.report_tuple(led.audit(at=cp))[:6] == (1, 0, 0, 0, 0, report[5])
        assert np.array_equal(led.root(), root) and np.array_equal(led.root(at=cp), root_cp)

    def changed(**kw):
        s, r, d, rx, ss = (a.copy() for a in SC.transfers(w, 1, 2))
        for name, value in kw.items():
            {"s": s, "r": r, "d": d}[name][0] = value
        return s, r, d, rx, ss

    refused(changed(r=8), Ledger.INDEX_RANGE)
    refused(changed(r=int(w.s_indices[1])), Ledger.SELF_TRANSFER)
    refused(changed(r=absent), Ledger.ABSENT)
    refused(changed(d=oracle.to_mont(np.array([SC.P - 1], np.uint64))[0]), Ledger.BALANCE)
    s, r, d, rx, ss = changed()
    ss[0, 0] ^= 1
    refused((s, r, d, rx, ss), Ledger.SIGNATURE, check_signatures=True)
    m = led.apply(SC.transfers(w, 1, 2), check_signatures=True)        # and the batch itself is still appliable
    assert np.array_equal(m.final_root, w.final_root) and np.array_equal(led.root(at=cp), w.initial_roots[0])
    led.close()


# ---- 5. witness and proof unchanged ---------------------------------------------------------------------------------------------------------
def test_apply_under_a_checkpoint_gives_the_same_witness_and_proof(backend):
    from certificate_stark_amd.prover import Ledger, get_example_options
    w = LC.generated((2, 3, 2))
    indices, initial = LC.initial_accounts(w)
    proofs, batches = [], []
    for with_checkpoint in (False, True):
        led = Ledger(3, backend)
        led.set_accounts(indices, initial)
        if with_checkpoint:
            led.checkpoint()
        batches.append(led.apply(SC.transfers(w)))
        _assert_batch(batches[-1], w)
        proofs.append(backend.prove(get_example_options()))             # from the resident witness
        led.close()
    assert proofs[0] == proofs[1] and len(proofs[0]) > 1000
    for f in ("initial_roots", "final_root", "s_old_values", "r_old_values", "s_indices", "r_indices", "s_paths", "r_paths", "deltas", "sig_rx", "sig_s"):
        assert np.array_equal(getattr(batches[0], f), getattr(batches[1], f)), f


# ---- 6. misuse ------------------------------------------------------------------------------------------------------------------------------
def test_misuse(backend):
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd import _lib
    lib, ctx = backend.lib, backend.ctx
    p, q = _started(backend, 3, seed=6), _started(backend, 3, seed=7)
    cp = p.checkpoint()
    for _ in range(3):
        theirs = q.checkpoint()
    assert (cp, theirs) == (1, 3)
    _applied(p, 2, CC.ACCOUNTS[3][0])
    led = p.led._led
    idx = np.array([0, 7, 5], np.uint64)

    def open_at(cp, indices=idx, null=None, ctx=ctx, led=led):
        n = len(indices)
        values, present = np.full((n, 14), PC.FILL64, np.uint64), np.full(n, PC.FILL8, np.uint8)
        paths, root = np.full((n, 4, 7), PC.FILL64, np.uint64), np.full(7, PC.FILL64, np.uint64)
        args = [indices.ctypes.data_as(u64p), values.ctypes.data_as(u64p), present.ctypes.data_as(u8p), paths.ctypes.data_as(u64p), root.ctypes.data_as(u64p)]
        if null is not None:
            args[null] = None
        rc = lib.cstark_ledger_open_accounts_at(ctx, led, C.c_uint64(cp), C.c_uint32(n), *args)
        untouched = all((a == (PC.FILL8 if a.dtype == np.uint8 else PC.FILL64)).all() for a in (values, present, paths, root))
        return rc, untouched

    assert open_at(cp) == (0, False)
    for null in range(5):
        assert open_at(cp, null=null) == (INVALID_ARG, True)
    assert open_at(theirs) == (INVALID_ARG, True)                       # an id of another ledger
    assert open_at(cp, indices=np.array([0, 8], np.uint64)) == (INVALID_ARG, True) and "indices[1]" in lib.cstark_last_error().decode()
    assert open_at(cp, ctx=None) == (INVALID_ARG, True) and open_at(cp, led=None) == (INVALID_ARG, True)
    other = Backend()
    assert open_at(cp, ctx=other.ctx) == (INVALID_ARG, True) and "another context" in lib.cstark_last_error().decode()
    root, out_id = np.full(7, PC.FILL64, np.uint64), C.c_uint64(77)
    report = _lib.LedgerAuditReportStruct(consistent=77)
    for rc in (lib.cstark_ledger_root_at(other.ctx, led, C.c_uint64(cp), root.ctypes.data_as(u64p)),
               lib.cstark_ledger_root_at(ctx, led, C.c_uint64(theirs), root.ctypes.data_as(u64p)),
               lib.cstark_ledger_root_at(ctx, led, C.c_uint64(cp), None),
               lib.cstark_ledger_root_at(ctx, None, C.c_uint64(cp), root.ctypes.data_as(u64p)),
               lib.cstark_ledger_checkpoint(ctx, led, None), lib.cstark_ledger_checkpoint(other.ctx, led, C.byref(out_id)),
               lib.cstark_ledger_checkpoint(None, led, C.byref(out_id)),
               lib.cstark_ledger_revert(other.ctx, led, C.c_uint64(cp)), lib.cstark_ledger_revert(ctx, led, C.c_uint64(theirs)),
               lib.cstark_ledger_revert(ctx, led, C.c_uint64(0)), lib.cstark_ledger_release(ctx, led, C.c_uint64(0)),
               lib.cstark_ledger_release(other.ctx, led, C.c_uint64(cp)), lib.cstark_ledger_release(ctx, None, C.c_uint64(cp)),
               lib.cstark_ledger_audit(ctx, led, C.c_uint64(cp), None), lib.cstark_ledger_audit(ctx, led, C.c_uint64(theirs), C.byref(report)),
               lib.cstark_ledger_audit(other.ctx, led, C.c_uint64(cp), C.byref(report))):
        assert rc == INVALID_ARG
    other.close()
    assert (root == PC.FILL64).all() and out_id.value == 77 and report.consistent == 77
    p.assert_all()                                                      # none of it changed anything
    p.release(cp)
    assert open_at(cp) == (INVALID_ARG, True)                           # a released id
    assert lib.cstark_ledger_release(ctx, led, C.c_uint64(cp)) == INVALID_ARG
    # the cap: 16 live checkpoints, one more is UNSUPPORTED, and a release makes room again
    ids = [p.checkpoint() for _ in range(16)]
    assert ids == list(range(2, 18))
    assert lib.cstark_ledger_checkpoint(ctx, led, C.byref(out_id)) == UNSUPPORTED and out_id.value == 77
    p.release(ids[5])
    assert p.checkpoint() == 18
    p.close()
    q.close()


# ---- 7. a pool growth while a checkpoint is live ----------------------------------------------------------------------------------------------
def test_1024_transfers_cross_a_pool_growth_under_a_live_checkpoint(backend):
    """The committed 1,024-transfer depth-15 witness: set_accounts reserves room for 1,996 (depth + 1) nodes, 32,768 slots; the batch may
    touch 2,048 (depth + 1) = 32,768 nodes more than are stored, so the pool doubles, and moves, while the checkpoint is live.  The
    reference of the old state is the opening taken before the batch, and the witness's own first root."""
    from certificate_stark_amd.prover import Ledger
    w = LC.golden_1024()
    indices, initial = LC.initial_accounts(w)
    assert len(indices) == 1996 and w.depth == 15
    led = Ledger(15, backend)
    led.set_accounts(indices, initial)
    before = led.open(indices)
    cp = led.checkpoint()
    _assert_batch(led.apply(SC.transfers(w)), w)
    past = led.open(indices, at=cp)
    for f in ("values", "present", "paths", "root"):
        assert np.array_equal(getattr(past, f), getattr(before, f)), f
    assert np.array_equal(past.root, w.initial_roots[0]) and np.array_equal(past.values, initial) and not past.check().any()
    now = led.open(indices)
    assert np.array_equal(now.root, w.final_root) and np.array_equal(now.values, LC.final_accounts(w, indices)) and not now.check().any()
    r0, r1 = led.audit(), led.audit(at=cp)
    assert (r0.consistent, r0.n_bad, r1.consistent, r1.n_bad) == (1, 0, 1, 0) and r0.n_nodes == r1.n_nodes == r0.slots_live
    assert r0.slots_held == r0.slots_live                               # every account was touched: every node was redirected once
    led.revert(cp)
    back = led.open(indices)
    assert np.array_equal(back.paths, before.paths) and np.array_equal(back.root, before.root) and np.array_equal(back.values, initial)
    r = led.audit()
    assert (r.consistent, r.slots_held, r.slots_free) == (1, 0, r0.slots_held)
    _assert_batch(led.apply(SC.transfers(w)), w)                        # the same batch on the restored state, in the freed slots
    assert led.audit().slots_free == 0 and np.array_equal(led.root(), w.final_root)
    led.close()
