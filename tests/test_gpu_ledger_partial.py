"""The partial ledger on the GPU (cstark_ledger_create_partial, Ledger.from_opening): a ledger P built from a multi-opening of a full
ledger F behaves as F does for the opened accounts -- batches, witnesses, roots, openings, refusals, checkpoints, audit, proofs -- and
refuses whatever names an account it does not know.  F itself is pinned against the plain model elsewhere; here P is compared with F byte
for byte, and the audit's expectations come from the reference's proof positions (multiproof_cases.py).  Every raw output buffer starts as
0xA5 and is compared whole."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC
import ledger_checkpoint_cases as CC
import ledger_model as LM
import ledger_scenarios as LS
import multiproof_cases as MC
import partial_cases as PC

pytestmark = pytest.mark.gpu

u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
FILL32 = 0xA5A5A5A5
UNKNOWN = 6


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _ptr(a, typ=u64p):
    return None if a is None else a.ctypes.data_as(typ)


def _error(backend):
    return backend.lib.cstark_last_error().decode()


def _untouched(*buffers):
    return all((a == {1: MC.FILL8, 4: FILL32, 8: MC.FILL64}[a.dtype.itemsize]).all() for a in buffers)


def _pair(backend, sc, at=None):
    """(F, P, opened): the full ledger of a scenario and the partial one built from the opening of PC.opened(sc)"""
    from certificate_stark_amd.prover import Ledger
    F = Ledger(sc.depth, backend)
    F.set_accounts(sc.indices(), LS.values(sc))
    opened = PC.opened(sc)
    opening = F.open_multi(opened, at=at)
    P = Ledger.from_opening(opening)
    assert P.partial and not F.partial and P.depth == sc.depth
    assert P.partial_info() == (True, len(opened), len(opening.nodes)) and F.partial_info() == (False, len(sc.accounts), 0)
    assert np.array_equal(P.root(), F.root()) and np.array_equal(P.root(), opening.root)
    return F, P, opened


def _same_witness(a, b):
    from certificate_stark_amd.prover import TransactionMetadata
    for f in TransactionMetadata.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


def _same_openings(F, P, opened, at_f=None, at_p=None):
    a, b = F.open(opened, at=at_f), P.open(opened, at=at_p)
    for f in ("values", "present", "paths", "root"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for subset in (opened, opened[::2], opened[-1:], opened[1:]):
        if len(subset):
            a, b = F.open_multi(subset, at=at_f), P.open_multi(subset, at=at_p)
            for f in ("indices", "values", "present", "nodes", "root"):
                assert np.array_equal(getattr(a, f), getattr(b, f)), f
    va, pa = F.accounts(opened)
    vb, pb = P.accounts(opened)
    assert np.array_equal(va, vb) and np.array_equal(pa, pb)


# ---- 1. equivalence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_a_partial_ledger_follows_the_full_one(backend, sc):
    F, P, opened = _pair(backend, sc)
    assert list(P.known(opened)) == [True] * len(opened)
    _same_openings(F, P, opened)
    opening = F.open_multi(opened)
    half = max(1, sc.n_tx // 2)
    for lo, hi in ((0, half), (half, sc.n_tx)):
        if lo == hi:
            continue
        _same_witness(F.apply(LS.transfers(sc, lo, hi)), P.apply(LS.transfers(sc, lo, hi)))
        assert np.array_equal(F.root(), P.root())
        _same_openings(F, P, opened)
        assert P.audit().consistent == 1
    assert np.array_equal(P.root(), LS.expected(sc).final_root)
    # the cross-check: the root P reaches is what the update check computes from the opening and the accounts after the batch
    got = opening.check_update(*P.accounts(opened))
    assert got.verdict == 0 and np.array_equal(got.new_root, P.root())
    F.close()
    P.close()


@pytest.mark.parametrize("sc,at,reason", LS.REFUSALS, ids=lambda v: getattr(v, "name", None))
def test_refusals_are_the_full_ledgers(backend, sc, at, reason):
    from certificate_stark_amd.prover import TransferRefused
    F, P, opened = _pair(backend, sc)
    root = P.root()
    for led in (F, P):
        with pytest.raises(TransferRefused) as e:
            led.apply(LS.transfers(sc))
        assert (e.value.index, e.value.reason) == (at, reason)
    assert np.array_equal(P.root(), root)
    _same_openings(F, P, opened)
    if at:
        _same_witness(F.apply(LS.transfers(sc, 0, at)), P.apply(LS.transfers(sc, 0, at)))
        _same_openings(F, P, opened)
    F.close()
    P.close()


# ---- 2. small shapes where the fold can go wrong --------------------------------------------------------------------------------------------------
def _from_model(backend, m, indices):
    from certificate_stark_amd.prover import Ledger
    indices = np.asarray(indices, np.uint64)
    values, present = MC.accounts_from_model(m, indices)
    nodes = MC.nodes_from_model(m, indices)
    P = Ledger.from_opening((m.depth, indices, values, present, nodes, m.root()), backend=backend)
    assert np.array_equal(P.root(), m.root())
    assert P.partial_info() == (True, len(indices), len(nodes))
    r = P.audit()
    stored = int(present.sum()) + len(nodes) + MC.shape(m.depth, indices)[1]
    assert (r.consistent, r.n_bad, r.n_nodes) == (1, 0, stored), CC.report_tuple(r)
    o = P.open_multi(indices)
    assert np.array_equal(o.nodes, nodes) and np.array_equal(o.values, values) and np.array_equal(o.present, present.astype(bool))
    paths = P.open(indices)
    assert not paths.check().any()
    for k, i in enumerate(indices):
        assert np.array_equal(paths.paths[k], m._path(int(i))), int(i)
    return P


def _model(depth, have, seed):
    m = LM.LedgerModel(depth)
    m.set_accounts(have, LS.account_values([(LS.B + i, i) for i in range(len(have))], seed=seed))
    return m


@pytest.mark.parametrize("name,depth,indices", [
    ("depth_1_one_leaf", 1, [1]),
    ("depth_1_both", 1, [0, 1]),
    ("depth_3_all_leaves", 3, list(range(8))),
] + [("depth_7_count_%d" % n, 7, [8 * k + (k % 2) for k in range(n)]) for n in (1, 2, 3, 4, 5, 8, 9)] + [
    ("depth_31_above_2_to_the_24", 31, sorted([2**24 + 1, 2**30 + 3, 2**30 + 2**24, 2**30 + 2**24 + 1, 2**31 - 2, 2**30 + 2, 2**31 - 1, 2**24])),
])
def test_small_shapes(backend, name, depth, indices):
    size = 1 << depth
    have = sorted(set(indices[::2] + [indices[-1]] + ([size - 1] if depth == 7 else [])))
    m = _model(depth, have, seed=len(name))
    P = _from_model(backend, m, indices)
    # a batch among the opened present accounts, and an opened absent account created, as in the model
    inside = [i for i in indices if i in m.value]
    absent = [i for i in indices if i not in m.value]
    if absent:
        fresh = LS.account_values([(5, 0)], seed=3)
        P.set_accounts(np.array(absent[:1], np.uint64), fresh)
        m.set_accounts(absent[:1], fresh)
        inside.append(absent[0])
    if len(inside) >= 2:
        tr = LS.transfer_arrays([(inside[0], inside[-1], 1), (inside[-1], inside[0], 2)])
        w = P.apply(tr)
        ref = m.apply(*tr)
        assert np.array_equal(w.final_root, ref.final_root) and np.array_equal(w.s_paths, ref.s_paths) and np.array_equal(w.r_paths, ref.r_paths)
    assert np.array_equal(P.root(), m.root()) and P.audit().consistent == 1
    P.close()


# ---- 3. UNKNOWN ---------------------------------------------------------------------------------------------------------------------------------
def test_unknown_accounts_are_refused(backend):
    from certificate_stark_amd.prover import Ledger, TransferRefused, get_example_options
    sc = LS.BY_NAME["bystander_siblings"]          # depth 7: accounts 10 11 20 21 8 9 22 23 127, all with balance B
    F = Ledger(7, backend)
    F.set_accounts(sc.indices(), LS.values(sc))
    opened = np.array([10, 11, 12, 20], np.uint64)          # 12 is a known absent account; 21, 8 and 127 exist and are unknown; 13 is neither
    P = F.open_multi(opened).to_ledger()
    assert list(P.known([10, 12, 21, 13, 127, 128, 2**40])) == [True, True, False, False, False, False, False]
    assert list(F.known([10, 12, 21, 13, 127, 128, 2**40])) == [True, True, True, True, True, False, False]
    backend.upload_witness(LC.generated((2, 3, 2)))
    resident = backend.prove(get_example_options())
    root, before = P.root(), P.accounts(opened)
    good = (10, 11, 1)
    cases = [
        ([(21, 10, 1)], 0, UNKNOWN), ([(10, 21, 1)], 0, UNKNOWN),                         # sender, receiver, at transfer 0
        ([good, good, (21, 10, 1)], 2, UNKNOWN), ([good, (10, 21, 1), good], 1, UNKNOWN),     # and later
        ([good, (21, 21, 1)], 1, LM.SELF_TRANSFER), ([good, (21, 128, 1)], 1, LM.INDEX_RANGE),     # index range and self come first
        ([good, (12, 21, 1)], 1, UNKNOWN), ([good, (13, 10, 1)], 1, UNKNOWN),                 # before ABSENT: known absent with unknown, unknown absent
        ([good, (10, 21, 5 * LS.B)], 1, UNKNOWN),                                           # before BALANCE
        ([good, (10, 12, 1)], 1, LM.ABSENT), ([good, (10, 11, 5 * LS.B)], 1, LM.BALANCE),    # known accounts: as in a full ledger
    ]
    for tr, at, reason in cases:
        for checked in (False, True):          # apply_checked: the arbitrary signatures are bad, but only transfers BEFORE the refusal are checked
            with pytest.raises(TransferRefused) as e:
                P.apply(LS.transfer_arrays(tr), check_signatures=checked)
            want = (at, reason) if not checked or at == 0 else (0, Ledger.SIGNATURE)
            assert (e.value.index, e.value.reason) == want, (tr, checked)
        assert np.array_equal(P.root(), root)
    after = P.accounts(opened)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert backend.prove(get_example_options()) == resident
    assert Ledger.REASONS[Ledger.UNKNOWN] and Ledger.UNKNOWN == UNKNOWN
    _same_witness(F.apply(LS.transfer_arrays([good])), P.apply(LS.transfer_arrays([good])))
    F.close()
    P.close()


def test_unknown_indices_are_misuse(backend):
    sc = LS.BY_NAME["bystander_siblings"]
    from certificate_stark_amd.prover import Ledger
    F = Ledger(7, backend)
    F.set_accounts(sc.indices(), LS.values(sc))
    P = F.open_multi([10, 11, 12, 20]).to_ledger()
    cp = P.checkpoint()
    root = P.root()
    lib, ctx, led = backend.lib, backend.ctx, P._led
    idx = np.array([10, 20, 21, 8], np.uint64)          # position 2 is the first unknown one
    n = len(idx)
    values, present = np.full((n, 14), MC.FILL64, np.uint64), np.full(n, MC.FILL8, np.uint8)
    paths, out_root = np.full((n, 8, 7), MC.FILL64, np.uint64), np.full(7, MC.FILL64, np.uint64)
    nodes, n_nodes = np.full((32, 7), MC.FILL64, np.uint64), np.full(1, FILL32, np.uint32)
    calls = {
        "get_accounts": lambda: lib.cstark_ledger_get_accounts(ctx, led, C.c_uint32(n), _ptr(idx), _ptr(values), _ptr(present, u8p)),
        "open_accounts": lambda: lib.cstark_ledger_open_accounts(ctx, led, C.c_uint32(n), _ptr(idx), _ptr(values), _ptr(present, u8p), _ptr(paths), _ptr(out_root)),
        "open_accounts_at": lambda: lib.cstark_ledger_open_accounts_at(ctx, led, C.c_uint64(cp), C.c_uint32(n), _ptr(idx), _ptr(values), _ptr(present, u8p),
                                                                       _ptr(paths), _ptr(out_root)),
        "open_multi": lambda: lib.cstark_ledger_open_multi(ctx, led, C.c_uint64(0), C.c_uint32(n), _ptr(np.sort(idx)), _ptr(values), _ptr(present, u8p),
                                                           _ptr(nodes), C.c_uint32(32), _ptr(n_nodes, u32p), _ptr(out_root)),
        "set_accounts": lambda: lib.cstark_ledger_set_accounts(ctx, led, C.c_uint32(n), _ptr(idx), _ptr(np.ascontiguousarray(LS.account_values([(1, 1)] * n)))),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert ("indices[0]" if name == "open_multi" else "indices[2]") in _error(backend) and "knows" in _error(backend), (name, _error(backend))
        assert _untouched(values, present, paths, out_root, nodes, n_nodes), name
        assert np.array_equal(P.root(), root), name
    assert P.audit().consistent == 1
    F.close()
    P.close()


# ---- 4. tampered openings give no ledger ---------------------------------------------------------------------------------------------------------
def test_tampered_openings_give_no_ledger(backend):
    from certificate_stark_amd.prover import Ledger
    sc = LS.BY_NAME["bystander_siblings"]
    F = Ledger(7, backend)
    F.set_accounts(sc.indices(), LS.values(sc))
    o = F.open_multi([8, 10, 12, 20, 127])
    F.close()

    def refused(verdict, at, indices=o.indices, values=o.values, nodes=o.nodes, root=o.root):
        with pytest.raises(ValueError) as e:
            Ledger.from_opening((7, indices, values, o.present, nodes, root), backend=backend)
        assert (e.value.verdict, e.value.at) == (verdict, at)
        led, v, a = backend.ledger_create_partial(7, indices, values, o.present, nodes, root)
        assert led is None and (v, a) == (verdict, at)
        fresh = Ledger(7, backend)              # a following Ledger(depth) still works
        fresh.set_accounts(sc.indices(), LS.values(sc))
        assert np.array_equal(fresh.root(), o.root)
        fresh.close()

    def bumped(a, *where):
        a = a.copy()
        a[where] = MC.bump(a[where])
        return a

    refused(MC.ROOT, 0, nodes=bumped(o.nodes, 1, 3))
    refused(MC.ROOT, 0, values=bumped(o.values, 1, 12))
    refused(MC.ROOT, 0, root=bumped(o.root, 6))
    refused(MC.INDEX, 2, indices=o.indices[[0, 2, 1, 3, 4]])
    refused(MC.NODE_COUNT, len(o.nodes), nodes=o.nodes[:-1])
    P = o.to_ledger()
    assert np.array_equal(P.root(), o.root)
    P.close()
    # misuse: outputs untouched, the first unreduced word named in the order values, nodes, root
    idx, val, pres, nd, root = (np.ascontiguousarray(a) for a in (o.indices, o.values, o.present.astype(np.uint8), o.nodes, o.root))

    def raw(depth=7, count=None, val=val, nd=nd, root=root, n_nodes=None, null=()):
        out, verdict, at = np.full(1, MC.FILL64, np.uint64), np.full(1, FILL32, np.uint32), np.full(1, FILL32, np.uint32)
        args = [_ptr(idx), _ptr(val), _ptr(pres, u8p), _ptr(nd), C.c_uint32(len(nd) if n_nodes is None else n_nodes), _ptr(root), _ptr(out),
                _ptr(verdict, u32p), _ptr(at, u32p)]
        for k in null:
            args[k] = None
        rc = backend.lib.cstark_ledger_create_partial(backend.ctx, C.c_uint32(depth), C.c_uint32(len(idx) if count is None else count), *args)
        assert rc == -1 and _untouched(out, verdict, at)
        return _error(backend)

    for null in (0, 1, 3, 5, 6, 7, 8):
        raw(null=(null,))
    raw(n_nodes=0)
    raw(count=0)
    for depth in (0, 2, 6, 32):
        assert "depth" in raw(depth=depth)
    bad_val, bad_nd, bad_root = val.copy(), nd.copy(), root.copy()
    bad_val[2, 5], bad_nd[1, 0], bad_root[3] = MC.P, MC.P, 2**64 - 1
    assert "values[2][5]" in raw(val=bad_val, nd=bad_nd, root=bad_root)
    assert "nodes[1][0]" in raw(nd=bad_nd, root=bad_root)
    assert "root[0][3]" in raw(root=bad_root)


# ---- 5. checkpoints ---------------------------------------------------------------------------------------------------------------------------------
def test_checkpoints_on_a_partial_ledger(backend):
    sc = LS.BY_NAME["bystander_siblings"]
    F, P, opened = _pair(backend, sc)
    cf, cp = F.checkpoint(), P.checkpoint()
    at_checkpoint = F.open(opened)
    for lo, hi in ((0, 2), (2, 4)):
        _same_witness(F.apply(LS.transfers(sc, lo, hi)), P.apply(LS.transfers(sc, lo, hi)))
    _same_openings(F, P, opened)
    _same_openings(F, P, opened, at_f=cf, at_p=cp)
    past = P.open(opened, at=cp)
    assert np.array_equal(past.paths, at_checkpoint.paths) and np.array_equal(past.root, LS.expected(sc).initial_root)
    assert P.audit().consistent == 1 and P.audit(at=cp).consistent == 1
    F.revert(cf)
    P.revert(cp)
    assert np.array_equal(P.root(), LS.expected(sc).initial_root)
    _same_openings(F, P, opened)
    now = P.open(opened)
    assert np.array_equal(now.paths, at_checkpoint.paths) and np.array_equal(now.values, at_checkpoint.values)
    P.release(cp)
    _same_witness(F.apply(LS.transfers(sc)), P.apply(LS.transfers(sc)))
    assert P.audit().consistent == 1 and P.partial_info()[2] == len(MC.proof_positions(7, opened))
    F.close()
    P.close()


# ---- 6. audit -----------------------------------------------------------------------------------------------------------------------------------------
def test_audit_does_not_test_an_opaque_node(backend):
    d = 7
    indices = [10, 11, 20, 40]
    m = _model(d, [10, 20, 21, 77], seed=6)
    P = _from_model(backend, m, indices)
    positions = MC.proof_positions(d, indices)
    assert P.partial_info()[2] == len(positions) == MC.shape(d, indices)[0]
    first = lambda r: (r.first_kind, r.first_level, r.first_index)
    for l, x in (positions[0], positions[len(positions) // 2], positions[-1]):
        # an opaque node: only its parent's test reads it, and the parent is named, never the node
        assert CC.xor_word(P, ("node", l, x), 2) == 0
        r = P.audit()
        assert (r.consistent, r.n_bad, first(r)) == (0, 1, (CC.INNER, l - 1, x >> 1)), (l, x, CC.report_tuple(r))
        assert CC.xor_word(P, ("node", l, x), 2) == 0
        assert P.audit().consistent == 1
    # a node of the fold: itself and its parent, the lower level first
    assert CC.xor_word(P, ("node", d - 1, 5), 4) == 0
    r = P.audit()
    assert (r.consistent, r.n_bad, first(r)) == (0, 2, (CC.INNER, d - 1, 5)), CC.report_tuple(r)
    assert CC.xor_word(P, ("node", d - 1, 5), 4) == 0
    # a stored leaf: its own test and its parent's
    assert CC.xor_word(P, ("node", d, 10), 0) == 0
    r = P.audit()
    assert (r.consistent, r.n_bad, first(r)) == (0, 2, (CC.LEAF, d, 10)), CC.report_tuple(r)
    assert CC.xor_word(P, ("node", d, 10), 0) == 0
    tr = LS.transfer_arrays([(10, 20, 3)])
    P.apply(tr)
    assert not isinstance(m.apply(*tr), tuple)
    r = P.audit()
    assert r.consistent == 1 and np.array_equal(P.root(), m.root()) and P.partial_info()[2] == len(positions)
    P.close()


# ---- 7. the resident witness and proving -------------------------------------------------------------------------------------------------------
def test_from_opening_leaves_a_resident_batch_and_proves_the_same(backend):
    from certificate_stark_amd.prover import Ledger, get_example_options
    w = LC.generated((2, 3, 2))
    backend.upload_witness(w)
    expected = backend.prove(get_example_options())
    indices, values = LC.initial_accounts(w)
    F = Ledger(3, backend)
    F.set_accounts(indices, values)
    assert F.apply(w, want_witness=False) is None          # the batch is resident
    G = Ledger(3, backend)
    G.set_accounts(indices, values)
    P = G.open_multi_for(w).to_ledger()                  # building P between apply and prove: the proof is the proof without it
    assert P.partial and np.array_equal(P.root(), w.initial_roots[0])
    assert backend.prove(get_example_options()) == expected
    # a prover that does not hold the state: the opening, P.apply, prove -- byte for byte the proof after F.apply
    backend.upload_witness(LC.generated((2, 3, 5)))
    assert P.apply(w, want_witness=False) is None
    assert backend.prove(get_example_options()) == expected
    assert np.array_equal(P.root(), w.final_root) and np.array_equal(P.root(), F.root())
    for led in (F, G, P):
        led.close()


# ---- 8. a full and a partial ledger in one context -------------------------------------------------------------------------------------------------
def test_a_full_and_a_partial_ledger_share_a_context(backend):
    a, b = LS.BY_NAME["bystander_siblings"], LS.BY_NAME["pingpong_halves"]
    F, P, opened = _pair(backend, a)
    F2, P2, opened2 = _pair(backend, b)
    for lo in range(4):          # calls interleaved: each ledger answers for itself
        wf = F.apply(LS.transfers(a, lo, lo + 1))
        w2 = P2.apply(LS.transfers(b, 2 * lo, 2 * lo + 2))
        _same_witness(wf, P.apply(LS.transfers(a, lo, lo + 1)))
        _same_witness(F2.apply(LS.transfers(b, 2 * lo, 2 * lo + 2)), w2)
        _same_openings(F, P, opened)
        _same_openings(F2, P2, opened2)
    assert np.array_equal(P.root(), LS.expected(a).final_root) and np.array_equal(P2.root(), LS.expected(b).final_root)
    for led in (F, P, F2, P2):
        assert led.audit().consistent == 1
        led.close()
