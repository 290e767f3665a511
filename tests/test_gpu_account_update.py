"""cstark_account_check_update on the GPU (k_multi_update: both states of a multi-opening folded in one pass) against two plain folds
(update_cases.py on multiproof_cases.fold) and against pairs of plain models (ledger_model.py): no change, one changed account among
many, all changed, accounts created and deleted, compute-only mode, the verdicts OLD_ROOT and NEW_ROOT, INDEX and NODE_COUNT as data,
misuse that launches nothing, the shapes at which the fold can go wrong, every steered scenario through a ledger, a resident witness
left alone.  Every raw output buffer starts as 0xA5 and is compared whole."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC
import ledger_scenarios as LS
import multiproof_cases as MC
import update_cases as UC

pytestmark = pytest.mark.gpu

u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
FILL32 = 0xA5A5A5A5
SPARE = 3


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _ptr(a, typ=u64p):
    return None if a is None else a.ctypes.data_as(typ)


def _u64(a):
    return None if a is None else np.ascontiguousarray(a, np.uint64)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8)


def _error(backend):
    return backend.lib.cstark_last_error().decode()


def _untouched(*buffers):
    return all((a == {1: MC.FILL8, 4: FILL32, 8: MC.FILL64}[a.dtype.itemsize]).all() for a in buffers)


def _call(backend, depth, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root=None, n_nodes=None, count=None,
          null=(), want=True):
    """the C call on 0xA5-filled outputs -> (status, verdict, at, new_root_out, n_changed); new_root_out has spare room"""
    idx, old, new, nd, r_old, r_new = _u64(indices), _u64(old_values), _u64(new_values), _u64(nodes), _u64(old_root), _u64(new_root)
    nd = None if nd is None or nd.size == 0 else nd.reshape(-1, 7)
    was, now = _u8(old_present), _u8(new_present)
    verdict, at, n_changed = (np.full(1, FILL32, np.uint32) for _ in range(3))
    out = np.full(7 + SPARE, MC.FILL64, np.uint64)
    args = [_ptr(idx), _ptr(old), _ptr(was, u8p), _ptr(new), _ptr(now, u8p), _ptr(nd), C.c_uint32((0 if nd is None else len(nd)) if n_nodes is None else n_nodes),
            _ptr(r_old), _ptr(r_new), _ptr(verdict, u32p), _ptr(at, u32p), _ptr(out) if want else None, _ptr(n_changed, u32p) if want else None]
    for k in null:
        args[k] = None
    rc = backend.lib.cstark_account_check_update(backend.ctx, C.c_uint32(depth), C.c_uint32(len(idx) if count is None else count), *args)
    return rc, verdict, at, out, n_changed


def _assert_update(backend, depth, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root=None, expected=None):
    """verdict, at, the new fold and the changed count are the reference's; `expected`: the verdict the case itself states"""
    ref_verdict, ref_at, ref_fold, ref_changed = UC.expected_update(depth, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root)
    if expected is not None:
        assert ref_verdict == expected, "the reference itself disagrees with the case"
    rc, verdict, at, out, n_changed = _call(backend, depth, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root)
    assert rc == 0, _error(backend)
    assert (int(verdict[0]), int(at[0])) == (ref_verdict, ref_at)
    if ref_fold is None:
        assert _untouched(out)
    else:
        assert np.array_equal(out[:7], ref_fold) and _untouched(out[7:])
    assert _untouched(n_changed) if ref_changed is None else int(n_changed[0]) == ref_changed
    return ref_fold


def _assert_pair(backend, old, new, indices, changed):
    """a model pair: the stated transition is VALID, compute-only gives the new model's root, and the way back holds too"""
    indices = np.asarray(indices, np.uint64)
    d = old.depth
    old_values, old_present, new_values, new_present, nodes, old_root, new_root = UC.states(old, new, indices)
    assert UC.n_changed(old_values, old_present, new_values, new_present) == changed
    fold = _assert_update(backend, d, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root, expected=UC.VALID)
    assert np.array_equal(fold, new_root)
    fold = _assert_update(backend, d, indices, old_values, old_present, new_values, new_present, nodes, old_root, expected=UC.VALID)
    assert np.array_equal(fold, new_root)
    fold = _assert_update(backend, d, indices, new_values, new_present, old_values, old_present, nodes, new_root, old_root, expected=UC.VALID)
    assert np.array_equal(fold, old_root)
    if changed:
        assert not np.array_equal(old_root, new_root)
        _assert_update(backend, d, indices, old_values, old_present, new_values, new_present, nodes, old_root, old_root, expected=UC.NEW_ROOT)
        _assert_update(backend, d, indices, old_values, old_present, new_values, new_present, nodes, new_root, new_root, expected=UC.OLD_ROOT)
    else:
        assert np.array_equal(old_root, new_root)


# ---- 1. what can change --------------------------------------------------------------------------------------------------------------------
MANY = [3, 8, 9, 10, 11, 20, 21, 22, 40, 41, 64, 100, 126, 127]        # depth 7: pairs, singles, both ends of a subtree


@pytest.mark.parametrize("name,change,create,delete", [
    ("no_change", [], [], []),
    ("one_changed_among_many", [21], [], []),
    ("the_first_and_the_last", [3, 127], [], []),
    ("all_changed", [i for i in MANY if i % 4], [i for i in MANY if i % 4 == 0][:2], [i for i in MANY if i % 4 == 0][2:]),
    ("absent_to_present", [], [8, 64], []),
    ("present_to_absent", [], [], [9, 126]),
    ("created_deleted_changed", [10], [40], [41]),
])
def test_what_can_change(backend, name, change, create, delete):
    # 3 and 11 are absent unless named; 5 and 77 are accounts nobody opens
    have = [i for i in MANY if i in change or i in delete or (i not in (3, 11) and i not in create)] + [5, 77]
    old, new = UC.model_pair(7, have, MANY, change, create, delete, seed=len(name))
    changed = len(change) + len(create) + len(delete)
    if name == "all_changed":
        assert changed == len(MANY)
    _assert_pair(backend, old, new, MANY, changed)


def test_value_words_of_two_absent_positions_do_not_count(backend):
    old, new = UC.model_pair(7, [8, 9, 127], MANY, [9])
    old_values, old_present, new_values, new_present, nodes, old_root, new_root = UC.states(old, new, MANY)
    k = MANY.index(40)
    assert not old_present[k] and not new_present[k]
    new_values = new_values.copy()
    new_values[k, 5] = 12345
    rc, verdict, at, out, n_changed = _call(backend, 7, MANY, old_values, old_present, new_values, new_present, nodes, old_root, new_root)
    assert rc == 0 and (int(verdict[0]), int(at[0]), int(n_changed[0])) == (UC.VALID, 0, 1) and np.array_equal(out[:7], new_root)
    # all present (null flags): the zero values of the absent positions are hashed on both sides, and the opening no longer folds
    rc, verdict, *_ = _call(backend, 7, MANY, old_values, None, new_values, None, nodes, old_root, new_root)
    assert rc == 0 and int(verdict[0]) == UC.OLD_ROOT


# ---- 2. the shapes at which the fold can go wrong ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,indices", [
    ("depth_1_one_leaf", 1, [1]),
    ("depth_1_both", 1, [0, 1]),
    ("depth_3_all_leaves", 3, list(range(8))),
    ("depth_2", 2, [1, 2]),
    ("ends_meet_at_the_root", 3, [0, 7]),
    ("unaligned_run_of_64", 7, list(range(33, 97))),
])
def test_structures_of_a_level(backend, name, depth, indices):
    size = 1 << depth
    have = sorted(set([0, size - 1, indices[0], indices[-1]]))
    change = [i for i in have if i in indices][:1]
    create = [i for i in indices if i not in have][:1]
    delete = [i for i in have if i in indices and i not in change][:1]
    old, new = UC.model_pair(depth, have, indices, change, create, delete, seed=depth)
    if name == "depth_3_all_leaves":
        assert len(UC.states(old, new, indices)[4]) == 0
    _assert_pair(backend, old, new, indices, len(change) + len(create) + len(delete))
    _assert_pair(backend, old, old, indices, 0)


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 8, 9])
def test_counts_around_a_wave(backend, count):
    """a wave carries two jobs of two sides: counts around two and four, with `count` nodes on levels 7, 6, 5 and 4"""
    indices = [8 * k + (k % 2) for k in range(count)]
    have = indices[::2] + [127]
    for change in ([indices[-1]] if indices[-1] in have else [], [i for i in indices if i in have]):
        create = [i for i in indices if i not in have][-1:]
        old, new = UC.model_pair(7, have, indices, change, create, seed=count)
        _assert_pair(backend, old, new, indices, len(change) + len(create))


def test_depth_31_above_2_to_the_24(backend):
    have = [2**24 + 1, 2**30 + 3, 2**30 + 2**24, 2**30 + 2**24 + 1, 2**31 - 2]
    indices = sorted(have + [2**30 + 2, 2**31 - 1, 2**24])
    assert all(i >= 2**24 for i in indices)
    old, new = UC.model_pair(31, have, indices, [2**30 + 3, 2**31 - 2], [2**31 - 1], [2**24 + 1], seed=31)
    _assert_pair(backend, old, new, indices, 4)


# ---- 3. the verdicts, each against the reference ------------------------------------------------------------------------------------------------
def test_tampered_updates(backend):
    d = 7
    old, new = UC.model_pair(d, [8, 9, 10, 20, 127], MANY, [10, 127], [40], [9], seed=3)
    indices = np.array(MANY, np.uint64)
    old_values, old_present, new_values, new_present, nodes, old_root, new_root = UC.states(old, new, indices)
    assert len(nodes) >= 4

    def case(expected, indices=indices, old_values=old_values, old_present=old_present, new_values=new_values, new_present=new_present, nodes=nodes,
             old_root=old_root, new_root=new_root):
        return _assert_update(backend, d, indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root, expected=expected)

    def bumped(a, *where):
        a = a.copy()
        a[where] = MC.bump(a[where])
        return a

    case(UC.VALID)
    # OLD_ROOT: nothing is said about the new side, new_root_out stays as it was (asserted by _assert_update)
    case(UC.OLD_ROOT, nodes=bumped(nodes, 0, 0))
    case(UC.OLD_ROOT, nodes=bumped(nodes, len(nodes) - 1, 6))
    case(UC.OLD_ROOT, nodes=bumped(nodes, 1, 3), new_root=None)
    case(UC.OLD_ROOT, old_values=bumped(old_values, MANY.index(8), 12))
    case(UC.OLD_ROOT, old_root=bumped(old_root, 4))
    flipped = old_present.copy()
    flipped[MANY.index(11)] ^= 1
    case(UC.OLD_ROOT, old_present=flipped)
    case(UC.OLD_ROOT, old_root=bumped(old_root, 0), new_root=bumped(new_root, 0))        # the first that applies
    # NEW_ROOT: new_root_out is the true fold of the new values
    assert np.array_equal(case(UC.NEW_ROOT, new_root=bumped(new_root, 3)), new_root)
    fold = case(UC.NEW_ROOT, new_values=bumped(new_values, MANY.index(10), 13))
    assert not np.array_equal(fold, new_root)
    fold = case(UC.NEW_ROOT, new_values=bumped(new_values, MANY.index(20), 0))         # an account the claim says is unchanged
    assert not np.array_equal(fold, new_root)
    flipped = new_present.copy()
    flipped[MANY.index(40)] ^= 1
    case(UC.NEW_ROOT, new_present=flipped)
    # the shape is data: NODE_COUNT, at = the need, whatever else is wrong
    case(UC.NODE_COUNT, nodes=nodes[:-1])
    case(UC.NODE_COUNT, nodes=nodes[1:], old_root=bumped(old_root, 0))
    case(UC.NODE_COUNT, nodes=np.concatenate([nodes, nodes[:1]]))
    case(UC.NODE_COUNT, nodes=None)
    assert UC.expected_update(d, indices, old_values, old_present, new_values, new_present, nodes[:-1], old_root, new_root)[:2] == (UC.NODE_COUNT, len(nodes))
    # INDEX, at = the position, ahead of NODE_COUNT and the roots
    order = np.arange(len(indices))
    order[[2, 3]] = [3, 2]
    for bad, at in ((indices[order], 3), (np.append(indices[:-1], np.uint64(128)), len(indices) - 1), (np.append(indices[:-1], indices[-2]), len(indices) - 1)):
        assert UC.expected_update(d, bad, old_values, old_present, new_values, new_present, nodes, old_root, new_root)[:2] == (UC.INDEX, at)
        case(UC.INDEX, indices=bad)
        case(UC.INDEX, indices=bad, nodes=nodes[:-1], old_root=bumped(old_root, 0))
    # a valid update after all of them: nothing stale is left in the context's block
    case(UC.VALID)
    case(UC.VALID, new_root=None)


def test_misuse_leaves_the_outputs(backend):
    old, new = UC.model_pair(3, [1, 6], [1, 2, 6], [6], [2], seed=8)
    indices = np.array([1, 2, 6], np.uint64)
    old_values, old_present, new_values, new_present, nodes, old_root, new_root = UC.states(old, new, indices)
    assert len(nodes) == 4
    good = (indices, old_values, old_present, new_values, new_present, nodes, old_root, new_root)

    def refused(*args, depth=3, **kw):
        rc, *outputs = _call(backend, depth, *args, **kw)
        assert rc == -1 and _untouched(*outputs)
        return _error(backend)

    _assert_update(backend, 3, *good, expected=UC.VALID)
    for null in (0, 1, 3, 7, 9, 10):        # indices, old_values, new_values, old_root, verdict, at
        refused(*good, null=(null,))
    refused(*good, null=(5,))               # nodes null with n_nodes = 4
    refused(*good, n_nodes=0)               # nodes given with n_nodes = 0
    refused(*good, count=0)
    refused(*good, count=(1 << 20) + 1)
    assert "depth" in refused(*good, depth=0) and "depth" in refused(*good, depth=32)

    def with_bad(k, *where, value=MC.P):
        args = [a.copy() for a in good]
        args[k][where] = value
        return args

    assert "old_values[1][13]" in refused(*with_bad(1, 1, 13))
    assert "new_values[2][0]" in refused(*with_bad(3, 2, 0, value=2**64 - 1))
    assert "nodes[3][2]" in refused(*with_bad(5, 3, 2))
    assert "old_root[0][5]" in refused(*with_bad(6, 5))
    assert "new_root[0][6]" in refused(*with_bad(7, 6))
    # the order of the scan: old values, new values, nodes, old root, new root
    bad = with_bad(7, 6)
    for k, where, named in ((6, (5,), "old_root[0][5]"), (5, (3, 2), "nodes[3][2]"), (3, (2, 0), "new_values[2][0]"), (1, (1, 13), "old_values[1][13]")):
        bad[k][where] = MC.P
        assert named in refused(*bad)
    # a word that is no field element is misuse even where the shape would be a verdict
    assert "nodes[3][2]" in refused(indices[::-1].copy(), *with_bad(5, 3, 2)[1:])
    # null outputs, null flags and a null new root are no misuse
    rc, verdict, at, out, n_changed = _call(backend, 3, *good, want=False)
    assert rc == 0 and (int(verdict[0]), int(at[0])) == (UC.VALID, 0) and _untouched(out, n_changed)
    rc, verdict, at, out, n_changed = _call(backend, 3, *good[:7])
    assert rc == 0 and int(verdict[0]) == UC.VALID and np.array_equal(out[:7], new_root) and int(n_changed[0]) == 2


# ---- 4. through a ledger: the root a batch leads to, from the opening before it and the accounts after it ----------------------------------------
@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_the_root_a_batch_leads_to(backend, sc):
    from certificate_stark_amd.prover import Ledger, UpdateCheck
    led = Ledger(sc.depth, backend)
    led.set_accounts(sc.indices(), LS.values(sc))
    opening = led.open_multi(MC.opened(sc))
    led.apply(LS.transfers(sc))
    values, present = led.accounts(opening.indices)
    final_root = led.root()
    led.close()
    assert np.array_equal(final_root, LS.expected(sc).final_root)
    got = opening.check_update(values, present, final_root)
    ref = UC.expected_update(sc.depth, opening.indices, opening.values, opening.present, values, present, opening.nodes, opening.root, final_root)
    assert isinstance(got, UpdateCheck) and (got.verdict, got.at, got.n_changed) == (UC.VALID, 0, ref[3]) == ref[:2] + (ref[3],)
    assert np.array_equal(got.new_root, final_root) and np.array_equal(ref[2], final_root)
    computed = opening.check_update(values, present)
    assert computed.verdict == UC.VALID and np.array_equal(computed.new_root, final_root)
    stale = opening.check_update(values, present, opening.root)
    assert stale.verdict == (UC.NEW_ROOT if ref[3] else UC.VALID) and np.array_equal(stale.new_root, final_root)


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=lambda sc: sc.name)
def test_open_multi_for_opens_what_a_batch_reads(backend, sc):
    """the opening of a batch's senders and receivers, and nothing else, is enough to follow the batch to its root"""
    from certificate_stark_amd.prover import Ledger
    led = Ledger(sc.depth, backend)
    led.set_accounts(sc.indices(), LS.values(sc))
    opening = led.open_multi_for(LS.transfers(sc))
    named = sorted(set(i for s, r, _ in sc.transfers for i in (s, r)))
    assert [int(i) for i in opening.indices] == named and opening.present.all()
    same = led.open_multi_for(LS.expected(sc).witness)              # an object with s_indices and r_indices
    assert np.array_equal(same.indices, opening.indices) and np.array_equal(same.nodes, opening.nodes)
    m = LS.model(sc)
    assert np.array_equal(opening.nodes, MC.nodes_from_model(m, opening.indices)) and np.array_equal(opening.root, m.root())
    led.apply(LS.transfers(sc))
    got = opening.check_update(*led.accounts(opening.indices), new_root=led.root())
    led.close()
    assert got.verdict == UC.VALID and np.array_equal(got.new_root, LS.expected(sc).final_root)


# ---- 5. the resident witness ----------------------------------------------------------------------------------------------------------------------
def test_check_update_leaves_a_resident_batch(backend):
    """a batch resident from apply(want_witness=False): update checks between apply and prove, and the proof is the proof without them"""
    from certificate_stark_amd.prover import Ledger, get_example_options
    w = LC.generated((2, 3, 2))
    backend.upload_witness(w)
    expected = backend.prove(get_example_options())
    indices, values = LC.initial_accounts(w)
    led = Ledger(3, backend)
    led.set_accounts(indices, values)
    before = led.open_multi(np.arange(8, dtype=np.uint64))
    assert led.apply(w, want_witness=False) is None
    after_values, after_present = led.accounts(before.indices)
    got = before.check_update(after_values, after_present, w.final_root)
    assert got.verdict == UC.VALID and got.n_changed >= 2 and np.array_equal(got.new_root, w.final_root)
    some = led.open_multi(indices[:2])
    assert some.check().verdict == MC.VALID and some.check_update(some.values, some.present, some.root).n_changed == 0
    assert backend.prove(get_example_options()) == expected
    led.close()


# ---- 6. the Python layers -----------------------------------------------------------------------------------------------------------------------
def test_python_layers(backend):
    from certificate_stark_amd.prover import UpdateCheck, check_account_update
    old, new = UC.model_pair(7, [8, 9, 127], MANY, [9], [64], seed=6)
    old_values, old_present, new_values, new_present, nodes, old_root, new_root = UC.states(old, new, MANY)
    got = check_account_update(7, MANY, old_values, new_values, nodes, old_root, new_root, old_present, new_present, backend=backend)
    assert isinstance(got, UpdateCheck) and (got.verdict, got.at, got.n_changed) == (backend.UPDATE_VALID, 0, 2) and np.array_equal(got.new_root, new_root)
    assert (backend.UPDATE_VALID, backend.UPDATE_INDEX, backend.UPDATE_NODE_COUNT, backend.UPDATE_OLD_ROOT, backend.UPDATE_NEW_ROOT) == (0, 1, 2, 3, 4)
    short = check_account_update(7, MANY, old_values, new_values, nodes[:-1], old_root, new_root, old_present, new_present, backend=backend)
    assert tuple(short) == (backend.UPDATE_NODE_COUNT, len(nodes), None, None)
    unsorted = check_account_update(7, MANY[::-1], old_values, new_values, nodes, old_root, new_root, old_present, new_present, backend=backend)
    assert tuple(unsorted) == (backend.UPDATE_INDEX, 1, None, None)
    wrong = check_account_update(7, MANY, old_values, new_values, nodes, new_root, new_root, old_present, new_present, backend=backend)
    assert (wrong.verdict, wrong.new_root, wrong.n_changed) == (backend.UPDATE_OLD_ROOT, None, 2)
    with pytest.raises(ValueError):
        backend.account_check_update(7, MANY, old_values[:2], new_values, nodes, old_root)
    with pytest.raises(ValueError):
        backend.account_check_update(7, MANY, old_values, new_values, nodes, old_root, new_present=new_present[:3])
