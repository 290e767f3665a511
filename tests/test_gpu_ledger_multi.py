"""The ledger's multi-openings on the GPU: cstark_ledger_open_multi (prover.Ledger.open_multi) against the plain model (ledger_model.py)
and cstark_account_check_multiproof against the plain fold (multiproof_cases.py).  Multi-openings of every steered scenario before and
after its batch, entry by entry against the paths Ledger.open gives; depth 31 above 2^24; counts around the four hashes of a workgroup;
the structures a level can have; checkpoints; tampered proofs; misuse that launches nothing; a resident witness left alone.  Every raw
output buffer starts as 0xA5 and is compared whole."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import ledger_scenarios as LS
import multiproof_cases as MC

pytestmark = pytest.mark.gpu

u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
FILL32 = 0xA5A5A5A5
SPARE = 3
_ids = lambda sc: sc.name


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _ledger(backend, sc):
    from certificate_stark_amd.prover import Ledger
    led = Ledger(sc.depth, backend)
    led.set_accounts(sc.indices(), LS.values(sc))
    return led


def _ptr(a, typ=u64p):
    return None if a is None else a.ctypes.data_as(typ)


def _u64(a):
    return None if a is None else np.ascontiguousarray(a, np.uint64)


def _error(backend):
    return backend.lib.cstark_last_error().decode()


def _untouched(*buffers):
    return all((a == {1: MC.FILL8, 4: FILL32, 8: MC.FILL64}[a.dtype.itemsize]).all() for a in buffers)


# ---- the two C calls on 0xA5-filled outputs --------------------------------------------------------------------------------------------
def _open(backend, led, indices, capacity, cp=0, count=None, null=None, ctx=None):
    """-> (status, values, present, nodes, n_nodes, root): whole buffers, SPARE rows longer than the call may fill"""
    idx = _u64(indices)
    n = len(idx)
    values = np.full((n + SPARE, 14), MC.FILL64, np.uint64)
    present = np.full(n + SPARE, MC.FILL8, np.uint8)
    nodes = np.full((capacity + SPARE, 7), MC.FILL64, np.uint64)
    n_nodes = np.full(1, FILL32, np.uint32)
    root = np.full(7 + SPARE, MC.FILL64, np.uint64)
    args = [_ptr(idx), _ptr(values), _ptr(present, u8p), _ptr(nodes), C.c_uint32(capacity), _ptr(n_nodes, u32p), _ptr(root)]
    if null is not None:
        args[null] = None
    rc = backend.lib.cstark_ledger_open_multi(ctx or backend.ctx, led._led, C.c_uint64(cp), C.c_uint32(n if count is None else count), *args)
    return rc, values, present, nodes, n_nodes, root


def _check(backend, depth, indices, nodes, root, values=None, present=None, leaves=None, n_nodes=None, count=None, null=(), want=True):
    """-> (status, verdict, at, root_out, n_merges): 0xA5-filled words and a root_out with spare room"""
    idx, nd, r, v, lv = _u64(indices), _u64(nodes), _u64(root), _u64(values), _u64(leaves)
    nd = None if nd is None or nd.size == 0 else nd.reshape(-1, 7)
    pr = None if present is None else np.ascontiguousarray(present, np.uint8)
    verdict, at, n_merges = (np.full(1, FILL32, np.uint32) for _ in range(3))
    out = np.full(7 + SPARE, MC.FILL64, np.uint64)
    args = [_ptr(idx), _ptr(v), _ptr(pr, u8p), _ptr(lv), _ptr(nd), C.c_uint32((0 if nd is None else len(nd)) if n_nodes is None else n_nodes), _ptr(r),
            _ptr(verdict, u32p), _ptr(at, u32p), _ptr(out) if want else None, _ptr(n_merges, u32p) if want else None]
    for k in null:
        args[k] = None
    rc = backend.lib.cstark_account_check_multiproof(backend.ctx, C.c_uint32(depth), C.c_uint32(len(idx) if count is None else count), *args)
    return rc, verdict, at, out, n_merges


def _assert_check(backend, depth, indices, nodes, root, values=None, present=None, leaves=None, expected=None):
    """verdict, at, folded root and merge count are the reference's; `expected`: the verdict the case itself states"""
    ref_verdict, ref_at, ref_root, ref_merges = MC.expected_verdict(depth, indices, nodes, root, values, present, leaves)
    if expected is not None:
        assert ref_verdict == expected, "the reference itself disagrees with the case"
    rc, verdict, at, out, n_merges = _check(backend, depth, indices, nodes, root, values, present, leaves)
    assert rc == 0, _error(backend)
    assert (int(verdict[0]), int(at[0])) == (ref_verdict, ref_at)
    if ref_root is None:
        assert _untouched(out)
    else:
        assert np.array_equal(out[:7], ref_root) and _untouched(out[7:])
    assert _untouched(n_merges) if ref_merges is None else int(n_merges[0]) == ref_merges
    return ref_verdict


def _model_proof(m, indices):
    """(nodes, values, present, leaves, root) of the model for the ascending indices"""
    values, present = MC.accounts_from_model(m, indices)
    return MC.nodes_from_model(m, indices), values, present, MC.leaves_from_model(m, indices), m.root()


def _assert_model_proof_verifies(backend, m, indices):
    nodes, values, present, leaves, root = _model_proof(m, indices)
    _assert_check(backend, m.depth, indices, nodes, root, values, present, expected=MC.VALID)
    _assert_check(backend, m.depth, indices, nodes, root, leaves=leaves, expected=MC.VALID)


# ---- 1. every scenario, through Ledger.open_multi and .check() ---------------------------------------------------------------------------
def _assert_opening(backend, led, m, asked, at=None):
    from certificate_stark_amd.prover import AccountMultiOpening
    d = m.depth
    o = led.open_multi(asked, at=at)
    indices = np.array(sorted(set(int(i) for i in asked)), np.uint64)
    assert isinstance(o, AccountMultiOpening) and o.depth == d and np.array_equal(o.indices, indices)
    assert np.array_equal(o.indices[o.inverse], np.asarray(asked, np.uint64))
    nodes, values, present, _, root = _model_proof(m, indices)
    assert o.nodes.shape == nodes.shape and np.array_equal(o.nodes, nodes)
    assert np.array_equal(o.values, values) and np.array_equal(o.present, present.astype(bool)) and np.array_equal(o.root, root)
    assert o.nbytes == 8 * len(indices) + 112 * len(indices) + len(indices) + 56 * len(nodes) + 56
    ref = MC.expected_verdict(d, indices, nodes, root, values, present)
    got = o.check()
    assert (got.verdict, got.at, got.n_merges) == (MC.VALID, 0, ref[3]) == ref[:2] + (MC.shape(d, indices)[1],)
    assert np.array_equal(got.root, ref[2]) and np.array_equal(got.root, root)
    return o


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=_ids)
def test_open_multi_reproduces_the_model(backend, sc):
    asked, d = MC.interesting_indices(sc), sc.depth
    assert len(set(asked.tolist())) < len(asked)
    led, m = _ledger(backend, sc), LS.model(sc)
    for when in ("before", "after"):
        o = _assert_opening(backend, led, m, asked)
        # entry by entry what the existing path opening gives: node (l, y) is entry d - l + 1 of the path of an opened index under y ^ 1
        paths = led.open(o.indices)
        assert np.array_equal(paths.root, o.root) and np.array_equal(paths.values, o.values) and np.array_equal(paths.present, o.present)
        for (l, y), digest in zip(MC.proof_positions(d, o.indices), o.nodes):
            under = [k for k, i in enumerate(o.indices) if int(i) >> (d - l) == y ^ 1]
            assert under and all(np.array_equal(paths.paths[k, d - l + 1], digest) for k in under), (when, l, y)
        if when == "before":
            led.apply(LS.transfers(sc))
            assert not isinstance(m.apply(*LS.transfers(sc)), tuple)
    assert np.array_equal(led.root(), LS.expected(sc).final_root)
    led.close()


# ---- 2. depth 31: accounts above 2^24 and with bit 30 set --------------------------------------------------------------------------------
def test_depth_31_above_2_to_the_24(backend):
    from certificate_stark_amd.prover import Ledger
    have = [2**24 + 1, 2**30 + 3, 2**30 + 2**24, 2**30 + 2**24 + 1, 2**31 - 2]
    values = LS.account_values([(LS.B + k, k) for k in range(len(have))], seed=31)
    m, led = LM.LedgerModel(31), Ledger(31, backend)
    m.set_accounts(have, values)
    led.set_accounts(np.array(have, np.uint64), values)
    asked = np.array(have + [2**30 + 2, 2**31 - 1, 2**24], np.uint64)
    assert all(int(i) >= 2**24 for i in asked) and sum(1 for i in asked if int(i) >> 30 & 1) >= 5
    o = _assert_opening(backend, led, m, asked)
    assert list(o.present) == [False, True, False, True, True, True, True, False]
    led.close()
    _assert_model_proof_verifies(backend, m, o.indices)


# ---- 3. counts around the four hashes of a workgroup, at the leaf level and above ----------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 5, 8, 9])
def test_counts_around_a_workgroup(backend, count):
    d = 7
    indices = np.array([8 * k + (k % 2) for k in range(count)], np.uint64)     # apart by 8: levels 7, 6, 5 and 4 all hold `count` nodes
    known = set(int(i) for i in indices)
    for _ in range(3):
        known = set(x >> 1 for x in known)
        assert len(known) == count
    m = LM.LedgerModel(d)
    have = [int(i) for i in indices[::2]] + [127]
    m.set_accounts(have, LS.account_values([(LS.B, k) for k in range(len(have))], seed=count))
    _assert_model_proof_verifies(backend, m, indices)


# ---- 4. the structures a level can have ---------------------------------------------------------------------------------------------------
def _small_model(depth, have, seed):
    m = LM.LedgerModel(depth)
    m.set_accounts(have, LS.account_values([(LS.B + i, i) for i in range(len(have))], seed=seed))
    return m


@pytest.mark.parametrize("name,depth,indices,positions", [
    # level 2: node 0 is computed and its right sibling comes from the proof; node 3 is computed and its LEFT sibling comes from the proof
    ("computed_left_and_computed_right", 3, [0, 1, 6, 7], [(2, 1), (2, 2)]),
    # level 2: both children of node (1, 0) are computed
    ("both_children_computed", 3, [0, 1, 2, 3], [(1, 1)]),
    ("ends_meet_at_the_root", 3, [0, 7], [(3, 1), (3, 6), (2, 1), (2, 2)]),
    ("all_leaves", 3, list(range(8)), []),
    ("aligned_run_of_64", 7, list(range(64, 128)), [(1, 0)]),
    ("unaligned_run_of_64", 7, list(range(33, 97)), None),
    ("depth_2", 2, [1, 2], [(2, 0), (2, 3)]),
    ("depth_1_one_leaf", 1, [1], [(1, 0)]),
    ("depth_1_both", 1, [0, 1], []),
])
def test_structures_of_a_level(backend, name, depth, indices, positions):
    indices = np.array(indices, np.uint64)
    if positions is not None:
        assert MC.proof_positions(depth, indices) == positions
    size = 1 << depth
    m = _small_model(depth, sorted(set([0, size - 1, size // 2, int(indices[0]), int(indices[-1])])), seed=depth)
    nodes, values, present, leaves, root = _model_proof(m, indices)
    _assert_model_proof_verifies(backend, m, indices)
    if name == "all_leaves":
        assert len(nodes) == 0
        got = backend.account_check_multiproof(depth, indices, None, root, values=values, present=present)
        assert got[0] == MC.VALID and np.array_equal(got[2], root) and got[3] == 7
    if name == "aligned_run_of_64":
        assert MC.shape(depth, indices) == (1, 64)


# ---- 5. checkpoints ---------------------------------------------------------------------------------------------------------------------------
def test_open_multi_under_a_past_root(backend):
    sc = LS.BY_NAME["bystander_siblings"]
    led, m = _ledger(backend, sc), LS.model(sc)
    old, cp = m.copy(), led.checkpoint()
    later = 12
    assert later not in sc.accounts
    for lo, hi in ((0, 2), (2, 4)):
        led.apply(LS.transfers(sc, lo, hi))
        assert not isinstance(m.apply(*LS.transfers(sc, lo, hi)), tuple)
        if lo == 0:
            fresh = LS.account_values([(77, 7)], seed=5)
            led.set_accounts(np.array([later], np.uint64), fresh)
            m.set_accounts([later], fresh)
    asked = np.array([10, later, 21, 11, 127, 13], np.uint64)
    past = _assert_opening(backend, led, old, asked, at=cp)
    now = _assert_opening(backend, led, m, asked)
    assert np.array_equal(past.root, LS.expected(sc).initial_root) and not np.array_equal(past.root, now.root)
    k = list(past.indices).index(later)
    assert not past.present[k] and now.present[k] and not past.values[k].any()
    assert not np.array_equal(past.values[list(past.indices).index(10)], now.values[list(now.indices).index(10)])
    led.close()


# ---- 6. tampering, each against the reference ----------------------------------------------------------------------------------------------------
def test_tampered_multiproofs(backend):
    sc = LS.BY_NAME["bystander_siblings"]
    d = sc.depth
    led = _ledger(backend, sc)
    o = led.open_multi([8, 10, 12, 20, 127])
    led.close()
    indices, nodes, root, values, present = o.indices, o.nodes, o.root, o.values, o.present.astype(np.uint8)
    assert list(present) == [1, 1, 0, 1, 1] and len(nodes) >= 4
    leaves = MC.leaves_of(values, present)

    def case(expected, indices=indices, nodes=nodes, root=root, values=values, present=present, leaves=None):
        if leaves is not None:
            values = present = None
        assert _assert_check(backend, d, indices, nodes, root, values, present, leaves, expected=expected) == expected

    def bumped(a, *where):
        a = a.copy()
        a[where] = MC.bump(a[where])
        return a

    case(MC.VALID)
    case(MC.VALID, leaves=leaves)
    case(MC.ROOT, nodes=bumped(nodes, 0, 0))
    case(MC.ROOT, nodes=bumped(nodes, len(nodes) - 1, 6))
    case(MC.ROOT, values=bumped(values, 1, 12))
    case(MC.ROOT, values=bumped(values, 4, 0))
    for k in (1, 2):        # an account said to be absent, an absent one said to be present
        flipped = present.copy()
        flipped[k] ^= 1
        case(MC.ROOT, present=flipped)
    swapped = nodes.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert not np.array_equal(swapped, nodes)
    case(MC.ROOT, nodes=swapped)
    case(MC.ROOT, root=bumped(root, 3))
    # one node dropped, one added: NODE_COUNT, at = the need, whatever else is wrong
    case(MC.NODE_COUNT, nodes=nodes[:-1])
    case(MC.NODE_COUNT, nodes=nodes[1:], root=bumped(root, 0))
    case(MC.NODE_COUNT, nodes=np.concatenate([nodes, nodes[:1]]))
    case(MC.NODE_COUNT, nodes=None)
    assert MC.expected_verdict(d, indices, nodes[:-1], root, values, present)[1] == len(nodes)
    # the order of the indices is data too: INDEX, at = the position, ahead of NODE_COUNT and ROOT
    for bad, at in ((indices[[0, 2, 1, 3, 4]], 2), (indices[[0, 1, 1, 3, 4]], 2), (np.append(indices[:4], np.uint64(128)), 4),
                    (np.append(indices[:4], np.uint64(2**64 - 1)), 4), (indices[[1, 0, 2, 3, 4]], 1)):
        assert MC.expected_verdict(d, bad, nodes, root, values, present)[:2] == (MC.INDEX, at)
        case(MC.INDEX, indices=bad)
        case(MC.INDEX, indices=bad, nodes=nodes[:-1], root=bumped(root, 0))
    # digest mode: the stated leaves are the leaves
    case(MC.ROOT, leaves=bumped(leaves, 0, 0))
    case(MC.ROOT, leaves=bumped(leaves, 2, 5))      # the absent account's all-zero leaf
    # a valid proof after all of them: nothing stale is left in the context's block
    case(MC.VALID)


def test_an_opening_goes_stale_with_the_root(backend):
    sc = LS.BY_NAME["pingpong_halves"]
    led = _ledger(backend, sc)
    old = led.open_multi([0, sc.bystanders()[0]])
    led.apply(LS.transfers(sc))
    new_root = led.root()
    led.close()
    assert old.check().verdict == MC.VALID
    _assert_check(backend, 3, old.indices, old.nodes, new_root, old.values, old.present.astype(np.uint8), expected=MC.ROOT)


# ---- 7. misuse launches nothing and leaves the outputs ------------------------------------------------------------------------------------------
def test_check_misuse_leaves_the_outputs(backend):
    m = _small_model(3, [1, 6], seed=8)
    indices = np.array([1, 2, 6], np.uint64)
    nodes, values, present, leaves, root = _model_proof(m, indices)
    assert len(nodes) == 4

    def refused(*args, **kw):
        rc, *outputs = _check(backend, 3, *args, **kw)
        assert rc == -1 and _untouched(*outputs)
        return _error(backend)

    _assert_check(backend, 3, indices, nodes, root, values, present, expected=MC.VALID)
    assert "exactly one" in refused(indices, nodes, root, values, present, leaves)
    assert "exactly one" in refused(indices, nodes, root)
    assert "present without values" in refused(indices, nodes, root, None, present, leaves)
    refused(indices, nodes, root, values, present, null=(0,))       # indices
    refused(indices, nodes, root, values, present, null=(6,))       # root
    refused(indices, nodes, root, values, present, null=(7,))       # verdict
    refused(indices, nodes, root, values, present, null=(8,))       # at
    refused(indices, nodes, root, values, present, null=(4,))       # nodes null with n_nodes = 4
    refused(indices, nodes, root, values, present, n_nodes=0)       # nodes given with n_nodes = 0
    refused(indices, nodes, root, values, present, count=0)
    refused(indices, nodes, root, values, present, count=(1 << 20) + 1)
    for depth in (0, 32):
        rc, *outputs = _check(backend, depth, indices, nodes, root, values, present)
        assert rc == -1 and _untouched(*outputs)
    bad = values.copy()
    bad[1, 13] = MC.P
    bad[2, 0] = MC.P
    assert "values[1][13]" in refused(indices, nodes, root, bad, present)
    bad = leaves.copy()
    bad[2, 6] = 2**64 - 1
    assert "leaves[2][6]" in refused(indices, nodes, root, leaves=bad)
    bad = nodes.copy()
    bad[3, 2] = MC.P
    assert "nodes[3][2]" in refused(indices, bad, root, values, present)
    assert "nodes[3][2]" in refused(indices, bad, root, leaves=leaves)
    bad_root = root.copy()
    bad_root[5] = MC.P
    assert "root[0][5]" in refused(indices, nodes, bad_root, values, present)
    # values are named before nodes, nodes before the root
    assert "nodes[3][2]" in refused(indices, bad, bad_root, values, present)
    # a word that is no field element is misuse even where the shape would be a verdict
    assert "nodes[3][2]" in refused(indices[::-1].copy(), bad, root, values, present)
    # a null root_out, a null n_merges and a null present are no misuse
    rc, verdict, at, out, n_merges = _check(backend, 3, indices, nodes, root, values, present, want=False)
    assert rc == 0 and (int(verdict[0]), int(at[0])) == (MC.VALID, 0) and _untouched(out, n_merges)
    rc, verdict, *_ = _check(backend, 3, indices, nodes, root, values)      # all present: index 2 holds no account
    assert rc == 0 and int(verdict[0]) == MC.ROOT


def test_shape_call(backend):
    lib = backend.lib

    def shape(depth, indices, count=None):
        idx = np.ascontiguousarray(indices, np.uint64)
        out = np.full(2, FILL32, np.uint32)
        rc = lib.cstark_account_multiproof_shape(C.c_uint32(depth), C.c_uint32(len(idx) if count is None else count), _ptr(idx),
                                                 _ptr(out[:1], u32p), _ptr(out[1:], u32p))
        return rc, out

    for depth, indices in ((3, [0, 7]), (3, list(range(8))), (7, list(range(33, 97))), (31, [0, 2**24 + 1, 2**31 - 1]), (1, [1])):
        rc, out = shape(depth, indices)
        assert rc == 0 and tuple(int(x) for x in out) == MC.shape(depth, indices) == backend.account_multiproof_shape(depth, indices)
    for depth, indices, count, named in ((3, [0, 8], None, "indices[1]"), (3, [2, 2], None, "indices[1]"), (3, [0, 5, 4], None, "indices[2]"),
                                         (0, [0], None, "depth"), (32, [0], None, "depth"), (3, [0], 0, "count"), (3, [0], (1 << 20) + 1, "count")):
        rc, out = shape(depth, indices, count)
        assert rc == -1 and _untouched(out) and named in _error(backend)


def test_open_misuse_leaves_the_outputs(backend):
    from certificate_stark_amd.backend import Backend
    sc = LS.BY_NAME["pingpong_halves"]
    led, m = _ledger(backend, sc), LS.model(sc)
    root = led.root()
    good = np.array([0, 5, 7], np.uint64)
    need = MC.shape(3, good)[0]
    assert need == 4

    def refused(indices, capacity=need, **kw):
        rc, *buffers = _open(backend, led, indices, capacity, **kw)
        assert rc == -1 and _untouched(*buffers)
        return _error(backend)

    assert "indices[1]" in refused(np.array([5, 0, 7], np.uint64))        # unsorted
    assert "indices[2]" in refused(np.array([0, 5, 5], np.uint64))        # repeated
    assert "indices[2]" in refused(np.array([0, 7, 8], np.uint64))        # out of range
    refused(good, count=0)
    refused(good, count=(1 << 20) + 1)
    for null in (0, 1, 2, 3, 5, 6):      # indices, values, present, nodes (capacity 4), n_nodes, root
        refused(good, null=null)
    refused(good, cp=99)
    other = Backend()
    assert "another context" in refused(good, ctx=other.ctx)
    other.close()
    # a short capacity: only *n_nodes is written, with the need
    for capacity in (0, need - 1):
        rc, values, present, nodes, n_nodes, out_root = _open(backend, led, good, capacity)
        assert rc == -1 and "nodes_capacity" in _error(backend)
        assert int(n_nodes[0]) == need and _untouched(values, present, nodes, out_root)
    # the call itself is good, with room to spare and exactly enough, and writes nothing beyond what it states
    for capacity in (need, need + 2):
        rc, values, present, nodes, n_nodes, out_root = _open(backend, led, good, capacity)
        assert rc == 0, _error(backend)
        want_nodes, want_values, want_present, _, want_root = _model_proof(m, good)
        assert int(n_nodes[0]) == need and np.array_equal(nodes[:need], want_nodes) and np.array_equal(values[:3], want_values)
        assert np.array_equal(present[:3], want_present) and np.array_equal(out_root[:7], want_root)
        assert _untouched(values[3:], present[3:], nodes[need:], out_root[7:])
    # all leaves: no node, a null nodes_out with capacity 0 is legal
    everything = np.arange(8, dtype=np.uint64)
    rc, values, present, nodes, n_nodes, out_root = _open(backend, led, everything, 0, null=3)
    assert rc == 0 and int(n_nodes[0]) == 0 and np.array_equal(out_root[:7], root) and _untouched(nodes)
    assert np.array_equal(led.root(), root)
    led.close()


# ---- 8. the resident witness ------------------------------------------------------------------------------------------------------------------
def test_open_multi_and_check_leave_a_resident_batch(backend):
    """a batch resident from apply(want_witness=False): open_multi and check between apply and prove, and the proof is the proof without them"""
    from certificate_stark_amd.prover import Ledger, get_example_options
    w = LC.generated((2, 3, 2))
    backend.upload_witness(w)
    expected = backend.prove(get_example_options())
    indices, values = LC.initial_accounts(w)
    led = Ledger(3, backend)
    led.set_accounts(indices, values)
    assert led.apply(w, want_witness=False) is None
    opening = led.open_multi(np.arange(8, dtype=np.uint64)[::-1])
    assert len(opening.nodes) == 0 and np.array_equal(opening.root, w.final_root)
    got = opening.check()
    assert got.verdict == MC.VALID and got.n_merges == 7 and np.array_equal(got.root, w.final_root)
    some = led.open_multi(indices[:2])
    assert some.check().verdict == MC.VALID
    assert backend.prove(get_example_options()) == expected
    led.close()


# ---- 9. the Python layers -----------------------------------------------------------------------------------------------------------------------
def test_python_layers(backend):
    from certificate_stark_amd.prover import MultiproofCheck, check_account_multiproof
    sc = LS.BY_NAME["single_deep"]
    led = _ledger(backend, sc)
    o = led.open_multi([12345, 0, 12346, 12345])
    led.close()
    assert list(o.indices) == [0, 12345, 12346] and list(o.inverse) == [1, 0, 2, 1] and list(o.present) == [True, True, False]
    assert o.nodes.shape == (MC.shape(15, o.indices)[0], 7) and o.nodes.dtype == np.uint64
    got = check_account_multiproof(15, o.indices, o.nodes, o.root, o.values, o.present, backend=backend)
    assert isinstance(got, MultiproofCheck) and got.verdict == backend.MULTI_VALID and np.array_equal(got.root, o.root)
    short = check_account_multiproof(15, o.indices, o.nodes[:-1], o.root, o.values, o.present, backend=backend)
    assert (short.verdict, short.at, short.root) == (backend.MULTI_NODE_COUNT, len(o.nodes), None)
    unsorted = check_account_multiproof(15, o.indices[::-1], o.nodes, o.root, leaves=MC.leaves_of(o.values, o.present), backend=backend)
    assert (unsorted.verdict, unsorted.at, unsorted.root, unsorted.n_merges) == (backend.MULTI_INDEX, 1, None, None)
    with pytest.raises(ValueError):
        backend.account_check_multiproof(15, o.indices, o.nodes, o.root)
    with pytest.raises(ValueError):
        backend.account_check_multiproof(15, o.indices, o.nodes, o.root, leaves=np.zeros((3, 7), np.uint64), present=o.present)
    with pytest.raises(ValueError):
        backend.account_check_multiproof(15, o.indices, o.nodes, o.root, values=o.values[:2])
