"""The read side of the account ledger on the GPU: cstark_ledger_open_accounts (prover.Ledger.open) against the plain model
(ledger_model.py) and cstark_account_check_paths against the plain fold (ledger_paths_cases.py).  Openings of every steered scenario
before and after its batch, openings that change nothing, paths of ledgers, of the model at depths no ledger takes, and of witnesses;
one launch of tampered paths whose verdicts differ inside every wave; synthetic paths at the operand extremes; refusals that launch
nothing.  Every output buffer starts as 0xA5 with spare room and is compared whole."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import ledger_paths_cases as PC
import ledger_scenarios as LS
from test_gpu_ledger import _assert_batch

pytestmark = pytest.mark.gpu

u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
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


def _error(backend):
    return backend.lib.cstark_last_error().decode()


# ---- the two C calls on 0xA5-filled outputs ------------------------------------------------------------------------------------------
def _open(backend, led, depth, indices, count=None, null=None, ctx=None):
    """-> (status, values, present, paths, root): whole buffers, SPARE rows longer than the call needs"""
    idx = np.ascontiguousarray(indices, np.uint64)
    n = len(idx)
    values = np.full((n + SPARE, 14), PC.FILL64, np.uint64)
    present = np.full(n + SPARE, PC.FILL8, np.uint8)
    paths = np.full((n + SPARE, depth + 1, 7), PC.FILL64, np.uint64)
    root = np.full(7 + SPARE, PC.FILL64, np.uint64)
    args = [_ptr(idx), _ptr(values), _ptr(present, u8p), _ptr(paths), _ptr(root)]
    if null is not None:
        args[null] = None
    rc = backend.lib.cstark_ledger_open_accounts(ctx or backend.ctx, led._led, C.c_uint32(n if count is None else count), *args)
    return rc, values, present, paths, root


def _assert_untouched(*buffers):
    for a in buffers:
        assert (a == (PC.FILL8 if a.dtype == np.uint8 else PC.FILL64)).all()


def _assert_opening(backend, led, m, indices):
    """the opening of `indices` is the model's: values, presence, paths, root, and nothing written beyond them"""
    n, d = len(indices), m.depth
    rc, values, present, paths, root = _open(backend, led, d, indices)
    assert rc == 0, _error(backend)
    for k, i in enumerate(int(i) for i in indices):
        assert present[k] == (i in m.value), i
        assert np.array_equal(values[k], m.value.get(i, np.zeros(14, np.uint64))), i
        assert np.array_equal(paths[k], m._path(i)), i
    assert np.array_equal(root[:7], m.root())
    _assert_untouched(values[n:], present[n:], paths[n:], root[7:])
    return values[:n], present[:n], paths[:n], root[:7]


def _check(backend, depth, indices, paths, roots, values=None, present=None, count=None, n_roots=None, null=None, want_out=True):
    """-> (status, verdicts, roots_out): whole buffers, SPARE rows longer than the call needs"""
    idx, p, r = (np.ascontiguousarray(a, np.uint64) for a in (indices, paths, roots))
    r = r.reshape(-1, 7)
    v = None if values is None else np.ascontiguousarray(values, np.uint64)
    pr = None if present is None else np.ascontiguousarray(present, np.uint8)
    n = len(idx)
    verdicts = np.full(n + SPARE, PC.FILL8, np.uint8)
    out = np.full((n + SPARE, 7), PC.FILL64, np.uint64)
    args = [_ptr(idx), _ptr(v), _ptr(pr, u8p), _ptr(p), _ptr(r), C.c_uint32(len(r) if n_roots is None else n_roots), _ptr(verdicts, u8p),
            _ptr(out) if want_out else None]
    if null is not None:
        args[null] = None
    rc = backend.lib.cstark_account_check_paths(backend.ctx, C.c_uint32(n if count is None else count), C.c_uint32(depth), *args)
    return rc, verdicts, out


def _assert_check(backend, depth, indices, paths, roots, values=None, present=None, expected=None):
    """verdicts and folded roots are the reference's for every path; `expected`: what the case itself says the verdicts are"""
    n = len(indices)
    roots = np.asarray(roots, np.uint64).reshape(-1, 7)
    ref_v, ref_r = [], []
    for k in range(n):
        root = roots[k if len(roots) > 1 else 0]
        ref_v.append(PC.expected_verdict(indices[k], paths[k], depth, root, None if values is None else values[k],
                                         True if present is None else bool(present[k])))
        ref_r.append(PC.fold(indices[k], paths[k], depth))
    if expected is not None:
        assert ref_v == list(expected), "the reference itself disagrees with the case"
    rc, verdicts, out = _check(backend, depth, indices, paths, roots, values, present)
    assert rc == 0, _error(backend)
    assert list(verdicts[:n]) == ref_v, (list(verdicts[:n]), ref_v)
    assert np.array_equal(out[:n], np.array(ref_r, np.uint64))
    _assert_untouched(verdicts[n:], out[n:])


# ---- 1. open against the model --------------------------------------------------------------------------------------------------------
assert sorted(set(sc.depth for sc in LS.SCENARIOS)) == [1, 3, 7, 15, 31]


@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=_ids)
def test_open_reproduces_the_model(backend, sc):
    indices = PC.interesting_indices(sc)
    assert len(set(indices.tolist())) < len(indices)
    assert len(sc.accounts) == 1 << sc.depth or any(int(i) not in sc.accounts for i in indices)
    led, m = _ledger(backend, sc), LS.model(sc)
    _assert_opening(backend, led, m, indices)
    _assert_batch(led.apply(LS.transfers(sc)), m.apply(*LS.transfers(sc)))
    _assert_opening(backend, led, m, indices)
    led.close()


@pytest.mark.parametrize("depth", [1, 7, 31])
def test_an_empty_ledger_opens_to_the_empty_digests(backend, depth):
    from certificate_stark_amd.prover import Ledger
    led, m = Ledger(depth, backend), LM.LedgerModel(depth)
    indices = np.array([0, (1 << depth) - 1, (1 << depth) // 3, 0], np.uint64)
    values, present, paths, root = _assert_opening(backend, led, m, indices)
    assert not present.any() and not values.any()
    assert all(np.array_equal(paths[k, j + 1], m.empty[depth - j]) for k in range(4) for j in range(depth)) and not paths[:, 0].any()
    assert np.array_equal(root, m.empty[0])
    led.close()


# ---- 2. open changes nothing ----------------------------------------------------------------------------------------------------------
def test_open_leaves_the_ledger_as_it_was(backend):
    sc = LS.BY_NAME["bystander_siblings"]
    led, m = _ledger(backend, sc), LS.model(sc)
    root, (values, present) = led.root(), led.accounts(sc.indices())
    opening = led.open(PC.interesting_indices(sc))
    assert not opening.check().any()
    assert np.array_equal(led.root(), root) and np.array_equal(opening.root, root)
    again = led.accounts(sc.indices())
    assert np.array_equal(again[0], values) and np.array_equal(again[1], present)
    _assert_batch(led.apply(LS.transfers(sc)), m.apply(*LS.transfers(sc)))
    led.close()


def test_open_and_check_leave_a_resident_batch(backend):
    """a batch resident from apply(want_witness=False): open and check between apply and prove, and the proof is the proof without them"""
    from certificate_stark_amd.prover import Ledger, get_example_options
    w = LC.generated((2, 3, 2))
    backend.upload_witness(w)
    expected = backend.prove(get_example_options())
    indices, values = LC.initial_accounts(w)
    led = Ledger(3, backend)
    led.set_accounts(indices, values)
    assert led.apply(w, want_witness=False) is None
    opening = led.open(np.arange(8, dtype=np.uint64))
    assert np.array_equal(opening.root, w.final_root) and not opening.check().any()
    assert backend.prove(get_example_options()) == expected
    led.close()


def test_open_refusals_leave_the_outputs(backend):
    from certificate_stark_amd.backend import Backend
    sc = LS.BY_NAME["pingpong_halves"]
    led = _ledger(backend, sc)
    root = led.root()
    good = np.array([0, 7, 5], np.uint64)

    def refused(indices, **kw):
        rc, *buffers = _open(backend, led, sc.depth, indices, **kw)
        assert rc == -1
        _assert_untouched(*buffers)
        return _error(backend)

    assert "indices[2]" in refused(np.array([0, 7, 8], np.uint64))
    assert "indices[0]" in refused(np.array([2**64 - 1, 7, 8], np.uint64))
    refused(good, count=0)
    refused(good, count=(1 << 20) + 1)
    for null in range(5):
        refused(good, null=null)
    other = Backend()
    assert "another context" in refused(good, ctx=other.ctx)
    other.close()
    assert np.array_equal(led.root(), root)
    _assert_opening(backend, led, LS.model(sc), good)
    led.close()


# ---- 3. check: valid paths ------------------------------------------------------------------------------------------------------------
# counts around the four paths of a wave and a partial last group
@pytest.mark.parametrize("count", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("name", ["depth1_busy", "pingpong_halves", "depth31_edges"])
def test_opened_paths_verify(backend, name, count):
    sc = LS.BY_NAME[name]
    pool = PC.interesting_indices(sc)
    indices = np.array([pool[k % len(pool)] for k in range(count)], np.uint64)
    led = _ledger(backend, sc)
    opening = led.open(indices)
    led.close()
    assert opening.paths.shape == (count, sc.depth + 1, 7)
    _assert_check(backend, sc.depth, indices, opening.paths, opening.root, opening.values, opening.present.astype(np.uint8), [PC.VALID] * count)


# depths no ledger takes: the checker folds any depth
@pytest.mark.parametrize("depth", [2, 5])
def test_model_paths_of_other_depths_verify(backend, depth):
    m = LM.LedgerModel(depth)
    top = (1 << depth) - 1
    have = [0, top]
    m.set_accounts(have, LS.account_values([(LS.B + i, i) for i in range(2)], seed=depth))
    indices = np.array([0, top, 0, 1, top - 1], np.uint64)
    paths = np.array([m._path(int(i)) for i in indices], np.uint64)
    values = np.array([m.value.get(int(i), np.zeros(14, np.uint64)) for i in indices], np.uint64)
    present = np.array([int(i) in m.value for i in indices], np.uint8)
    assert list(present) == [1, 1, 1, 0, 0] and 0 < top - 1 < top
    _assert_check(backend, depth, indices, paths, m.root(), values, present, [PC.VALID] * 5)
    _assert_check(backend, depth, indices, paths, m.root(), expected=[PC.VALID] * 5)


# ---- 4. check: the paths of a witness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generated_2_3_2", "chain_full_balance"])
def test_witness_paths_verify(backend, oracle, which):
    w = LC.generated((2, 3, 2)) if which == "generated_2_3_2" else LS.expected(LS.BY_NAME[which]).witness
    n = w.n_tx
    assert w.depth == 3 and n == (2 if which == "generated_2_3_2" else 8)
    # the sender's path and old value under the root before transfer t
    _assert_check(backend, 3, w.s_indices, w.s_paths, w.initial_roots, w.s_old_values, expected=[PC.VALID] * n)
    # the receiver's path with its NEW value under the root after transfer t
    r_new = w.r_old_values.copy()
    r_new[:, 12] = oracle.fp_add(w.r_old_values[:, 12].copy(), w.deltas)
    after = np.concatenate([w.initial_roots[1:], w.final_root.reshape(1, 7)])
    _assert_check(backend, 3, w.r_indices, w.r_paths, after, r_new, expected=[PC.VALID] * n)


# ---- 5. check: tampered paths, one launch with mixed verdicts ---------------------------------------------------------------------------
def _tampered(backend):
    """(indices, values, present, paths, roots, expected with values, expected in digest mode): every case behind a valid path"""
    sc = LS.BY_NAME["bystander_siblings"]
    assert sc.depth == 7 and 10 in sc.accounts and 12 not in sc.accounts
    led = _ledger(backend, sc)
    o = led.open(np.array([10, 12], np.uint64))
    led.close()
    assert list(o.present) == [True, False]
    good = (10, o.values[0], 1, o.paths[0], o.root)
    absent = (12, o.values[1], 0, o.paths[1], o.root)
    cases = []      # (index, value, present, path, root), verdict with values, verdict in digest mode

    def add(with_values, digest, index=good[0], value=good[1], present=1, path=good[3], root=good[4]):
        cases.append(((index, value, present, path, root), with_values, digest))

    for k in range(8):      # entry k, word k mod 7
        path = good[3].copy()
        path[k, k % 7] = PC.bump(path[k, k % 7])
        add(PC.LEAF if k == 0 else PC.ROOT, PC.ROOT, path=path)
    for b in range(7):
        add(PC.ROOT, PC.ROOT, index=10 ^ (1 << b))
    richer = good[1].copy()
    richer[12] = PC.bump(richer[12])
    add(PC.LEAF, PC.VALID, value=richer)
    add(PC.LEAF, PC.VALID, present=0)
    cases.append(((absent[0], absent[1], 1, absent[3], absent[4]), PC.LEAF, PC.VALID))
    root = good[4].copy()
    root[6] = PC.bump(root[6])
    add(PC.ROOT, PC.ROOT, root=root)
    add(PC.INDEX_RANGE, PC.INDEX_RANGE, index=10 + 128)
    bad_leaf = good[3].copy()
    bad_leaf[0, 3] = PC.bump(bad_leaf[0, 3])
    add(PC.INDEX_RANGE, PC.INDEX_RANGE, index=10 + 128, path=bad_leaf)
    rows, with_values, digest = [], [], []
    for k, (case, v, dg) in enumerate(cases):
        rows += [case, absent if k % 3 == 2 else good]
        with_values += [v, PC.VALID]
        digest += [dg, PC.VALID]
    columns = [np.array([r[j] for r in rows], t) for j, t in enumerate((np.uint64, np.uint64, np.uint8, np.uint64, np.uint64))]
    return columns, with_values, digest


def test_tampered_paths_in_one_launch(backend):
    (indices, values, present, paths, roots), with_values, digest = _tampered(backend)
    n = len(indices)
    assert n == 42 and roots.shape == (n, 7)
    # every wave (four consecutive paths) holds at least two different verdicts
    assert all(len(set(with_values[g:g + 4])) >= 2 for g in range(0, n, 4))
    assert set(with_values) == {PC.VALID, PC.INDEX_RANGE, PC.LEAF, PC.ROOT}
    _assert_check(backend, 7, indices, paths, roots, values, present, with_values)
    _assert_check(backend, 7, indices, paths, roots, expected=digest)


# ---- 6. digest mode -------------------------------------------------------------------------------------------------------------------
def test_digest_mode_takes_the_sibling_for_the_leaf(backend):
    sc = LS.BY_NAME["bystander_siblings"]
    led = _ledger(backend, sc)
    o = led.open(np.array([10, 20, 127], np.uint64))     # siblings 11 and 21 hold accounts, 126 holds none
    led.close()
    swapped = o.paths.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    _assert_check(backend, 7, o.indices ^ np.uint64(1), swapped, o.root, expected=[PC.VALID] * 3)
    # with the accounts' values the same pairs are no openings of them
    _assert_check(backend, 7, o.indices ^ np.uint64(1), swapped, o.root, o.values, o.present.astype(np.uint8), [PC.LEAF] * 3)


# ---- 7. extremes: synthetic paths that are no tree's -----------------------------------------------------------------------------------
def test_synthetic_paths_at_the_operand_extremes(backend):
    depth, top = 31, np.uint64(PC.P - 1)
    zeros, tops = np.zeros((depth + 1, 7), np.uint64), np.full((depth + 1, 7), top, np.uint64)
    alternating = zeros.copy()
    alternating[0::2, 1::2] = top
    alternating[1::2, 0::2] = top
    indices = np.repeat(np.array([0, 2**31 - 1, 0x55555555, 0x2AAAAAAA], np.uint64), 3)
    paths = np.array([zeros, tops, alternating] * 4, np.uint64)
    roots = np.array([PC.fold(i, p, depth) for i, p in zip(indices, paths)], np.uint64)
    _assert_check(backend, depth, indices, paths, roots, expected=[PC.VALID] * 12)
    for k in range(12):
        roots[k, k % 7] = PC.bump(roots[k, k % 7])
    _assert_check(backend, depth, indices, paths, roots, expected=[PC.ROOT] * 12)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_check_refusals_launch_nothing_and_leave_the_outputs(backend):
    m = LM.LedgerModel(3)
    have = [1, 6]
    m.set_accounts(have, LS.account_values([(5, 0), (6, 1)], seed=8))
    indices = np.array([1, 6, 2, 1, 7], np.uint64)
    paths = np.array([m._path(int(i)) for i in indices], np.uint64)
    values = np.array([m.value.get(int(i), np.zeros(14, np.uint64)) for i in indices], np.uint64)
    present = np.array([int(i) in m.value for i in indices], np.uint8)
    roots = np.tile(m.root(), (5, 1))

    def refused(*args, **kw):
        rc, verdicts, out = _check(backend, *args, **kw)
        assert rc == -1
        _assert_untouched(verdicts, out)
        return _error(backend)

    # the call itself is good
    _assert_check(backend, 3, indices, paths, roots, values, present, [PC.VALID] * 5)
    for null in (0, 3, 4, 6):       # indices, paths, roots, verdicts
        refused(3, indices, paths, roots, values, present, null=null)
    refused(3, indices, paths, roots, values, present, count=0)
    refused(3, indices, paths, roots, values, present, count=(1 << 20) + 1)
    refused(0, indices, paths, roots, values, present)
    refused(32, indices, paths, roots, values, present)
    for n_roots in (0, 2, 4, 6):
        refused(3, indices, paths, roots, values, present, n_roots=n_roots)
    refused(3, indices, paths, roots, None, present)
    bad = values.copy()
    bad[2, 13] = PC.P
    bad[4, 0] = PC.P
    assert "values[2][13]" in refused(3, indices, paths, roots, bad, present)
    bad = paths.copy()
    bad[1, 2, 5] = PC.P
    bad[3, 0, 0] = 2**64 - 1
    assert "paths[1][2][5]" in refused(3, indices, bad, roots, values, present)
    assert "paths[1][2][5]" in refused(3, indices, bad, roots)
    bad = roots.copy()
    bad[3, 6] = PC.P
    assert "roots[3][6]" in refused(3, indices, paths, bad, values, present)
    # a null roots_out, a null present and null values are no refusals
    rc, verdicts, out = _check(backend, 3, indices, paths, roots, values, present, want_out=False)
    assert rc == 0 and not verdicts[:5].any()
    _assert_untouched(verdicts[5:], out)
    rc, verdicts, _ = _check(backend, 3, indices[:2], paths[:2], roots[:1], values[:2])
    assert rc == 0 and not verdicts[:2].any()


# ---- 9. an opening taken before a batch -------------------------------------------------------------------------------------------------
def test_an_opening_goes_stale_with_the_root(backend):
    sc = LS.BY_NAME["pingpong_halves"]
    touched, bystander = 0, sc.bystanders()[0]
    led = _ledger(backend, sc)
    old = led.open(np.array([touched, bystander], np.uint64))
    led.apply(LS.transfers(sc))
    new_root = led.root()
    led.close()
    assert np.array_equal(old.root, LS.expected(sc).initial_root) and np.array_equal(new_root, LS.expected(sc).final_root)
    present = old.present.astype(np.uint8)
    _assert_check(backend, 3, old.indices, old.paths, new_root, old.values, present, [PC.ROOT] * 2)
    _assert_check(backend, 3, old.indices, old.paths, old.root, old.values, present, [PC.VALID] * 2)


# ---- 10. the Python layers ------------------------------------------------------------------------------------------------------------
def test_python_layers(backend):
    from certificate_stark_amd.prover import AccountOpening, check_account_paths
    sc = LS.BY_NAME["single_deep"]
    led = _ledger(backend, sc)
    o = led.open([12345, 12346, 0])
    led.close()
    assert isinstance(o, AccountOpening) and o.depth == 15 and o.paths.shape == (3, 16, 7) and list(o.present) == [True, False, True]
    assert o.check().dtype == np.uint8 and not o.check().any()
    paths = o.paths.copy()
    paths[1, 9, 0] = PC.bump(paths[1, 9, 0])
    verdicts, folded = check_account_paths(o.indices, paths, o.root, o.values, o.present, backend=backend, want_roots=True)
    assert list(verdicts) == [backend.PATH_VALID, backend.PATH_ROOT, backend.PATH_VALID]
    assert np.array_equal(folded[0], o.root) and np.array_equal(folded[1], PC.fold(12346, paths[1], 15))
    assert list(check_account_paths(o.indices, paths, np.tile(o.root, (3, 1)), backend=backend)) == [0, backend.PATH_ROOT, 0]
    with pytest.raises(ValueError):
        backend.account_check_paths(o.indices, paths[:2], o.root)
    with pytest.raises(ValueError):
        backend.account_check_paths(o.indices, paths, o.root, present=o.present)
