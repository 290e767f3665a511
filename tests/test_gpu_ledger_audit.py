"""cstark_ledger_audit on the GPU (k_ledger_audit): job counts around the four hashes of a wave, one corrupted digest per run
(cstark_debug_ledger_xor_word: nothing else can make a resident tree inconsistent) named with the failing jobs the job order predicts,
a digest that only a checkpoint's log reaches, and the audit's read-only contract.  The expected failures are worked out from the plain
model (ledger_checkpoint_cases.audit_jobs), not from the ledger.  Clean audits of every state the checkpoint tests reach, at id 0 and at
every live id, run inside test_gpu_ledger_checkpoints.py (ledger_checkpoint_cases.assert_state)."""
import numpy as np
import pytest

import ledger_cases as LC
import ledger_checkpoint_cases as CC
import sig_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _pair(backend, depth, accounts, seed=11):
    p = CC.Pair(backend, depth, seed)
    p.set_accounts(list(accounts))
    return p


def _first(r):
    return (r.first_kind, r.first_level, r.first_index)


def _assert_clean(led, m, at=None):
    r = led.audit(at=at)
    assert (r.consistent, r.n_bad, r.n_nodes) == (1, 0, m.n_nodes()) and _first(r) == (0, 0, 0), CC.report_tuple(r)


def _assert_corruption_is_named(led, m, symbol, word, at=None):
    """one word of one digest wrong: the audit fails the jobs that read it, names the first of them, and has written nothing"""
    n_bad, first = CC.expected_failures(m, symbol)
    assert CC.xor_word(led, symbol, word, at=at or 0) == 0
    r = led.audit(at=at)
    assert (r.consistent, r.n_bad, _first(r)) == (0, n_bad, first), (CC.report_tuple(r), n_bad, first)
    again = led.audit(at=at)
    assert CC.report_tuple(again) == CC.report_tuple(r)
    assert CC.xor_word(led, symbol, word, at=at or 0) == 0
    _assert_clean(led, m, at)
    return n_bad, first


# depth 3, the accounts chosen for depth + n_nodes = 7, 8, 9, 10 jobs: every residue of the four hashes of a wave, two or three workgroups
RESIDUES = {3: [0], 0: [0, 1], 1: [0, 2], 2: [0, 4]}


@pytest.mark.parametrize("residue", sorted(RESIDUES))
def test_one_corrupted_digest_is_named(backend, residue):
    accounts = RESIDUES[residue]
    p = _pair(backend, 3, accounts)
    m, led, d = p.m, p.led, 3
    n_jobs = d + m.n_nodes()
    assert n_jobs % 4 == residue and n_jobs > 4
    _assert_clean(led, m)
    jobs = CC.audit_jobs(m)
    assert len(jobs) == n_jobs + 1                                  # and the all-zero test of the empty leaf digest, run on the host
    leaf, top = max(accounts), accounts[0] >> 1
    word = [0, 6, 3, 0][residue]
    # a leaf: its own job, then its parent's
    assert _assert_corruption_is_named(led, m, ("node", d, leaf), word) == (2, (CC.LEAF, d, leaf))
    # an inner node: itself and its parent, the lower level first
    assert _assert_corruption_is_named(led, m, ("node", d - 1, top), 6 - word) == (2, (CC.INNER, d - 1, top))
    # the root, the last job (of a partial group unless the count is a multiple of four): nothing above it fails
    assert jobs[-1][:3] == (CC.INNER, 0, 0)
    assert _assert_corruption_is_named(led, m, ("node", 0, 0), word) == (1, (CC.INNER, 0, 0))
    # the first job of the launch: empty-subtree digest depth - 1, read by its own test, by the test above it and by every inner
    # node of level depth - 2 with an untouched child
    n_bad, first = _assert_corruption_is_named(led, m, ("empty", d - 1, 0), 6 - word)
    assert first == (CC.EMPTY, d - 1, 0) and n_bad == 2 + sum(1 for x in m.node[d - 2] if not (2 * x in m.node[d - 1] and 2 * x + 1 in m.node[d - 1]))
    # the empty leaf digest: its all-zero test comes first, then the test of the level above and the parents of single leaves
    n_bad, first = _assert_corruption_is_named(led, m, ("empty", d, 0), word)
    assert first == (CC.EMPTY, d, 0) and n_bad >= 2
    # empty-subtree digest 0 is read by its own test only (the root is stored)
    assert _assert_corruption_is_named(led, m, ("empty", 0, 0), word) == (1, (CC.EMPTY, 0, 0))
    p.close()


@pytest.mark.parametrize("depth", [1, 15, 31])
def test_corruptions_at_other_depths(backend, depth):
    first, later = CC.ACCOUNTS[depth]
    p = _pair(backend, depth, first + later)
    got, want = p.apply(4, first)
    assert np.array_equal(got.final_root, want.final_root)
    m, led = p.m, p.led
    _assert_clean(led, m)
    leaf = first[-1]
    n_bad, named = _assert_corruption_is_named(led, m, ("node", depth, leaf), 0)       # depth 1: a leaf is also the root's child
    assert (n_bad, named) == (2, (CC.LEAF, depth, leaf))
    if depth > 1:
        level = depth // 2
        n_bad, named = _assert_corruption_is_named(led, m, ("node", level, leaf >> (depth - level)), 6)
        assert (n_bad, named) == (2, (CC.INNER, level, leaf >> (depth - level)))
    assert _assert_corruption_is_named(led, m, ("node", 0, 0), 6) == (1, (CC.INNER, 0, 0))
    p.close()


def test_a_digest_only_a_checkpoint_reaches(backend):
    depth = 3
    first, later = CC.ACCOUNTS[depth]
    p = _pair(backend, depth, first)
    cp = p.checkpoint()
    got, want = p.apply(8, first)                                                    # every touched node moves to a fresh slot
    assert np.array_equal(got.final_root, want.final_root)
    old, m, led = p.live[0][1], p.m, p.led
    touched = int(got.s_indices[0])
    _assert_clean(led, old, cp)
    _assert_clean(led, m)
    # the old leaf of a touched account: wrong at the checkpoint, and the current state never reads it
    assert CC.xor_word(led, ("node", depth, touched), 0, at=cp) == 0
    r = led.audit(at=cp)
    assert (r.consistent, r.n_bad, _first(r)) == (0, 2, (CC.LEAF, depth, touched))
    _assert_clean(led, m)
    assert CC.xor_word(led, ("node", depth, touched), 0, at=cp) == 0
    _assert_clean(led, old, cp)
    # and the other way round: the current leaf is wrong now and was not there at the checkpoint
    _assert_corruption_is_named(led, m, ("node", depth, touched), 6)
    assert CC.xor_word(led, ("node", depth, touched), 6) == 0
    _assert_clean(led, old, cp)
    assert led.audit().consistent == 0
    assert CC.xor_word(led, ("node", depth, touched), 6) == 0
    # refusals of the debug call: an id that is not live, a node the state does not store, a word out of range
    assert CC.xor_word(led, ("node", depth, touched), 0, at=99) == 1
    assert CC.xor_word(led, ("node", depth, later[0]), 0) == 1
    assert CC.xor_word(led, ("node", depth, touched), 7) == 1
    assert CC.xor_word(led, ("empty", depth + 1, 0), 0) == 1
    p.assert_all()
    p.close()


def test_the_audit_is_read_only(backend):
    """neither root nor openings nor the resident witness change, and a proof after it is the proof without it"""
    from certificate_stark_amd.prover import Ledger, get_example_options
    w = LC.generated((2, 3, 2))
    indices, initial = LC.initial_accounts(w)
    backend.upload_witness(w)
    expected = backend.prove(get_example_options())
    led = Ledger(3, backend)
    led.set_accounts(indices, initial)
    cp = led.checkpoint()
    assert led.apply(SC.transfers(w), want_witness=False) is None
    root, opening, past = led.root(), led.open(np.arange(8, dtype=np.uint64)), led.open(np.arange(8, dtype=np.uint64), at=cp)
    assert led.audit().consistent == 1 and led.audit(at=cp).consistent == 1
    assert backend.prove(get_example_options()) == expected
    assert np.array_equal(led.root(), root) and np.array_equal(root, w.final_root)
    for at, before in ((None, opening), (cp, past)):
        after = led.open(np.arange(8, dtype=np.uint64), at=at)
        for f in ("values", "present", "paths", "root"):
            assert np.array_equal(getattr(after, f), getattr(before, f)), f
    led.close()
