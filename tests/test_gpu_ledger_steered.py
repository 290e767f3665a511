"""The account ledger on the GPU (prover.Ledger) on steered batches against the plain model (ledger_model.py, ledger_scenarios.py):
collisions at every level of the predecessor map, balance edges, bystander accounts whose stored nodes are read as siblings, depths 1
and 31, merge launches with 1, 2 and 3 hashes in the last wave, refusals at every position with their precedence, a pool that grows
while it holds nodes, and MerkleAir proofs of the resident witness that show it satisfies the update constraints."""
import random

import numpy as np
import pytest

import ledger_cases as LC
import ledger_model as LM
import ledger_scenarios as LS
from test_gpu_ledger import _assert_batch

pytestmark = pytest.mark.gpu

MERKLE_OPTIONS = (8, 4, 0, 0, 0, 4, 128)    # the smallest set the suite proves MerkleAir with (test_gpu_air_verify.MERKLE_CASES[0])
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


def _assert_state(led, indices, root, values):
    assert np.array_equal(led.root(), root), "root"
    got, present = led.accounts(indices)
    assert present.all() and np.array_equal(got, values), "accounts"


# ---- 1. array parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", LS.SCENARIOS + LS.ACCEPTED, ids=_ids)
def test_apply_reproduces_the_model(backend, sc):
    e = LS.expected(sc)
    led = _ledger(backend, sc)
    _assert_state(led, sc.indices(), e.initial_root, LS.values(sc))
    _assert_batch(led.apply(LS.transfers(sc)), e.witness)
    _assert_state(led, sc.indices(), e.final_root, e.final_values)      # bystanders included
    led.close()


# ---- 2. batch composition -------------------------------------------------------------------------------------------------------------------
_SPLIT = [sc for sc in LS.SCENARIOS if sc.n_tx >= 2]
assert [sc.name for sc in LS.SCENARIOS if sc not in _SPLIT] == ["single_deep"]       # one transfer: no cut point


@pytest.mark.parametrize("sc", _SPLIT, ids=_ids)
def test_batches_compose_at_every_cut(backend, sc):
    e = LS.expected(sc)
    for cut in range(1, sc.n_tx):
        led = _ledger(backend, sc)
        _assert_batch(led.apply(LS.transfers(sc, 0, cut)), e.witness, 0, cut)
        assert np.array_equal(led.root(), e.witness.initial_roots[cut]), cut
        _assert_batch(led.apply(LS.transfers(sc, cut, sc.n_tx)), e.witness, cut, sc.n_tx)
        _assert_state(led, sc.indices(), e.final_root, e.final_values)
        led.close()


# ---- 3. set_accounts launch shapes ------------------------------------------------------------------------------------------------------------
# depth 7; a call's launch at level l hashes the distinct ancestors its accounts have there, four to a wave.  One leaf, sibling pairs,
# cousins and isolated leaves, chosen so that no launch of any call fills its last wave
SHAPES = [[77], [4, 5], [4, 5, 100], [6, 7, 90, 91, 119], [8, 16, 69, 91, 92, 124, 125], [67, 70, 71, 75, 87, 92, 93, 124, 125]]


def _launch_sizes(indices, depth):
    """jobs per launch of one set_accounts call: the leaves, then the distinct parents level by level up to the root"""
    sizes, level = [], set(indices)
    for _ in range(depth + 1):
        sizes.append(len(level))
        level = set(x >> 1 for x in level)
    return sizes


def test_set_accounts_launch_shapes(backend):
    from certificate_stark_amd.prover import Ledger
    sizes = [_launch_sizes(ix, 7) for ix in SHAPES]
    assert [s[0] for s in sizes] == [1, 2, 3, 5, 7, 9]
    assert all(n % 4 for s in sizes for n in s), sizes
    assert {n % 4 for s in sizes for n in s[1:]} == {1, 2, 3} and {s[0] % 4 for s in sizes} == {1, 2, 3}
    for k, indices in enumerate(SHAPES):
        n = len(indices)
        first = LS.account_values([(LS.B + i, i) for i in range(n)], seed=100 + k)
        led, m = Ledger(7, backend), LM.LedgerModel(7)
        led.set_accounts(np.array(indices, np.uint64), first)
        m.set_accounts(indices, first)
        _assert_state(led, indices, m.root(), first)
        if n > 1:       # an overwrite of a strict subset: its leaves are hashed anew, the other accounts' stored nodes are read
            subset = indices[1::2]
            assert 0 < len(subset) < n
            second = LS.account_values([(7 * i, LS.P - 1 - i) for i in range(len(subset))], seed=200 + k)
            led.set_accounts(np.array(subset, np.uint64), second)
            m.set_accounts(subset, second)
            _assert_state(led, indices, m.root(), m.accounts(indices))
        led.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc,at,reason", LS.REFUSALS, ids=lambda v: getattr(v, "name", None))
def test_refused_batches_change_nothing(backend, sc, at, reason):
    """The refusal's position and reason are the scenario's (and the model's); root, accounts and the resident witness -- another
    batch's, uploaded before -- are as before the call, also where earlier transfers of the refused batch had changed balances in the
    plan; the ledger then applies the valid prefix as the model does."""
    from certificate_stark_amd.prover import TransferRefused, get_example_options
    assert LS.expected(sc).refusal == (at, reason)
    led = _ledger(backend, sc)
    root = led.root()
    assert np.array_equal(root, LS.expected(sc).initial_root)
    backend.upload_witness(LC.generated((2, 3, 2)))
    previous = backend.prove(get_example_options())
    with pytest.raises(TransferRefused) as e:
        led.apply(LS.transfers(sc))
    assert (e.value.index, e.value.reason) == (at, reason)
    _assert_state(led, sc.indices(), root, LS.values(sc))
    absent = [i for s, r, _ in sc.transfers for i in (s, r) if i not in sc.accounts]
    if absent:
        assert not led.accounts(np.array(absent, np.uint64))[1].any()
    assert backend.prove(get_example_options()) == previous, "a refused batch changed the resident witness"
    if at:
        valid = LS.expected(sc.prefix(at))
        _assert_batch(led.apply(LS.transfers(sc, 0, at)), valid.witness)
        _assert_state(led, sc.indices(), valid.final_root, valid.final_values)
    led.close()


# ---- 5. pool growth -------------------------------------------------------------------------------------------------------------------------
def test_pool_grows_while_it_holds_nodes(backend):
    """One ledger at depth 15: three set_accounts calls of 70 fresh accounts, each followed by two transfers between the oldest account
    and the call's newest, then 80 transfers in one batch.  The pool of stored nodes grows when n_stored + leaves * (depth + 1) exceeds
    its capacity (none at first, then 1024 doubled until it fits), where leaves is the call's accounts, or twice its transfers.  With
    these indices the tree holds 685, 1250 and 1787 nodes after the three set_accounts calls, so: the first set_accounts allocates
    (0 + 1120 > 0: capacity 2048), the second stays (685 + 1120 <= 2048), the third grows to 4096 while 1250 nodes are stored
    (1250 + 1120 > 2048), none of the two-transfer batches grows (64 more at most), and the 80-transfer batch grows to 8192 while
    1787 nodes are stored (1787 + 160 * 16 > 4096).  The test asserts these crossings from the model's node counts."""
    from certificate_stark_amd.prover import Ledger
    rng = random.Random(0x9001)
    indices = rng.sample(range(1 << 15), 210)
    led, m = Ledger(15, backend), LM.LedgerModel(15)
    capacity, crossed = 0, []

    def reserve(leaves):
        nonlocal capacity
        need = m.n_nodes() + leaves * 16
        crossed.append(need > capacity)
        if need > capacity:
            capacity = capacity or 1024
            while capacity < need:
                capacity *= 2

    def batch(tr):
        reserve(2 * len(tr))
        arrays = LS.transfer_arrays(tr)
        _assert_batch(led.apply(arrays), m.apply(*arrays))

    for call in range(3):
        fresh = indices[70 * call:70 * call + 70]
        values = LS.account_values([(LS.B, i) for i in range(70)], seed=300 + call)
        reserve(70)
        led.set_accounts(np.array(fresh, np.uint64), values)
        m.set_accounts(fresh, values)
        assert np.array_equal(led.root(), m.root()), call
        batch([(indices[0], fresh[-1], 3), (fresh[-1], indices[0], 2)])
        _assert_state(led, indices[:70 * call + 70], m.root(), m.accounts(indices[:70 * call + 70]))
    batch([(indices[i], indices[209 - i], i) for i in range(80)])
    _assert_state(led, indices, m.root(), m.accounts(indices))
    assert crossed == [True, False, False, False, True, False, True] and capacity == 8192
    led.close()


# ---- 6. the resident witness satisfies the Merkle-update constraints -----------------------------------------------------------------------
@pytest.mark.parametrize("sc", LS.SCENARIOS, ids=_ids)
def test_resident_witness_proves_the_merkle_update(backend, sc):
    """MerkleAir (root chaining, balances cancelling, sender nonce + 1, receiver nonce unchanged) on the witness the ledger left resident
    for the scenario's power-of-two form: accepted by the GPU verifier and by the restated one with the model's roots as the statement,
    rejected by both with a root of another scenario."""
    from certificate_stark_amd import VERDICTS
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import ProofOptions
    from oracle import verifier as Vf
    form = sc.proof_form()
    assert form.n_tx in (1, 2, 4, 8)
    e = LS.expected(form)
    other = LS.expected(LS.SCENARIOS[(LS.SCENARIOS.index(sc) + 1) % len(LS.SCENARIOS)].proof_form())
    led = _ledger(backend, form)
    assert led.apply(LS.transfers(form), want_witness=False) is None
    proof = backend.air_prove(Backend.AIR_MERKLE, ProofOptions(*MERKLE_OPTIONS))
    led.close()
    statements = [(e.initial_root, e.final_root), (e.initial_root, other.final_root), (other.initial_root, e.final_root)]
    assert not np.array_equal(e.final_root, other.final_root) and not np.array_equal(e.initial_root, other.initial_root)
    verdicts = backend.air_verify([proof] * 3, Backend.AIR_MERKLE, np.stack([np.concatenate(s) for s in statements]), ProofOptions(*MERKLE_OPTIONS))
    assert [VERDICTS[int(v)] for v in verdicts] == ["OK", "OOD", "OOD"]
    assert Vf.verify_merkle(proof, *statements[0], options=list(MERKLE_OPTIONS))
    for wrong in statements[1:]:
        with pytest.raises(Vf.VerifierError):
            Vf.verify_merkle(proof, *wrong, options=list(MERKLE_OPTIONS))
