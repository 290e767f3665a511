"""The model of cstark_tx_witness_check (witness_check_cases.py) on its own, without a GPU: honest witnesses are all VALID and fold to
their stated final root, the messages of an honest witness are the ledger's, and the mutation set of every depth holds every verdict --
so that the GPU tests, which expect what the model says, cannot pass by producing one kind only."""
import numpy as np
import pytest

import sig_cases as SC
import witness_check_cases as WC


@pytest.mark.parametrize("depth", WC.DEPTHS)
def test_generated_witnesses_are_valid_at_every_size(depth):
    for n in WC.SIZES:
        w = WC.generated(n, depth)
        assert (w.n_tx, w.depth) == (n, depth)
        e = WC.check(w, check_signatures=True)
        assert not e.verdicts.any() and (e.first_bad, e.first_verdict, e.n_bad) == (-1, WC.VALID, 0)
        assert np.array_equal(e.final_root, w.final_root)
        assert np.array_equal(e.folds[:, 0], w.initial_roots) and np.array_equal(e.folds[:, 1], e.folds[:, 2])
        assert np.array_equal(WC.check(w, final_root=None).verdicts, e.verdicts)


def test_the_messages_of_an_honest_witness_are_the_ledgers():
    for depth in WC.DEPTHS:
        w = WC.generated(8, depth)
        assert np.array_equal(WC.messages(w), SC.tx_messages(w))


def test_steered_witnesses_are_valid_and_cover_the_named_shapes():
    cases = dict(WC.steered())
    for name, w in cases.items():
        e = WC.check(w)
        assert not e.verdicts.any(), name
        assert np.array_equal(e.final_root, w.final_root), name
    assert sorted(set(w.depth for w in cases.values())) == [1, 3, 7, 15, 31]
    siblings, halves, deep, wraps = cases["pingpong_siblings"], cases["pingpong_halves"], cases["depth31_edges"], cases["receiver_wraps_p"]
    assert all(int(s) ^ int(r) == 1 for s, r in zip(siblings.s_indices, siblings.r_indices))
    assert all((int(s) ^ int(r)) >> (halves.depth - 1) == 1 for s, r in zip(halves.s_indices, halves.r_indices))
    assert any(int(i) >> 30 & 1 for i in deep.s_indices) and any(int(i) >> 30 & 1 for i in deep.r_indices)
    canon = WC.LM.canonical
    assert canon(wraps.s_old_values[0][13]) == WC.P - 1                                        # nonce + 1 wraps to 0
    assert any(canon(w_) + canon(d) >= WC.P for w_, d in zip(wraps.r_old_values[:, 12], wraps.deltas))   # the receiver's balance wraps
    every = list(cases.values())
    assert any(canon(d) == 0 for w in every for d in w.deltas)
    assert any(canon(d) == canon(b) != 0 for w in every for d, b in zip(w.deltas, w.s_old_values[:, 12]))


def test_a_steered_witness_with_unsigned_transfers_fails_the_signature_test_only():
    name, w = WC.steered()[0]
    assert list(WC.check(w, check_signatures=True).verdicts) == [WC.SIGNATURE] * w.n_tx


@pytest.mark.parametrize("depth", WC.DEPTHS)
def test_the_mutation_set_holds_every_verdict(depth):
    cases = WC.mutation_set(depth)
    base = WC.generated(3, depth)
    assert len(cases) == len(WC.mutations(base, 1)) >= 34                  # nothing is dropped, whatever its verdict
    seen = set()
    for name, m, e in cases:
        assert any(not np.array_equal(getattr(m, f), getattr(base, f)) for f in m.FIELDS), name
        seen.update(int(v) for v in e.verdicts)
    assert seen == set(range(10)), sorted(seen)
    by_name = {name: e for name, _, e in cases}
    # what the mutations are FOR, stated on the model's output: the test that names the changed part is the one that fails
    assert by_name["s_index_range"].verdicts[1] == by_name["r_index_range"].verdicts[1] == WC.INDEX_RANGE
    assert by_name["self_transfer"].verdicts[1] == WC.SELF_TRANSFER
    assert by_name["s_leaf"].verdicts[1] == by_name["s_key"].verdicts[1] == WC.SENDER_LEAF
    assert by_name["s_first_sibling"].verdicts[1] == WC.SENDER_PATH
    assert list(by_name["initial_root"].verdicts) == [WC.NEXT_ROOT, WC.SENDER_PATH, WC.VALID]
    assert list(by_name["next_initial_root"].verdicts) == [WC.VALID, WC.NEXT_ROOT, WC.SENDER_PATH]
    assert list(by_name["final_root"].verdicts) == [WC.VALID, WC.VALID, WC.NEXT_ROOT]
    assert by_name["delta_balance_plus_1"].verdicts[1] == WC.BALANCE
    assert by_name["r_balance"].verdicts[1] == by_name["r_key"].verdicts[1] == WC.MIDDLE_ROOT
    assert by_name["r_leaf"].verdicts[1] == WC.RECEIVER_LEAF
    assert by_name["sig_rx"].verdicts[1] == by_name["sig_s_byte"].verdicts[1] == by_name["sig_s_bit255"].verdicts[1] == WC.SIGNATURE
    assert by_name["path_and_signature"].verdicts[1] == WC.SENDER_PATH and by_name["receiver_leaf_and_signature"].verdicts[1] == WC.RECEIVER_LEAF


def test_the_verdict_is_the_first_failing_test_and_the_others_still_run():
    """two bad transfers in one witness: each has its own verdict"""
    m = WC._copy(WC.generated(3, 3))
    WC._bump(m.s_paths, (0, 1, 0))
    WC._bump(m.r_paths, (2, 0, 0))
    e = WC.check(m)
    assert list(e.verdicts) == [WC.SENDER_PATH, WC.VALID, WC.RECEIVER_LEAF] and (e.first_bad, e.first_verdict, e.n_bad) == (0, WC.SENDER_PATH, 2)
