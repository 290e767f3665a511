"""No GPU: the references that test_gpu_commit_layouts.py and test_gpu_open_gather.py hold the kernels to (tests/commit_cases.py) are
checked against the oracle's own tree here, so that a GPU failure there points at the kernel and not at the test."""
import numpy as np
import pytest

import commit_cases as K


def test_slot_permutation_and_its_inverse():
    for log_b in range(5):
        for log_s in range(log_b + 1):
            b, s, ce = 1 << log_b, 1 << log_s, 1 << (log_b - log_s)
            slots = [K.coset_slot(k, log_b, log_s) for k in range(b)]
            assert sorted(slots) == list(range(b))
            assert [K.slot_coset(v, log_b, log_s) for v in slots] == list(range(b))
            assert [K.coset_slot(K.slot_coset(v, log_b, log_s), log_b, log_s) for v in range(b)] == list(range(b))
            # block r = the cosets k = r (mod s) in increasing order; block 0 starts the table; no blocks: natural order
            for r in range(s):
                assert [K.slot_coset(r * ce + i, log_b, log_s) for i in range(ce)] == [i * s + r for i in range(ce)]
            if log_s == 0:
                assert slots == list(range(b))
    table = np.arange(16 * 3 * 4, dtype=np.uint64).reshape(16, 3, 4)
    slots = K.to_slots(table, 2)
    assert (slots[0] == table[0]).all() and (slots[1] == table[4]).all() and (slots[4] == table[1]).all() and (slots[15] == table[15]).all()
    # a row read back through the slots is the natural table's row
    pos = [0, 63, 17, 16, 5]
    assert (K.rows_at(slots, pos, 2) == K.rows_at(table, pos, 0)).all()
    assert (K.rows_at(table, [16 * 3 + 5], 0)[0] == table[5, :, 3]).all()


@pytest.mark.parametrize("hash_fn", [0, 1])
def test_indexed_paths_fold_to_the_root(oracle, hash_fn):
    leaves = np.random.default_rng(64 + hash_fn).integers(0, 256, size=(64, 32), dtype=np.uint8)
    nodes = oracle.merkle_build(leaves, hash_fn)
    # the merge is the oracle's: every inner node is the merge of its children
    for i in (1, 2, 31, 63):
        assert (K.merge(nodes[2 * i], nodes[2 * i + 1], hash_fn, oracle) == nodes[i]).all()
    for pos in range(64):
        path = K.path_at(nodes, pos)
        assert len(path) == 6
        assert (K.fold_path(leaves[pos], pos, path, hash_fn, oracle) == nodes[1]).all(), pos
        # a path that starts higher continues from the node it would have reached
        assert (K.fold_path(nodes[(64 + pos) >> 2], pos >> 2, K.path_at(nodes, pos, 2), hash_fn, oracle) == nodes[1]).all(), pos
    wrong = K.path_at(nodes, 5)
    assert not (K.fold_path(leaves[4], 4, wrong, hash_fn, oracle) == nodes[1]).all()


@pytest.mark.parametrize("hash_fn", [0, 1])
@pytest.mark.parametrize("nk", [1, 2, 4])
def test_window_siblings_are_the_paths_of_a_rank_s_own_subtree(oracle, hash_fn, nk):
    """A rank that owns cosets [k0, k0 + nk) of 8 builds a tree over its own leaves only, leaf nk j + (k - k0); the siblings it reads there
    below the level of n nodes must be the bottom log2(nk) levels of the global path -- and each row's nk leaves a stand-alone tree."""
    n, b = 8, 8
    leaves = np.random.default_rng(8 * nk + hash_fn).integers(0, 256, size=(n * b, 32), dtype=np.uint8)
    nodes = oracle.merkle_build(leaves, hash_fn)
    log_nk = nk.bit_length() - 1
    for k0 in range(0, b, nk):
        own = leaves.reshape(n, b, 32)[:, k0:k0 + nk].reshape(n * nk, 32)
        heap = oracle.merkle_build(own, hash_fn) if n * nk > 1 else None
        for pos in range(n * b):
            j, k = divmod(pos, b)
            got = K.window_siblings(nodes, pos, k0, nk)
            if not k0 <= k < k0 + nk:
                assert got is None
                continue
            assert got.size == 4 * log_nk
            leaf = n * nk + nk * j + (k - k0)
            want = [heap[(leaf >> lvl) ^ 1] for lvl in range(log_nk)]
            assert got.tobytes() == b"".join(w.tobytes() for w in want), (k0, pos)
            if nk > 1:
                alone = oracle.merkle_build(leaves[b * j + k0:b * j + k0 + nk], hash_fn)
                assert got.tobytes() == b"".join(s.tobytes() for s in K.path_at(alone, k - k0)), (k0, pos)
                assert (alone[1] == nodes[(n * b + pos) >> log_nk]).all()
