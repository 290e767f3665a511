"""GPU: the public coin of a FRI layer on the device (csrc/blake3.hip k_fri_coin, k_fri_coin_ext) on chosen (seed, root) pairs against
oracle/verifier.py's Coin: reseed with the root, then one draw (base field) or m draws (extension).  The kernels try sixteen counters
per pass; a whole proof reaches their second pass by chance (0.9 % of base-field layers) -- here the pairs are steered so that the
first acceptance falls on the first and the last counter of a pass, into the second and the third pass, and so that the first pass of
the extension coin accepts 0, 1, 2, exactly m and more than m candidates."""
import numpy as np
import pytest

import tail_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def dev(oracle, backend):
    return T.Dev(backend)


def pair(i):
    """steered pair i: the coin's seed and the layer root"""
    return T.tagged("fri-seed", i), T.tagged("fri-root", i)


def reseeded(i):
    seed, root = pair(i)
    return T.H(seed + root)


def first_pass(i):
    """offsets of the counters of the first pass (sixteen) that the reference accepts"""
    return T.accepted_offsets(reseeded(i), 16)


def first_accepted(i, n):
    acc = T.accepted_offsets(reseeded(i), n)
    return acc[0] if acc else n


def run(dev, m, seed, root):
    """-> (new seed, root_out, alpha words [m]) with the words behind alpha checked untouched"""
    seed_t, root_t = dev.raw(seed), dev.raw(root)
    alpha_t, out_t = dev.u64([T.NON_ELEMENT] * (m + 2)), dev.raw(b"\xAA" * 32)
    assert dev.fri_coin(m, seed_t, root_t, alpha_t, out_t) == T.HIP_SUCCESS
    alpha = dev.get_u64(alpha_t)
    assert alpha[m:] == [T.NON_ELEMENT] * 2, "words behind the m drawn ones were written"
    assert dev.get_raw(root_t) == root
    return dev.get_raw(seed_t), dev.get_raw(out_t), alpha[:m]


def check(dev, m, seed, root):
    coin = T.coin_at(seed)
    coin.reseed(root)
    want = [T.mont(coin.draw()) for _ in range(m)]
    new_seed, root_out, alpha = run(dev, m, seed, root)
    assert new_seed == coin.seed
    assert root_out == root
    assert alpha == want
    return coin.counter - T.first_counter()   # offset of the last counter the reference consumed


@pytest.mark.parametrize("m", [1, 2, 3])
def test_random_pairs(dev, m):
    """64 pairs: the new seed, the copied root and the m drawn words equal Coin.reseed + draw"""
    rng = np.random.default_rng(1900 + m)
    for _ in range(64):
        check(dev, m, rng.bytes(32), rng.bytes(32))


# Steered pairs: i of pair(i), found by
#   next(i for i in range(1 << 20) if wanted(i))
# with the properties re-derived below (the third pass: one pair in 13 000, found after 0.9 s of search).
FIRST_AT_0, FIRST_AT_15, SECOND_PASS, THIRD_PASS = 3, 313, 0, 4781


def test_base_coin_first_and_last_counter_of_a_pass(dev):
    T.require(first_accepted(FIRST_AT_0, 16) == 0, "first acceptance at offset 0")
    T.require(first_accepted(FIRST_AT_15, 16) == 15, "first acceptance at offset 15")
    assert check(dev, 1, *pair(FIRST_AT_0)) == 0
    assert check(dev, 1, *pair(FIRST_AT_15)) == 15


def test_base_coin_second_and_third_pass(dev):
    """sixteen (thirty-two) rejections first: counter += 16 and the selection of the first accepted candidate across passes"""
    T.require(16 <= first_accepted(SECOND_PASS, 32) < 32, "first acceptance in the second pass")
    T.require(32 <= first_accepted(THIRD_PASS, 48) < 48, "first acceptance in the third pass")
    assert 16 <= check(dev, 1, *pair(SECOND_PASS)) < 32
    assert 32 <= check(dev, 1, *pair(THIRD_PASS)) < 48
    # the same pairs through the extension coin: its first pass (two first passes) accepts nothing
    for m in (2, 3):
        check(dev, m, *pair(SECOND_PASS))
        check(dev, m, *pair(THIRD_PASS))


# the first and the last counter of the second pass: a pass that starts one counter late or ends one early loses exactly these
FIRST_AT_16, FIRST_AT_31 = 18, 20330


def test_base_coin_edges_of_the_second_pass(dev):
    T.require(first_accepted(FIRST_AT_16, 17) == 16, "first acceptance at offset 16")
    T.require(first_accepted(FIRST_AT_31, 32) == 31, "first acceptance at offset 31")
    assert check(dev, 1, *pair(FIRST_AT_16)) == 16
    assert check(dev, 1, *pair(FIRST_AT_31)) == 31
    for m in (2, 3):
        check(dev, m, *pair(FIRST_AT_16))
        check(dev, m, *pair(FIRST_AT_31))


# first pass of the extension coin accepts exactly 0, 1, 2, 3 and at least 5 candidates
EXT_FIRST_PASS = {0: 0, 1: 25, 2: 1, 3: 2}
EXT_FIRST_PASS_5 = 3


def test_cubic_coin_by_acceptances_of_the_first_pass(dev):
    for n, i in EXT_FIRST_PASS.items():
        T.require(len(first_pass(i)) == n, "%d acceptances in the first pass" % n)
        last = check(dev, 3, *pair(i))
        assert (last < 16) == (n >= 3)
    T.require(len(first_pass(EXT_FIRST_PASS_5)) >= 5, "at least 5 acceptances in the first pass")
    assert check(dev, 3, *pair(EXT_FIRST_PASS_5)) < 15   # candidates of the pass behind the third accepted one are dropped


def test_quadratic_coin_completed_in_the_second_pass(dev):
    i = EXT_FIRST_PASS[1]
    T.require(len(first_pass(i)) == 1, "1 acceptance in the first pass")
    assert check(dev, 2, *pair(i)) >= 16
    for n in (2, 3):                                          # exactly m, more than m
        check(dev, 2, *pair(EXT_FIRST_PASS[n]))
    check(dev, 2, *pair(EXT_FIRST_PASS_5))


def test_extension_degree_is_checked(dev):
    seed, root = pair(1)
    for m in (0, 4):
        seed_t = dev.raw(seed)
        alpha_t = dev.u64([T.NON_ELEMENT] * 4)
        assert dev.fri_coin(m, seed_t, dev.raw(root), alpha_t, dev.raw(b"\0" * 32)) == T.HIP_INVALID_VALUE
        assert dev.get_raw(seed_t) == seed and dev.get_u64(alpha_t) == [T.NON_ELEMENT] * 4
