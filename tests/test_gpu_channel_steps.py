"""GPU: the device-side Fiat-Shamir channel (csrc/channel.hip, k_chan_step) one step at a time on chosen inputs, against
oracle/verifier.py's Coin over oracle.digest: the seed of a transcript, the three kinds of absorb, the four layouts of drawn field
elements and the query positions with their folded lists.  A whole proof presents the kernel only the list lengths, draw counts and
domain sizes of the existing AIRs; here the lengths end inside a block, on a block, on a chunk and at the cap of 64 chunks, the draw
counts straddle the end of a pass of 512 candidates, and the query draw is steered into a third candidate pass, into the exhaustion
verdict and into folded lists longer than a wave.

Layouts restated from csrc/channel.h.  A drawn element is m consecutive draws; draw i = component q = i mod m of element e = i div m.
  CHAN_DRAW_LINEAR  out[i]
  CHAN_DRAW_COEFFS  2 a elements (alpha, beta) of the transition constraints, then 2 b of the assertions, in coefficient set q (out +
                    q set_stride): alpha_j at [j], beta_j at [stride + j], assertion alpha_j at [2 stride + j], beta_j at [2 stride + b + j]
  CHAN_DRAW_DEEP    per draws for each of a registers (alpha, beta, the rest unused): alpha_r at out[m r ..], beta_r at out[m (a + r) ..];
                    then b elements at out[m (2 a + j) ..]; then two elements at out2[3 m ..] and out2[4 m ..]
  CHAN_DRAW_POINT   one element z: out = z | z w | z^e as m-tuples (e = b), the same at out2[0 .. 3 m) if given
  CHAN_DRAW_QUERIES count distinct integers below 2^log_domain -> pos[0 .. count); layer l: first occurrences of the previous list mod
                    2^(log_domain - (l + 1) log_f) -> pos[slot (l + 1) ..], their number -> cnt[l + 1]; cnt[0] = count"""
import functools

import numpy as np
import pytest

import tail_cases as T
from tail_cases import P, mont

pytestmark = pytest.mark.gpu
SEED0 = T.tagged("chan-seed", 0)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def dev(oracle, backend):
    return T.Dev(backend)


def V():
    from oracle import verifier
    return verifier


def run(dev, seed, expect=T.HIP_SUCCESS, **kw):
    """one step on a coin standing at `seed` -> the seed written back"""
    seed_t = dev.raw(seed)
    assert dev.channel_step(seed_t, **kw) == expect
    return dev.get_raw(seed_t)


# ---- seed ---------------------------------------------------------------------------------------------------------------------------------
def public_inputs(npub):
    """canonical values: 0 and p - 1 first, then random ones, p - 1 last"""
    rng = np.random.default_rng(npub)
    vals = [0, P - 1] + [int(v) % P for v in rng.integers(0, 2**63, size=max(npub - 3, 0), dtype=np.uint64)] + [P - 1]
    return vals[:npub]


@pytest.mark.parametrize("prefix_len,npub", [(0, 0), (7, 1), (32, 4), (32, 14), (32, 124)])   # the last: exactly one chunk of 1024 bytes
def test_seed_of_a_transcript(dev, prefix_len, npub):
    prefix, pub = bytes(range(1, prefix_len + 1)), public_inputs(npub)
    coin = V().Coin(prefix + b"".join(T.le64(v) for v in pub))
    got = run(dev, b"\x55" * 32, init=1, prefix=prefix, npub=npub, pub=dev.u64([mont(v) for v in pub] + [T.NON_ELEMENT]))
    assert got == coin.seed
    # ... and the next step goes on from it
    coin.reseed_int(2**40 + 7)
    assert run(dev, got, absorbs=[(T.CHAN_INT, 0, None, 2**40 + 7, None)]) == coin.seed


def test_seed_too_long_is_refused(dev):
    pub = dev.u64([mont(3)] * 125)
    assert run(dev, SEED0, T.HIP_INVALID_VALUE, init=1, prefix=bytes(32), npub=125, pub=pub) == SEED0     # 1032 bytes
    assert run(dev, SEED0, T.HIP_INVALID_VALUE, init=1, prefix=bytes(33), npub=0, pub=pub) == SEED0
    assert run(dev, SEED0, T.HIP_INVALID_VALUE, init=0, prefix=bytes(33)) == SEED0                        # (the prefix table, init or not)
    for m in (0, 4):
        assert run(dev, SEED0, T.HIP_INVALID_VALUE, m=m) == SEED0


# ---- absorb -------------------------------------------------------------------------------------------------------------------------------
# chunks of 128 elements, blocks of 8: 1 chunk (empty, inside the first block, one short of a block, on it, one past; one short of the
# chunk, on it), 2 (one past, on the second), 3, 5, 7, 9, 32, 63 chunks on the chunk, 64 one short and on the cap
ELEM_COUNTS = [0, 1, 7, 8, 9, 127, 128, 129, 384, 640, 896, 1152, 4096, 8064, 8191, 8192]


@pytest.fixture(scope="module")
def lists(dev):
    """the two element lists (memory-form words), host and device: random words below p; all p - 1"""
    rng = np.random.default_rng(8193)
    rnd = (rng.integers(0, 2**63, size=8193, dtype=np.uint64) % np.uint64(P)).astype(np.uint64)
    rnd[:3] = [0, P - 1, 1]
    top = np.full(8193, P - 1, np.uint64)
    return [(rnd, dev.u64(rnd)), (top, dev.u64(top))]


@pytest.mark.parametrize("count", ELEM_COUNTS)
def test_absorb_element_list(dev, lists, count):
    for host, t in lists:
        coin, out_t = T.coin_at(SEED0), dev.raw(b"\xAA" * 40)
        d = T.elems_digest(host[:count])
        coin.reseed(d)
        assert run(dev, SEED0, absorbs=[(T.CHAN_ELEMS, count, t, 0, out_t)]) == coin.seed, count
        assert dev.get_raw(out_t) == d + b"\xAA" * 8


def test_absorb_list_over_the_cap_is_refused(dev, lists):
    for k in range(3):
        absorbs = [(0, 0, None, 0, None)] * k + [(T.CHAN_ELEMS, 8193, lists[0][1], 0, None)]
        assert run(dev, SEED0, T.HIP_INVALID_VALUE, absorbs=absorbs) == SEED0


def test_absorb_digest_and_integers(dev):
    d = T.tagged("chan-digest", 0)
    coin, out_t = T.coin_at(SEED0), dev.raw(b"\xAA" * 40)
    coin.reseed(d)
    assert run(dev, SEED0, absorbs=[(T.CHAN_DIGEST, 0, dev.raw(d), 0, out_t)]) == coin.seed
    assert dev.get_raw(out_t) == d + b"\xAA" * 8
    assert run(dev, SEED0, absorbs=[(T.CHAN_DIGEST, 0, dev.raw(d), 0, None)]) == coin.seed
    for v in (0, 1, 2**32 - 1, 2**32, 2**64 - 1):
        coin = T.coin_at(SEED0)
        coin.reseed_int(v)
        assert run(dev, SEED0, absorbs=[(T.CHAN_INT, 0, None, v, None)]) == coin.seed, v


def test_three_absorbs_in_order_and_a_step_that_continues(dev, lists):
    host, t = lists[0]
    d = T.tagged("chan-digest", 1)
    prefix, pub = b"three absorbs", public_inputs(4)
    pub_t, d_t = dev.u64([mont(v) for v in pub]), dev.raw(d)
    out0, out1 = dev.raw(b"\xAA" * 32), dev.raw(b"\xAA" * 32)
    coin = V().Coin(prefix + b"".join(T.le64(v) for v in pub))
    coin.reseed(T.elems_digest(host[:137]))
    coin.reseed(d)
    coin.reseed_int(2**32 + 5)
    absorbs = [(T.CHAN_ELEMS, 137, t, 0, out0), (T.CHAN_DIGEST, 0, d_t, 0, out1), (T.CHAN_INT, 0, None, 2**32 + 5, None)]
    seed1 = run(dev, b"\0" * 32, init=1, prefix=prefix, npub=4, pub=pub_t, absorbs=absorbs)
    assert seed1 == coin.seed
    assert dev.get_raw(out0) == T.elems_digest(host[:137]) and dev.get_raw(out1) == d
    # the other orders differ, so the order is observable
    other = [absorbs[1], absorbs[0], absorbs[2]]
    assert run(dev, b"\0" * 32, init=1, prefix=prefix, npub=4, pub=pub_t, absorbs=other) != seed1
    # a second step with init = 0 continues from the first step's seed; gaps in the absorb table are skipped
    coin.reseed(T.elems_digest(host[:1152]))
    coin.reseed_int(9)
    absorbs = [(T.CHAN_ELEMS, 1152, t, 0, None), (0, 0, None, 0, None), (T.CHAN_INT, 0, None, 9, None)]
    out_t = dev.u64([T.NON_ELEMENT] * 6)
    seed2 = run(dev, seed1, init=0, prefix=prefix, npub=4, pub=pub_t, absorbs=absorbs, draw=T.DRAW_LINEAR, count=4, out=out_t)
    assert seed2 == coin.seed
    assert dev.get_u64(out_t) == [mont(coin.draw()) for _ in range(4)] + [T.NON_ELEMENT] * 2


# ---- draws of field elements ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def draws(n, seed=SEED0):
    """the first n draws of a coin at `seed`, memory form (computed once for the largest n a test asks for, shared)"""
    coin = T.coin_at(seed)
    return tuple(mont(coin.draw()) for _ in range(n))


def first_draws(n):
    return list(draws(2200)[:n])


def linear(dev, ndraw, m):
    out_t = dev.u64([T.NON_ELEMENT] * (ndraw + 8))
    assert run(dev, SEED0, draw=T.DRAW_LINEAR, count=ndraw // m, m=m, out=out_t) == SEED0    # drawing leaves the seed alone
    return dev.get_u64(out_t)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_draw_linear(dev, m):
    """count m in {1, 3, 130, 512, 714, 2000}, rounded up to a multiple of m where m does not divide it: below one pass's yield (about
    131 of 512 candidates), around it, 16 passes"""
    for ndraw in (1, 3, 130, 512, 714, 2000):
        ndraw = (ndraw + m - 1) // m * m
        assert linear(dev, ndraw, m) == first_draws(ndraw) + [T.NON_ELEMENT] * 8, ndraw


def test_draw_count_at_the_end_of_a_pass(dev):
    """a request of exactly what one pass (two passes) of 512 candidates yields, one fewer and one more"""
    acc = T.accepted_offsets(SEED0, 1024)
    a1, a2 = len([k for k in acc if k < 512]), len(acc)
    assert 100 < a1 < 165 and 220 < a2 < 305            # (0.256 of 512: five standard deviations either way)
    for ndraw in (a1 - 1, a1, a1 + 1, a2 - 1, a2, a2 + 1):
        assert linear(dev, ndraw, 1) == first_draws(ndraw) + [T.NON_ELEMENT] * 8, ndraw


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("a,b", [(115, 4), (3, 2), (1, 0)])
def test_draw_coefficients(dev, a, b, m):
    stride, n = a + 3, 2 * (a + b)
    set_stride = 2 * stride + 2 * b + 5
    dr = first_draws(m * n)
    want = [T.NON_ELEMENT] * (m * set_stride + 8)
    for e in range(n):
        for q in range(m):
            if e < 2 * a:
                at = (e & 1) * stride + (e >> 1)
            else:
                r = e - 2 * a
                at = 2 * stride + (r & 1) * b + (r >> 1)
            want[q * set_stride + at] = dr[m * e + q]
    out_t = dev.u64([T.NON_ELEMENT] * len(want))
    assert run(dev, SEED0, draw=T.DRAW_COEFFS, count=n, a=a, b=b, stride=stride, set_stride=set_stride, m=m, out=out_t) == SEED0
    assert dev.get_u64(out_t) == want
    assert sum(w != T.NON_ELEMENT for w in want) == m * n


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("a,b,per", [(94, 8, 2), (2, 2, 3)])
def test_draw_deep_coefficients(dev, a, b, per, m):
    n = per * a + b + 2
    dr = first_draws(m * n)
    want, want2 = [T.NON_ELEMENT] * (m * (2 * a + b) + 4), [T.NON_ELEMENT] * (5 * m + 4)
    for e in range(n):
        for q in range(m):
            v = dr[m * e + q]
            if e < per * a:
                reg, k = divmod(e, per)
                if k == 0:
                    want[m * reg + q] = v
                elif k == 1:
                    want[m * (a + reg) + q] = v
            elif e - per * a < b:
                want[m * (2 * a + e - per * a) + q] = v
            else:
                want2[m * (3 + e - per * a - b) + q] = v
    out_t, out2_t = dev.u64([T.NON_ELEMENT] * len(want)), dev.u64([T.NON_ELEMENT] * len(want2))
    assert run(dev, SEED0, draw=T.DRAW_DEEP, count=n, a=a, b=b, per=per, m=m, out=out_t, out2=out2_t) == SEED0
    assert dev.get_u64(out_t) == want
    assert dev.get_u64(out2_t) == want2
    assert T.NON_ELEMENT not in want[:m * (2 * a + b)] and T.NON_ELEMENT not in want2[3 * m:5 * m]


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("with_out2,e", [(True, 8), (False, 2**32 - 1)])
def test_draw_point(dev, m, with_out2, e):
    wc = V().root_of_unity(10)
    z = tuple(T.canon(w) for w in first_draws(m))
    if m == 1:
        zw, ze = (z[0] * wc % P,), (pow(z[0], e, P),)
    else:
        zw, ze = V().e_scale(z, wc), V().e_pow(z, e)
    want = [mont(v) for v in z + tuple(zw) + tuple(ze)]
    out_t, out2_t = dev.u64([T.NON_ELEMENT] * (3 * m + 4)), dev.u64([T.NON_ELEMENT] * (5 * m + 4))
    assert run(dev, SEED0, draw=T.DRAW_POINT, count=1, b=e, w=mont(wc), m=m, out=out_t, out2=out2_t if with_out2 else None) == SEED0
    assert dev.get_u64(out_t) == want + [T.NON_ELEMENT] * 4
    assert dev.get_u64(out2_t) == (want if with_out2 else [T.NON_ELEMENT] * (3 * m)) + [T.NON_ELEMENT] * (2 * m + 4)
    assert run(dev, SEED0, T.HIP_INVALID_VALUE, draw=T.DRAW_POINT, count=2, b=e, w=mont(wc), m=m, out=out_t) == SEED0


# ---- query positions ------------------------------------------------------------------------------------------------------------------------
def folded_lists(positions, log_domain, log_f, n_layers):
    out, cur = [list(positions)], positions
    for l in range(n_layers):
        cur = V().fold_positions(cur, 1 << (log_domain - (l + 1) * log_f))
        out.append(cur)
    return out


def queries(dev, seed, count, log_domain, log_f, n_layers, slot, expect=T.HIP_SUCCESS):
    pos_t, cnt_t = dev.u32([T.NON_POSITION] * (slot * (n_layers + 1) + 8)), dev.u32([T.NON_POSITION] * 64)
    got = run(dev, seed, expect, draw=T.DRAW_QUERIES, count=count, log_domain=log_domain, log_f=log_f, n_layers=n_layers, slot=slot, pos=pos_t, cnt=cnt_t)
    assert got == seed
    return dev.get_u32(pos_t), dev.get_u32(cnt_t)


def check_queries(dev, seed, count, log_domain, log_f, n_layers):
    """-> the reference's lists"""
    slot = count + 5
    lists_ = folded_lists(T.coin_at(seed).draw_integers(count, 1 << log_domain), log_domain, log_f, n_layers)
    want = [T.NON_POSITION] * (slot * (n_layers + 1) + 8)
    for l, lst in enumerate(lists_):
        want[slot * l:slot * l + len(lst)] = lst
    pos, cnt = queries(dev, seed, count, log_domain, log_f, n_layers, slot)
    assert cnt == [len(lst) for lst in lists_] + [T.NON_POSITION] * (63 - n_layers)
    assert pos == want                                  # words beyond every layer's count included
    return lists_


QUERY_SHAPES = [(1, 9, 2, 1), (128, 9, 2, 1), (128, 8, 2, 0), (96, 13, 2, 3), (42, 14, 3, 2), (20, 14, 4, 2), (128, 31, 2, 4)]


@pytest.mark.parametrize("count,log_domain,log_f,n_layers", QUERY_SHAPES)
def test_query_positions_and_folded_lists(dev, count, log_domain, log_f, n_layers):
    lists_ = check_queries(dev, T.tagged("chan-q", 100 + log_domain), count, log_domain, log_f, n_layers)
    if (count, log_domain) in ((128, 9), (128, 31)):
        assert len(lists_[1]) > 64                      # the second entry per lane of the folding wave
    if (count, log_domain) == (128, 9):
        assert len(lists_[1]) < 128                     # ... and a fold that drops repeats


# i of tagged("chan-q", i), found by tail_cases.search("chan-q", wanted) over the first 1024 candidates of the coin; 128 distinct values
# of a domain of 128 points take 128 (ln 128 + 0.58) = 695 candidates on average, and 1024 do not suffice for 4 % of the seeds
THREE_PASSES, EXHAUSTED = 0, 50


def candidates_needed(seed, count, domain, cap):
    seen, order = set(), []
    for k, v in enumerate(T.candidates(seed, cap)):
        if v & (domain - 1) not in seen:
            seen.add(v & (domain - 1))
            order.append(v & (domain - 1))
        if len(order) == count:
            return k + 1, order
    return None, order


def test_query_draw_needs_a_third_candidate_pass(dev):
    seed = T.tagged("chan-q", THREE_PASSES)
    need, _ = candidates_needed(seed, 128, 128, 1024)
    T.require(need is not None and need > 512, "more than two passes of 256 candidates, at most four")
    lists_ = check_queries(dev, seed, 128, 7, 2, 1)
    assert sorted(lists_[0]) == list(range(128)) and lists_[1] == V().fold_positions(lists_[0], 32)


def test_query_draw_gives_up_after_1024_candidates(dev):
    seed = T.tagged("chan-q", EXHAUSTED)
    need, order = candidates_needed(seed, 128, 128, 1024)
    T.require(need is None and len(order) < 128, "1024 candidates do not hold 128 distinct values")
    pos, cnt = queries(dev, seed, 128, 7, 2, 1, 133)
    assert cnt[0] == 0xFFFFFFFF and cnt[2:] == [T.NON_POSITION] * 62
    assert pos[:len(order)] == order and pos[len(order):133] == [T.NON_POSITION] * (133 - len(order))


def test_query_requests_the_tables_cannot_hold_are_refused(dev):
    for count, log_domain, log_f, n_layers, slot in [(0, 9, 2, 1, 8), (129, 9, 2, 1, 256), (128, 9, 2, 1, 127), (20, 9, 2, 5, 32), (20, 9, 4, 3, 32),
                                                     (20, 32, 2, 1, 32)]:
        pos, cnt = queries(dev, SEED0, count, log_domain, log_f, n_layers, slot, T.HIP_INVALID_VALUE)
        assert set(pos) == {T.NON_POSITION} and set(cnt) == {T.NON_POSITION}
