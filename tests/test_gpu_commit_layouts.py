"""GPU: the row-hash and Merkle kernels on every layout the provers run them in, one call at a time through
include/cstark_debug_commit.h, against oracle.hash_rows / oracle.merkle_build of the natural-order table, bit for bit.
test_gpu_commit.py pins the plain form (natural coset order, one table, Blake3 trees of every size); here: tables in BLOCK ORDER
(csrc/blake3.h; the trace table of every proof whose blowup exceeds the AIR's constraint blowup) through both Blake3 kernels and the
Sha3 kernel, whole and windowed; the claim about the extension that block order rests on; row widths on both sides of the kernels' own
boundaries; Sha3 trees of every size; the batched tables and trees of the batched range prover at every group width.

Every output buffer is filled with 0xA5 first and checked whole: the bytes a call does not own must still be 0xA5."""
import numpy as np
import pytest

import commit_cases as K
from commit_cases import FILL, P

pytestmark = pytest.mark.gpu
GUARD = 96   # bytes behind every output buffer that nothing may touch


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def dev(oracle, backend):
    return K.CommitDev(backend)


def random_table(seed, b, width, n):
    """memory-form words below p, [b][width][n]"""
    return np.random.default_rng(seed).integers(0, P, size=(b, width, n), dtype=np.uint64)


def hash_whole_table(dev, hash_fn, table, log_s):
    """the table as the kernel reads it -> (leaves [N][32], guard bytes)"""
    b, width, n = table.shape
    log_n, log_b = n.bit_length() - 1, b.bit_length() - 1
    out = dev.filled(32 * n * b + GUARD)
    assert dev.hash_rows_slots(hash_fn, dev.u64(table), out, width, log_n, log_b, log_s, 0, b) == K.HIP_SUCCESS
    got = dev.bytes_of(out)
    return got[:32 * n * b].reshape(n * b, 32), got[32 * n * b:]


# ---- block order ----------------------------------------------------------------------------------------------------------------------------
# (94, 8, 4, 1) and (17, 6, 4, 2): the lane-per-row kernel; the widths up to 16: the lane-per-leaf kernel; Sha3: one kernel for all
BLOCK_ORDER_SHAPES = [(94, 8, 4, 1), (2, 6, 4, 3), (2, 6, 3, 2), (14, 7, 3, 1), (17, 6, 4, 2), (16, 6, 2, 1), (1, 6, 1, 1), (3, 6, 2, 2)]


@pytest.mark.parametrize("hash_fn", [0, 1])
@pytest.mark.parametrize("width,log_n,log_b,log_s", BLOCK_ORDER_SHAPES)
def test_block_order_gives_the_natural_leaves(oracle, dev, hash_fn, width, log_n, log_b, log_s):
    natural = random_table(1000 * width + 10 * log_b + log_s, 1 << log_b, width, 1 << log_n)
    s, ce = 1 << log_s, 1 << (log_b - log_s)
    slots = np.empty_like(natural)
    for k in range(1 << log_b):
        slots[(k % s) * ce + k // s] = natural[k]            # the formula of csrc/blake3.h, written out
    leaves, guard = hash_whole_table(dev, hash_fn, slots, log_s)
    assert (leaves == oracle.hash_rows(natural, log_b, hash_fn=hash_fn)).all()
    assert (guard == FILL).all()


@pytest.mark.parametrize("hash_fn", [0, 1])
@pytest.mark.parametrize("k0,nk", [(0, 4), (4, 4), (2, 1), (5, 3)])
def test_block_order_window_writes_its_cosets_only(oracle, dev, hash_fn, k0, nk):
    """slots [k0, k0 + nk) of a table in block order: exactly the leaves of the cosets those slots hold"""
    width, log_n, log_b, log_s = 7, 6, 3, 1
    n, b = 1 << log_n, 1 << log_b
    natural = random_table(70 + k0, b, width, n)
    slots = K.to_slots(natural, log_s)
    ref = oracle.hash_rows(natural, log_b, hash_fn=hash_fn).reshape(n, b, 32)
    out = dev.filled(32 * n * b + GUARD)
    assert dev.hash_rows_slots(hash_fn, dev.u64(slots[k0:k0 + nk]), out, width, log_n, log_b, log_s, k0, nk) == K.HIP_SUCCESS
    got = dev.bytes_of(out)
    leaves = got[:32 * n * b].reshape(n, b, 32)
    owned = sorted(K.slot_coset(k0 + kk, log_b, log_s) for kk in range(nk))
    assert owned == sorted((v % 4) * 2 + v // 4 for v in range(k0, k0 + nk))       # log_s = 1, ce = 4, written out
    for k in range(b):
        if k in owned:
            assert (leaves[:, k] == ref[:, k]).all(), k
        else:
            assert (leaves[:, k] == FILL).all(), k
    assert (got[32 * n * b:] == FILL).all()


def test_hash_rows_refusals_write_nothing(dev):
    table, out = dev.u64(random_table(1, 8, 7, 64)), dev.filled(32 * 512)
    bad = [dict(width=0), dict(width=129), dict(log_s=4), dict(k0=8, nk=1), dict(k0=6, nk=3), dict(nk=0), dict(log_b=5), dict(hash_fn=2),
           dict(width=8), dict(log_n=7)]   # the last two: the stated buffers are too small for the shape
    for change in bad:
        a = dict(hash_fn=0, width=7, log_n=6, log_b=3, log_s=1, k0=0, nk=8)
        a.update(change)
        rc = dev.hash_rows_slots(a["hash_fn"], table, out, a["width"], a["log_n"], a["log_b"], a["log_s"], a["k0"], a["nk"])
        assert rc == K.HIP_INVALID_VALUE, change
    assert (dev.bytes_of(out) == FILL).all()


# ---- the extension behind block order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_b,log_ce", [(4, 3), (3, 1), (4, 2)])
def test_lde_blocks_are_the_cosets_of_a_residue(oracle, backend, log_b, log_ce):
    """csrc/blake3.h: block r of a table in block order, i.e. the blowup-ce extension with offset g w_(b n)^r, IS the cosets k = r (mod s)
    of the blowup-b extension -- what lde_trace (csrc/prove.hip) builds the trace table from"""
    from certificate_stark_amd.backend import to_numpy_u64
    log_n, width = 8, 3
    s, ce = 1 << (log_b - log_ce), 1 << log_ce
    coeffs = np.random.default_rng(log_b * 10 + log_ce).integers(0, P, size=(width, 1 << log_n), dtype=np.uint64)
    full = to_numpy_u64(backend.lde_columns(backend.from_numpy_u64(coeffs), log_b))
    assert (full == oracle.lde_columns(coeffs, log_b)).all()
    g = np.array([backend.field_lde_offset()], np.uint64)
    w = np.array([oracle.root_of_unity(log_n + log_b)], np.uint64)
    for r in range(s):
        offset = int(oracle.fp_mul(g, oracle.fp_pow(w, r))[0])
        block = to_numpy_u64(backend.lde_columns(backend.from_numpy_u64(coeffs), log_ce, offset=offset))
        assert block.shape == (ce, width, 1 << log_n)
        for i in range(ce):
            assert (block[i] == full[i * s + r]).all(), (r, i)


# ---- widths and blowups at the kernels' own boundaries, natural order -------------------------------------------------------------------------
# Blake3: lane per leaf up to 16 columns (and only with more than one coset), lane per row above; 8 columns per compression.
# Sha3: 17 columns per block, an empty padding block behind a multiple of 17 (119 = 7 x 17 is the widest), 127 = 7 blocks + 8.
@pytest.mark.parametrize("hash_fn,width", [(0, 15), (0, 16), (0, 17), (0, 24), (1, 51), (1, 119), (1, 127)])
@pytest.mark.parametrize("log_n,log_b", [(9, 0), (6, 4)])
def test_row_width_and_blowup_boundaries(oracle, dev, hash_fn, width, log_n, log_b):
    table = random_table(width * 10 + log_b, 1 << log_b, width, 1 << log_n)
    leaves, guard = hash_whole_table(dev, hash_fn, table, 0)
    assert (leaves == oracle.hash_rows(table, log_b, hash_fn=hash_fn)).all()
    assert (guard == FILL).all()


@pytest.mark.parametrize("hash_fn,width,log_b", [(0, 24, 1), (0, 16, 1), (1, 51, 1)])
def test_rows_of_extreme_words(oracle, dev, hash_fn, width, log_b):
    """memory-form words at the ends of the field and of the Montgomery form (the hashed bytes are a conversion of them): every row a
    rotation of the list, then a row of zeros and a row of p - 1"""
    n, b = 64, 1 << log_b
    ext = np.array(K.EXTREME_WORDS, np.uint64)
    idx = (np.arange(b)[:, None, None] * 5 + np.arange(width)[None, :, None] + np.arange(n)[None, None, :]) % ext.size
    table = ext[idx]
    table[:, :, n - 2] = 0
    table[:, :, n - 1] = P - 1
    assert set(K.EXTREME_WORDS) <= set(int(v) for v in table.reshape(-1)) and int(table.max()) < P
    leaves, guard = hash_whole_table(dev, hash_fn, table, 0)
    assert (leaves == oracle.hash_rows(table, log_b, hash_fn=hash_fn)).all()
    assert (guard == FILL).all()


# ---- Sha3 trees -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_leaves", list(range(1, 14)))
def test_sha3_tree_every_size(oracle, backend, dev, log_leaves):
    """up to 2^11 leaves the one-workgroup kernel alone; 2^12 and 2^13: one and two launches of k_merkle_level_sha3 below it"""
    import torch
    L = 1 << log_leaves
    leaves = np.random.default_rng(300 + log_leaves).integers(0, 256, size=(L, 32), dtype=np.uint8)
    buf = dev.filled(64 * L + GUARD)
    buf[32 * L:64 * L] = torch.from_numpy(leaves.reshape(-1)).to(backend.device)
    backend.merkle_build_fn(1, buf[:64 * L].view(2 * L, 32))
    got = dev.bytes_of(buf)
    assert (got[:64 * L].reshape(2 * L, 32) == oracle.merkle_build(leaves, 1)).all()     # node 0 included: zeros
    assert (got[64 * L:] == FILL).all()


# ---- batched tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_fn", [0, 1])
@pytest.mark.parametrize("gw", list(range(1, 9)))
def test_batched_tables_and_trees(oracle, dev, hash_fn, gw):
    """table t = columns [t gw, (t + 1) gw) of one wide table; its tree at a stride larger than the tree: the gap stays untouched"""
    for log_n, log_b in [(6, 3), (7, 0), (6, 1)]:
        for batch in (1, 5):
            n, b = 1 << log_n, 1 << log_b
            L, gap = n * b, 64
            stride = 64 * L + gap
            table = random_table(gw * 100 + log_n * 10 + log_b + batch, b, gw * batch, n)
            out = dev.filled(batch * stride + GUARD)
            assert dev.commit_batch(hash_fn, dev.u64(table), out, gw, log_n, log_b, batch, stride) == K.HIP_SUCCESS
            got = dev.bytes_of(out)
            for t in range(batch):
                part = np.ascontiguousarray(table[:, t * gw:(t + 1) * gw])
                ref = oracle.merkle_build(oracle.hash_rows(part, log_b, hash_fn=hash_fn), hash_fn)
                mine = got[t * stride:(t + 1) * stride]
                assert (mine[:64 * L].reshape(2 * L, 32) == ref).all(), (log_n, log_b, batch, t)
                assert (mine[64 * L:] == FILL).all(), (log_n, log_b, batch, t)
            assert (got[batch * stride:] == FILL).all()


@pytest.mark.parametrize("hash_fn", [0, 1])
@pytest.mark.parametrize("log_leaves", list(range(1, 12)))
def test_batched_trees_every_size(oracle, backend, dev, hash_fn, log_leaves):
    """the tree-only form on leaves already in place, three trees side by side, one of them at the tightest stride"""
    import torch
    L, batch = 1 << log_leaves, 3
    for stride in (64 * L, 64 * L + 32):
        leaves = np.random.default_rng(500 + log_leaves).integers(0, 256, size=(batch, L, 32), dtype=np.uint8)
        out = dev.filled(batch * stride + GUARD)
        for t in range(batch):
            out[t * stride + 32 * L:t * stride + 64 * L] = torch.from_numpy(leaves[t].reshape(-1)).to(backend.device)
        assert dev.merkle_batch(hash_fn, out, log_leaves, batch, stride) == K.HIP_SUCCESS
        got = dev.bytes_of(out)
        for t in range(batch):
            mine = got[t * stride:(t + 1) * stride]
            assert (mine[:64 * L].reshape(2 * L, 32) == oracle.merkle_build(leaves[t], hash_fn)).all(), t
            assert (mine[64 * L:] == FILL).all(), t
        assert (got[batch * stride:] == FILL).all()


@pytest.mark.parametrize("hash_fn", [0, 1])
def test_batched_refusals_write_nothing(dev, hash_fn):
    table = dev.u64(random_table(9, 16, 9 * 2, 256))           # large enough for every shape below: a refusal is about the shape
    out = dev.filled(2 * (64 << 12))
    ok = dict(gw=2, log_n=6, log_b=3, batch=2)
    for change in [dict(gw=0), dict(gw=9), dict(batch=0), dict(log_n=0, log_b=0), dict(log_n=8, log_b=4), dict(log_n=9, log_b=3)]:
        a = dict(ok, **change)
        stride = 64 << (a["log_n"] + a["log_b"])
        assert dev.commit_batch(hash_fn, table, out, a["gw"], a["log_n"], a["log_b"], a["batch"], stride) == K.HIP_INVALID_VALUE, change
    for log_leaves, batch in [(0, 2), (12, 2), (9, 0)]:
        assert dev.merkle_batch(hash_fn, out, log_leaves, batch, 64 << max(log_leaves, 1)) == K.HIP_INVALID_VALUE, (log_leaves, batch)
    # a stride below the tree, an odd stride, a buffer that ends inside the last tree
    assert dev.merkle_batch(hash_fn, out, 9, 2, (64 << 9) - 32) == K.HIP_INVALID_VALUE
    assert dev.merkle_batch(hash_fn, out, 9, 2, (64 << 9) + 16) == K.HIP_INVALID_VALUE
    assert dev.merkle_batch(hash_fn, out, 11, 5, 64 << 11) == K.HIP_INVALID_VALUE
    assert (dev.bytes_of(out) == FILL).all()
