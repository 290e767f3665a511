"""GPU: the opening kernels on positions of the test's choice.  Inside a proof the positions come from Fiat-Shamir, so an index or stride
error at position 0 or N - 1, on a sibling pair, across the cosets of one row or on a duplicate would show only if a drawn position
happened to land there.  Here k_gather_batch (csrc/prove.hip: all opening gathers of a proof in one launch), k_rb_open
(csrc/range_batch.hip) and k_gather_rows_window (the sharded prover's rows with their subtree siblings) open known tables at steered
positions, through include/cstark_debug_commit.h and cstark_tx_shard_open_rows, and every byte of the output is compared with plain numpy
indexing (tests/commit_cases.py, itself checked by test_open_reference_cpu.py); what a call does not own must still be 0xA5."""
import numpy as np
import pytest

import commit_cases as K
from commit_cases import FILL, P

pytestmark = pytest.mark.gpu
GUARD = 64


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
    return np.random.default_rng(seed).integers(0, P, size=(b, width, n), dtype=np.uint64)


# ---- k_gather_batch: one launch, many jobs -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables(oracle):
    """name -> (natural table, the table the kernel reads, log_s); trees: (name, hash_fn) -> node array over the natural-order leaves"""
    nat = {"trace": random_table(1, 8, 94, 64), "blocks": random_table(2, 16, 94, 64), "comp": random_table(3, 8, 8, 64),
           "column": random_table(4, 4, 1, 128), "layer": random_table(5, 1, 4, 128)}
    tabs = {name: (t, t, 0) for name, t in nat.items()}
    tabs["blocks"] = (nat["blocks"], K.to_slots(nat["blocks"], 1), 1)
    trees = {}
    for name in ("trace", "blocks", "layer"):
        for hash_fn in (0, 1):
            log_b = nat[name].shape[0].bit_length() - 1
            trees[name, hash_fn] = oracle.merkle_build(oracle.hash_rows(nat[name], log_b, hash_fn=hash_fn), hash_fn)
    return tabs, trees


# (kind, source, count, dcount, lvl0): counts 1, 7, 128 and 0 side by side, jobs of each kind with a device-side count below their
# own, paths that start at level 0, 1, 2 and at the top (nothing to write)
JOB_MIX = [("rows", "trace", 128, -1, 0), ("paths", "trace", 128, -1, 0), ("rows", "blocks", 128, -1, 0), ("paths", "blocks", 128, -1, 1),
           ("rows", "comp", 7, -1, 0), ("paths", "trace", 7, -1, 2), ("rows", "column", 1, -1, 0), ("paths", "layer", 7, -1, 7),
           ("rows", "layer", 128, 40, 0), ("paths", "layer", 128, 40, 0), ("rows", "comp", 0, -1, 0), ("paths", "trace", 0, -1, 0),
           ("rows", "trace", 7, 0, 0), ("paths", "blocks", 1, -1, 0), ("paths", "blocks", 7, 3, 10), ("rows", "column", 128, 128, 0)]


def build_jobs(dev, tables, hash_fn, spec):
    """-> (jobs for CommitDev.gather, expected bytes of every output buffer)"""
    tabs, trees = tables
    dev_tabs = {name: dev.u64(t[1]) for name, t in tabs.items()}
    dev_trees = {name: dev.u8(trees[name, hash_fn]) for name in ("trace", "blocks", "layer")}
    jobs, expected = [], []
    for kind, name, count, dcount, lvl0 in spec:
        natural, read, log_s = tabs[name]
        b, width, n = natural.shape
        rng = np.random.default_rng(900 + 1000 * len(name) + count)       # (jobs of one table and count share their positions)
        pos = K.steered_positions(b * n, b, rng, count)
        live = count if dcount < 0 else dcount
        if kind == "rows":
            want = np.full(count * width * 8 + GUARD, FILL, np.uint8)
            rows = K.rows_at(read, pos[:live], log_s) if live else np.zeros((0, width), np.uint64)
            assert all((rows[q] == natural[p % b, :, p // b]).all() for q, p in enumerate(pos[:live]))   # block order or not: the natural row
            want[:live * width * 8] = rows.reshape(-1).view(np.uint8)
            job = dict(src=dev_tabs[name], positions=pos, out=dev.filled(want.size), width=width, log_n=n.bit_length() - 1, log_b=b.bit_length() - 1,
                       log_s=log_s)
        else:
            nodes = trees[name, hash_fn]
            log_leaves = (b * n).bit_length() - 1
            want = np.full(count * log_leaves * 32 + GUARD, FILL, np.uint8)
            view = want[:count * log_leaves * 32].reshape(count, log_leaves, 32)
            for q, p in enumerate(pos[:live]):
                for lvl, sib in zip(range(lvl0, log_leaves), K.path_at(nodes, p, lvl0)):
                    view[q, lvl] = sib
            job = dict(src=dev_trees[name], positions=pos, out=dev.filled(want.size), log_leaves=log_leaves, lvl0=lvl0)
        if dcount >= 0:
            job["dcount"] = dcount
        jobs.append(job)
        expected.append(want)
    return jobs, expected


@pytest.mark.parametrize("hash_fn", [0, 1])
def test_many_jobs_in_one_launch(oracle, dev, tables, hash_fn):
    spec = JOB_MIX
    jobs, expected = build_jobs(dev, tables, hash_fn, spec)
    assert dev.gather(jobs) == K.HIP_SUCCESS
    for i, (job, want) in enumerate(zip(jobs, expected)):
        got = dev.bytes_of(job["out"])
        assert (got == want).all(), (i, spec[i], np.flatnonzero(got != want)[:8])
    # commitment and opening together: the digest of every opened trace row, folded up its opened path, is the root
    root = tables[1]["trace", hash_fn][1]
    rows = dev.bytes_of(jobs[0]["out"])[:128 * 94 * 8].view(np.uint64).reshape(128, 94)
    paths = dev.bytes_of(jobs[1]["out"])[:128 * 9 * 32].reshape(128, 9, 32)
    assert jobs[0]["positions"] == jobs[1]["positions"]
    seen = set()
    for q, p in enumerate(jobs[0]["positions"]):
        if p in seen:
            continue
        seen.add(p)
        digest = oracle.hash_rows(np.ascontiguousarray(rows[q].reshape(1, 94, 1)), 0, hash_fn=hash_fn)[0]
        assert (K.fold_path(digest, p, list(paths[q]), hash_fn, oracle) == root).all(), p
    assert {0, 511, 1, 510} <= set(jobs[0]["positions"])


def test_single_jobs_and_all_32(dev, tables):
    """every job of the mix on its own (its count is then the grid's), and 32 jobs in one launch"""
    spec = JOB_MIX
    for one in spec:
        jobs, expected = build_jobs(dev, tables, 0, [one])
        assert dev.gather(jobs) == K.HIP_SUCCESS
        got = dev.bytes_of(jobs[0]["out"])
        assert (got == expected[0]).all(), one
    jobs, expected = build_jobs(dev, tables, 0, spec + spec)
    assert len(jobs) == 32 and dev.gather(jobs) == K.HIP_SUCCESS
    for i, (job, want) in enumerate(zip(jobs, expected)):
        assert (dev.bytes_of(job["out"]) == want).all(), i


def test_gather_refusals_launch_nothing(dev, tables):
    spec = JOB_MIX
    good = spec[:6]

    def refused(jobs):
        assert dev.gather(jobs) == K.HIP_INVALID_VALUE
        for job in jobs:
            assert (dev.bytes_of(job["out"]) == FILL).all()

    for victim, domain in [(0, 512), (1, 512), (2, 1024), (3, 1024), (4, 512)]:      # a position one past the domain, rows and paths
        jobs, _ = build_jobs(dev, tables, 0, good)
        jobs[victim]["positions"] = jobs[victim]["positions"][:-1] + [domain]
        refused(jobs)
        jobs[victim]["positions"] = [2**32 - 1] + jobs[victim]["positions"][1:]
        refused(jobs)
    jobs, _ = build_jobs(dev, tables, 0, good)
    jobs[4]["dcount"] = 8                                                             # above its count of 7
    refused(jobs)
    jobs, _ = build_jobs(dev, tables, 0, good)
    jobs[3]["lvl0"] = 11                                                              # above the top of a tree of 2^10 leaves
    refused(jobs)
    jobs, _ = build_jobs(dev, tables, 0, good)
    jobs[2]["log_b"] = 5
    refused(jobs)
    jobs, _ = build_jobs(dev, tables, 0, good)
    jobs[0]["log_n"] = 7                                                              # the table is too small for the stated shape
    refused(jobs)
    jobs, _ = build_jobs(dev, tables, 0, spec + spec + spec[:1])                      # 33 jobs
    refused(jobs)
    assert dev.gather([]) == K.HIP_INVALID_VALUE


# ---- k_rb_open ----------------------------------------------------------------------------------------------------------------------------------
def rb_case(dev, batch, n_layers, lcount, seed=0):
    """random tables and node arrays of the batched range prover's shapes, steered positions -> (arguments, expected output bytes)"""
    rng = np.random.default_rng(40 + 7 * batch + n_layers + seed)
    nq = 5
    lde, clde = random_table(rng.integers(1 << 30), 8, 2 * batch, 64), random_table(rng.integers(1 << 30), 8, 2 * batch, 64)
    layer = rng.integers(0, P, size=(batch, 512), dtype=np.uint64)
    tnodes, cnodes = [rng.integers(0, 256, size=(batch, 1024, 32), dtype=np.uint8) for _ in range(2)]
    lnodes = rng.integers(0, 256, size=(batch, 256, 32), dtype=np.uint8)
    pos, lpos = np.zeros((batch, nq), np.uint32), np.zeros((batch, nq), np.uint32)
    for t in range(batch):
        i, m = int(rng.integers(1, 255)), int(rng.integers(1, 63))
        pos[t] = np.roll([0, 511, 2 * i, 2 * i + 1, 2 * i], t)           # both ends, a sibling pair, a duplicate
        lpos[t] = np.roll([127, 0, 2 * m + 1, 2 * m, 127], t)
    # the sections of a slot with gaps between them and behind the last
    sizes = [nq * 16, nq * 9 * 32, nq * 16, nq * 9 * 32, nq * 32, nq * 7 * 32]
    offsets, at = [], 16
    for s in sizes:
        offsets.append(at)
        at += s + 16
    slot = at + 16
    want = np.full(batch * slot + GUARD, FILL, np.uint8)
    for t in range(batch):
        mine = want[t * slot:(t + 1) * slot]
        sec = [mine[o:o + s] for o, s in zip(offsets, sizes)]
        for q in range(nq):
            p = int(pos[t, q])
            k, j = p % 8, p // 8
            sec[0].view(np.uint64).reshape(nq, 2)[q] = lde[k, 2 * t:2 * t + 2, j]
            sec[2].view(np.uint64).reshape(nq, 2)[q] = clde[k, 2 * t:2 * t + 2, j]
            sec[1].reshape(nq, 9, 32)[q] = K.path_at(tnodes[t], p)[:9]     # (the node arrays hold 512 leaves: nine levels)
            sec[3].reshape(nq, 9, 32)[q] = K.path_at(cnodes[t], p)[:9]
            if n_layers and q < lcount[t]:
                lp = int(lpos[t, q])
                sec[4].view(np.uint64).reshape(nq, 4)[q] = [layer[t, lp + 128 * i] for i in range(4)]
                sec[5].reshape(nq, 7, 32)[q] = K.path_at(lnodes[t], lp)[:7]
    out = dev.filled(want.size)
    args = dict(lde=dev.u64(lde), clde=dev.u64(clde), layer=dev.u64(layer) if n_layers else None, tnodes=dev.u8(tnodes), cnodes=dev.u8(cnodes),
                lnodes=dev.u8(lnodes) if n_layers else None, pos=pos, lpos=lpos if n_layers else None,
                lcount=np.array(lcount, np.uint32) if n_layers else None, out=out, nq=nq, batch=batch, n_layers=n_layers, slot=slot, offsets=offsets)
    return args, want


@pytest.mark.parametrize("n_layers", [0, 1])
@pytest.mark.parametrize("batch,lcounts", [(1, [(0, ), (5, ), (2, )]), (3, [(0, 5, 2)])])
def test_range_batch_openings(dev, batch, lcounts, n_layers):
    for lcount in lcounts:
        args, want = rb_case(dev, batch, n_layers, lcount)
        assert dev.range_open(**args) == K.HIP_SUCCESS
        got = dev.bytes_of(args["out"])
        assert (got == want).all(), (lcount, np.flatnonzero(got != want)[:8])


def test_range_batch_open_refusals(dev):
    def refused(args):
        assert dev.range_open(**args) == K.HIP_INVALID_VALUE
        assert (dev.bytes_of(args["out"]) == FILL).all()

    args, _ = rb_case(dev, 3, 1, (0, 5, 2))
    args["pos"][2, 4] = 512
    refused(args)
    args, _ = rb_case(dev, 3, 1, (0, 5, 2))
    args["lpos"][1, 0] = 128
    refused(args)
    args, _ = rb_case(dev, 3, 1, (0, 6, 2))
    refused(args)
    args, _ = rb_case(dev, 3, 1, (0, 5, 2))
    args["batch"] = 4                                   # tables, node arrays and the output hold three proofs
    args["pos"], args["lpos"], args["lcount"] = [np.concatenate([a, a[:1]]) for a in (args["pos"], args["lpos"], args["lcount"])]
    refused(args)
    args, _ = rb_case(dev, 3, 1, (0, 5, 2))
    args["offsets"][5] = args["slot"] - 32              # the last section would end behind its slot
    refused(args)
    args, _ = rb_case(dev, 3, 1, (0, 5, 2))
    args["n_layers"] = 2
    refused(args)


# ---- k_gather_rows_window: the sharded prover's rows with the siblings of the rank's own subtree ---------------------------------------------
SHARD_OPTS = (42, 8, 0, 0, 0, 4, 256)


@pytest.fixture(scope="module")
def shard_reference(oracle):
    """4 transfers at depth 3: the witness, the whole extended trace and its global tree from the oracle, the single-GPU proof"""
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import ProofOptions, TransactionMetadata
    w = oracle.TxWitness.generate(4, 3, seed=77)
    meta = TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS])
    lde = oracle.lde_columns(oracle.interpolate_columns(oracle.tx_build_trace(w)), 3)
    nodes = oracle.merkle_build(oracle.hash_rows(lde, 3))
    b = Backend()
    b.upload_witness(meta)
    proof = b.prove(ProofOptions(*SHARD_OPTS))
    b.close()
    return meta, lde, nodes, proof


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_window_rows_at_steered_positions(shard_reference, world):
    import torch
    from certificate_stark_amd.backend import Backend, to_numpy_u64
    from certificate_stark_amd.prover import ProofOptions
    meta, lde, nodes, single = shard_reference
    nk, n = 8 // world, lde.shape[2]
    N, nq, log_nk = 8 * n, SHARD_OPTS[0], (8 // world).bit_length() - 1
    rng = np.random.default_rng(world)
    row, i = int(rng.integers(0, n)), int(rng.integers(1, N // 2 - 1))
    steered = [0, N - 1] + [8 * int(rng.integers(0, n)) + k for k in range(8)]       # both ends, one position in every coset
    steered += [8 * row + nk - 1, 8 * row + nk]           # neighbouring leaves of two ranks (nk = 1: they are siblings)
    steered += [2 * i, 2 * i + 1, 2 * i]                  # a sibling pair and a duplicate
    steered += [int(v) for v in rng.integers(0, N, size=nq - len(steered))]
    assert len(steered) == nq
    options = ProofOptions(*SHARD_OPTS)
    ranks = [Backend() for _ in range(world)]
    try:
        for b in ranks:
            b.upload_witness(meta)
        leaves = torch.cat([b.shard_commit(options, r * nk, nk) for r, b in enumerate(ranks)])
        combined = torch.cat([b.shard_evaluate(leaves) for b in ranks])
        positions = ranks[0].shard_compose(combined)
        pos_t = torch.from_numpy(np.array(steered, np.uint32).view(np.int32)).to(ranks[0].device)
        for r, b in enumerate(ranks):
            got = to_numpy_u64(b.shard_open_rows(pos_t))
            assert got.shape == (nq, 94 + 4 * log_nk)
            want = np.zeros_like(got)                      # foreign cosets: zeros (the owners' rows are summed in)
            for q, p in enumerate(steered):
                sib = K.window_siblings(nodes, p, r * nk, nk)
                if sib is not None:
                    want[q, :94] = lde[p % 8, :, p // 8]
                    want[q, 94:] = sib
            assert (got == want).all(), (r, np.argwhere(got != want)[:8])
        # the proof's own positions after the steered ones: the same bytes as the single-GPU proof
        rows = sum(b.shard_open_rows(positions) for b in ranks)
        assert ranks[0].shard_finish(rows) == single
    finally:
        for b in ranks:
            b.close()
        torch.cuda.empty_cache()
