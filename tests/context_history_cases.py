"""The catalogue of the context-history tests (test_context_history_cpu.py, test_gpu_context_history.py): every kind of call a
cstark_ctx serves, each with an expectation that comes from the CPU side alone (oracle.*, oracle/prover.py, oracle/verifier.py,
ledger_model.LedgerModel and the helpers of multiproof_cases.py, sig_cases.py, validate_cases.py), the table STATE that classifies
every data member of struct cstark_ctx (csrc/ctx.h), and the schedules -- pure functions of their seeds -- in which the GPU tests drive
one long-lived context through these calls.  Not a conftest; no GPU is needed to import it or to compute an expectation.

An operation is self-contained: it brings its own inputs.  A witness is uploaded only when the context does not already hold it
(Env.resident), as the product's own _ResidentWitness does: a proof of a witness that an earlier call left resident is then a proof
from device memory that every call in between had a chance to disturb."""
import functools
import hashlib
import os
import random
import re
import struct

import numpy as np

import ledger_cases as LC
import ledger_model as LM
import multiproof_cases as MC
import sig_cases as SC
import validate_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = LM.P

Q28 = (28, 8, 0, 0, 0, 4, 256)          # base field, device channel
Q42 = (42, 8, 0, 0, 0, 4, 256)          # the reference's example options
TX_OPTION_SETS = {
    "q28": Q28, "q96": (96, 8, 0, 0, 0, 4, 256), "cubic42": (42, 8, 0, 0, 2, 4, 256), "quad": (42, 8, 0, 0, 1, 4, 256),
    "sha3": (42, 8, 0, 1, 0, 4, 256), "b16": (28, 16, 0, 0, 0, 4, 256), "f8r128": (28, 8, 0, 0, 0, 8, 128),
    "grind8": (28, 8, 8, 0, 0, 4, 256),       # below the device search's threshold: the host searches
    "grind15": (20, 8, 15, 0, 0, 4, 256),     # the device search (tests/test_gpu_prove.py)
}
TX_SHAPES = [(1, 3), (2, 3), (2, 7), (2, 15), (4, 7)]
AIR_WIDTH_CE = {0: (94, 8), 1: (65, 4), 2: (56, 8), 3: (2, 2), 4: (14, 4)}   # oracle/prover.py: the jobs' width and ce


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle import oracle as O
    O.build()
    return O


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


class Env:
    """One context under test: the Backend and what this catalogue knows to be resident in it."""

    def __init__(self, backend):
        self.backend = backend
        self.resident = None

    def hold(self, key, upload):
        """the witness `key` is resident after this call: uploaded now unless an earlier operation left exactly it there"""
        if self.resident != key:
            self.resident = None
            upload()
            self.resident = key


class Op:
    def __init__(self, name, family, touches, run, expect, refused=False, proof=None):
        self.name, self.family, self.touches, self._run, self._expect, self.refused, self.proof = name, family, frozenset(touches), run, expect, refused, proof

    def run(self, env):
        return normalise(self._run(env))

    @property
    def expectation(self):
        if not hasattr(self, "_memo"):
            self._memo = normalise(self._expect())
        return self._memo

    def __repr__(self):
        return self.name


def normalise(r):
    """bytes stay bytes; anything else becomes a tuple of numpy arrays"""
    if isinstance(r, (bytes, bytearray)):
        return bytes(r)
    if not isinstance(r, (tuple, list)):
        r = (r,)
    out = []
    for a in r:
        if isinstance(a, (bytes, bytearray)):
            a = np.frombuffer(bytes(a), np.uint8)
        elif hasattr(a, "detach"):
            a = a.detach().cpu().contiguous().numpy()
            if a.dtype == np.int64:
                a = a.view(np.uint64)
        out.append(np.asarray(a))
    return tuple(out)


def first_difference(op, got, want):
    """None when equal, else a sentence that says where the two answers part"""
    if isinstance(want, bytes):
        if got == want:
            return None
        if not isinstance(got, bytes):
            return "the answer is no byte string"
        at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        where = "first differing byte %d of %d (got %d bytes)" % (at, len(want), len(got))
        if op.proof is not None and len(got) == len(want):
            from tools.make_proof_digest import section_digests
            nq, width, ce = op.proof
            try:
                a, b = section_digests(got, nq, width, ce), section_digests(want, nq, width, ce)
                where += "; sections that differ: %s" % [k for k in b if a[k] != b[k]]
            except Exception as e:                      # a proof too broken to be cut into sections
                where += "; no section digest (%s)" % e
        return where
    if not isinstance(got, tuple) or len(got) != len(want):
        return "%d parts instead of %d" % (len(got) if isinstance(got, tuple) else -1, len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape:
            return "part %d has shape %s instead of %s" % (k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(np.atleast_1d(g != w))
            return "part %d differs at %d of %d places, first at index %s" % (k, len(bad), w.size, tuple(int(v) for v in bad[0]))
    return None


OPS = []
BY_NAME = {}


def add(name, family, touches, run, expect, refused=False, proof=None):
    assert name not in BY_NAME
    op = Op(name, family, touches, run, expect, refused, proof)
    OPS.append(op)
    BY_NAME[name] = op
    return op


def _dev(b, a):
    """a device copy of a shared (read-only) host array"""
    return b.from_numpy_u64(np.array(a, np.uint64))


def options(opts):
    from certificate_stark_amd.prover import ProofOptions
    return ProofOptions(*opts)


# ---- transforms ---------------------------------------------------------------------------------------------------------------------------
WIDTH = 3
NTT = {"plans", "cosets", "ws", "ws_bytes"}
STEP = NTT | {"steps"}


@functools.lru_cache(maxsize=None)
def offset(kind):
    O = oracle()
    if kind == "default":
        return None
    if kind == "one":
        return int(O.to_mont([1])[0])
    return int(O.fp_pow(np.array([O.generator()], np.uint64), 8)[0])      # g^8


@functools.lru_cache(maxsize=None)
def columns(log_n, block=0, split=0):
    """[WIDTH][2^log_n] elements; block: constant over blocks of that many rows (split: two values per block)"""
    rng = np.random.default_rng(9000 + 97 * log_n + block + split)
    n = 1 << log_n
    if not block:
        return _frozen(rng.integers(0, P, size=(WIDTH, n), dtype=np.uint64))[0]
    u = rng.integers(0, P, size=(WIDTH, n // block), dtype=np.uint64)
    v = rng.integers(0, P, size=(WIDTH, n // block), dtype=np.uint64) if split else u
    first = np.arange(n) % block < (split or block)
    return _frozen(np.ascontiguousarray(np.where(first[None, :], np.repeat(u, block, axis=1), np.repeat(v, block, axis=1))))[0]


def _transform_expect(log_n, log_b, off, block=0, split=0):
    O = oracle()
    co = O.interpolate_columns(columns(log_n, block, split).copy())
    return co, O.lde_columns(co, log_b, offset=offset(off))


def _lde_run(log_n, log_b, off):
    def run(env):
        b = env.backend
        co = b.interpolate_columns(_dev(b, columns(log_n)))
        return co, b.lde_columns(co, log_b, offset=offset(off))
    return run


def _step_run(block, split):
    def run(env):
        b = env.backend
        ev = _dev(b, columns(16, block, split))
        return b.step2_columns(ev, block, split, 3) if split else b.step_columns(ev, block, 3)
    return run


for _log_n in (6, 10, 14, 16):
    add("lde_n%d" % _log_n, "transform", NTT, _lde_run(_log_n, 3, "default"), functools.partial(_transform_expect, _log_n, 3, "default"))
for _log_b in (1, 2, 4):
    add("lde_n10_b%d" % (1 << _log_b), "transform", NTT, _lde_run(10, _log_b, "default"), functools.partial(_transform_expect, 10, _log_b, "default"))
for _off in ("one", "g8"):
    add("lde_n10_off_%s" % _off, "transform", NTT, _lde_run(10, 3, _off), functools.partial(_transform_expect, 10, 3, _off))
for _block in (1024, 512):
    add("step_n16_blk%d" % _block, "transform", STEP, _step_run(_block, 0), functools.partial(_transform_expect, 16, 3, "default", _block, 0))
for _split in (127, 255):
    add("step2_n16_s%d" % _split, "transform", STEP, _step_run(1024, _split), functools.partial(_transform_expect, 16, 3, "default", 1024, _split))


# ---- commitments --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def commit_table():
    return _frozen(np.random.default_rng(77).integers(0, P, size=(2, 9, 128), dtype=np.uint64))[0]


def _commit_run(hash_fn):
    def run(env):
        import torch
        b = env.backend
        leaves = b.hash_rows_fn(hash_fn, _dev(b, commit_table()), 1)
        nodes = torch.zeros((512, 32), dtype=torch.uint8, device=b.device)
        nodes[256:] = leaves
        return b.merkle_build_fn(hash_fn, nodes)[1:]
    return run


def _commit_expect(hash_fn):
    O = oracle()
    return O.merkle_build(O.hash_rows(commit_table(), 1, hash_fn=hash_fn), hash_fn=hash_fn)[1:]


for _h, _nm in ((0, "blake3"), (1, "sha3")):
    add("commit_%s" % _nm, "commit", set(), _commit_run(_h), functools.partial(_commit_expect, _h))


# ---- TransactionAir proofs ----------------------------------------------------------------------------------------------------------------
TX_STATE = NTT | STEP | {"wit_buf", "wit_bytes", "wit", "periodic", "coef_buf", "coef_stage", "coef_ev", "gfold_j", "desc_buf", "desc_bytes", "arena",
                         "side", "side2", "ev_fork", "ev_join", "ev_join2", "ev_mid"}
HOST_CHANNEL = {"deep_buf", "deep_stage", "deep_words", "deep_ev"}      # base field with the Sha3 coin or a proof of work: prove.hip, cstark_deep_composition


@functools.lru_cache(maxsize=None)
def tx_witness(n_tx, depth):
    """(1, 3): the witness of test_gpu_split_merge.py's proof comparison"""
    w = oracle().TxWitness.generate(n_tx, depth, seed=505 if (n_tx, depth) == (1, 3) else 700 + 16 * n_tx + depth)
    _frozen(*[getattr(w, f) for f in w.FIELDS])
    return w


@functools.lru_cache(maxsize=None)
def cpu_tx_proof(n_tx, depth, opts):
    from oracle import prover as OP
    return OP.prove(tx_witness(n_tx, depth), opts)


def hold_tx(env, n_tx, depth):
    env.hold(("tx", n_tx, depth), lambda: env.backend.upload_witness(tx_witness(n_tx, depth)))


def _tx_run(n_tx, depth, opts):
    def run(env):
        hold_tx(env, n_tx, depth)
        return env.backend.prove(options(opts))
    return run


def tx_name(n_tx, depth, key="q28"):
    return "tx_%d_d%d" % (n_tx, depth) + ("" if key == "q28" else "_" + key)


def _host_channel(opts):
    return opts[4] == 0 and (opts[3] == 1 or opts[2] > 0)


for _n, _d in TX_SHAPES:
    _o = Q42 if (_n, _d) == (1, 3) else Q28
    add(tx_name(_n, _d), "tx_prove", TX_STATE, _tx_run(_n, _d, _o), functools.partial(cpu_tx_proof, _n, _d, _o), proof=(_o[0], 94, 8))
for _key, _o in TX_OPTION_SETS.items():
    if _key != "q28":
        add(tx_name(2, 3, _key), "tx_prove", TX_STATE | (HOST_CHANNEL if _host_channel(_o) else set()), _tx_run(2, 3, _o),
            functools.partial(cpu_tx_proof, 2, 3, _o), proof=(_o[0], 94, 8))


def _shard_run(n_tx, depth):
    """One proof sharded by LDE coset over two ranks, as tests/test_gpu_sharding.py runs it on one GPU: the context under test is rank 0
    (cosets 0..3; it composes and finishes), a short-lived second context is rank 1, and the buffers the ranks would exchange are moved
    here.  Rank 0's share of the degree-split evaluation extends register 37 into shard_bit37, 8 n words."""
    def run(env):
        import torch
        from certificate_stark_amd.backend import Backend
        hold_tx(env, n_tx, depth)
        ranks, opt = [env.backend, Backend()], options(Q28)
        try:
            ranks[1].upload_witness(tx_witness(n_tx, depth))
            leaves = torch.cat([b.shard_commit(opt, 4 * r, 4) for r, b in enumerate(ranks)])
            combined = torch.cat([b.shard_evaluate(leaves) for b in ranks])
            positions = ranks[0].shard_compose(combined)
            rows = sum(b.shard_open_rows(positions) for b in ranks)
            proof = ranks[0].shard_finish(rows)
        except Exception:
            ranks[1].ctx = None   # abandoned, not destroyed: after an error nothing more is asked of the GPU
            raise
        ranks[1].close()
        return proof
    return run


for _n, _d in ((2, 3), (4, 7)):      # the bytes of tx_2_d3 / tx_4_d7: a sharded proof is the single-GPU proof
    add("shard_%d_d%d" % (_n, _d), "tx_prove", TX_STATE | HOST_CHANNEL | {"shard_bit37", "shard_bit37_words"}, _shard_run(_n, _d),
        functools.partial(cpu_tx_proof, _n, _d, Q28), proof=(28, 94, 8))


# ---- sub-AIR proofs -----------------------------------------------------------------------------------------------------------------------
AIR_STATE = NTT | {"small_periodic", "assert_inv", "air_static", "air_coef_buf", "air_coef_stage", "air_coef_words", "air_coef_ev", "desc_buf",
                   "desc_bytes", "arena"}
SCHNORR_STATE = AIR_STATE | {"wit_buf", "wit_bytes", "wit", "tail_buf", "tail_bytes", "schnorr_rx", "schnorr_av_stage", "schnorr_pub", "schnorr_s",
                             "schnorr_seed", "schnorr_seed_key", "side", "side2", "ev_fork", "ev_join", "ev_join2", "ev_mid"}
RANGE_WORDS = {6: np.array([0x0123456789ABCDEF], np.uint64),      # n / 64 words of an (n - 1)-bit value
               10: (np.arange(1, 17, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.array([0] * 15 + [1], np.uint64)}
RANGE_BATCH = {3: 3, 40: 40}
RESCUE_SEED = tuple(range(42, 49))
SCHNORR_ALT = (42, 8, 0, 0, 2, 4, 256)      # the same statement under a second option set: another channel seed


@functools.lru_cache(maxsize=None)
def cpu_air_proof(kind, *args):
    from oracle import prover as OP
    O = oracle()
    if kind == "merkle":
        return OP.prove_air(O.AIR_MERKLE, tx_witness(2, args[0]), Q28)
    if kind == "range_bits":
        return OP.prove_air(O.AIR_RANGE, RANGE_WORDS[args[0]], args[1], log_n=args[0])
    if kind == "range_number":
        return OP.prove_air(O.AIR_RANGE, int(args[0]), Q28)
    if kind == "rescue":
        return OP.prove_air(O.AIR_RESCUE_CHAIN, (O.to_mont(np.array(RESCUE_SEED, np.uint64)), args[0]), args[1] if len(args) > 1 else Q28)
    if kind == "schnorr":
        return OP.prove_air(O.AIR_SCHNORR, schnorr_witness(args[0], args[1]), args[2])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def schnorr_witness(n_sig, seed):
    w = oracle().SchnorrWitness.generate(n_sig, seed)
    _frozen(w.messages, w.sig_rx, w.sig_s)
    return w


def hold_schnorr(env, n_sig, seed):
    w = schnorr_witness(n_sig, seed)
    env.hold(("schnorr", n_sig, seed), lambda: env.backend.upload_schnorr_witness(w.messages, w.sig_rx, w.sig_s))


@functools.lru_cache(maxsize=None)
def range_numbers(count):
    O = oracle()
    values = [0, 1, 2**63 - 1] + [int(v) >> 1 for v in np.random.default_rng(count).integers(0, 2**63, size=count, dtype=np.uint64)]
    return _frozen(O.to_mont(np.array(values[:count], np.uint64)))[0]


def _merkle_run(depth):
    def run(env):
        hold_tx(env, 2, depth)
        return env.backend.air_prove(env.backend.AIR_MERKLE, options(Q28))
    return run


def _schnorr_run(n_sig, seed, opts):
    def run(env):
        hold_schnorr(env, n_sig, seed)
        return env.backend.air_prove(env.backend.AIR_SCHNORR, options(opts))
    return run


def _sub(name, touches, run, expect, air, nq=28):
    add(name, "sub_air", touches, run, expect, proof=(nq,) + AIR_WIDTH_CE[air])


for _d in (3, 15):       # the same (air, n_items, log_n, log_b), another Merkle depth
    _sub("merkle_d%d" % _d, AIR_STATE | {"wit_buf", "wit_bytes", "wit"}, _merkle_run(_d), functools.partial(cpu_air_proof, "merkle", _d), 1)
for _ln in (6, 10):
    _sub("range_bits_%d" % _ln, AIR_STATE, (lambda ln: lambda env: env.backend.range_prove_bits(options(Q28), RANGE_WORDS[ln], ln))(_ln),
         functools.partial(cpu_air_proof, "range_bits", _ln, Q28), 3)
_sub("range_bits_6_sha3", AIR_STATE | HOST_CHANNEL, lambda env: env.backend.range_prove_bits(options(TX_OPTION_SETS["sha3"]), RANGE_WORDS[6], 6),
     functools.partial(cpu_air_proof, "range_bits", 6, TX_OPTION_SETS["sha3"]), 3, nq=42)
for _c in RANGE_BATCH:
    add("range_batch_%d" % _c, "sub_air", AIR_STATE | {"rb_dev", "rb_host", "rb_dev_bytes", "rb_host_bytes"},
        (lambda c: lambda env: list(env.backend.range_prove_batch(options(Q28), range_numbers(c))))(_c),
        (lambda c: lambda: [cpu_air_proof("range_number", int(v)) for v in range_numbers(c)])(_c))
for _len in (16, 128):
    _sub("rescue_%d" % _len, AIR_STATE,
         (lambda L: lambda env: env.backend.rescue_prove(options(Q28), oracle().to_mont(np.array(RESCUE_SEED, np.uint64)), L))(_len),
         functools.partial(cpu_air_proof, "rescue", _len), 4)
_sub("rescue_16_b16", AIR_STATE, lambda env: env.backend.rescue_prove(options(TX_OPTION_SETS["b16"]), oracle().to_mont(np.array(RESCUE_SEED, np.uint64)), 16),
     functools.partial(cpu_air_proof, "rescue", 16, TX_OPTION_SETS["b16"]), 4)      # the same (air, items, log_n), another blowup
_sub("schnorr_2", SCHNORR_STATE, _schnorr_run(2, 9, Q28), functools.partial(cpu_air_proof, "schnorr", 2, 9, Q28), 2)
_sub("schnorr_2_alt", SCHNORR_STATE, _schnorr_run(2, 9, SCHNORR_ALT), functools.partial(cpu_air_proof, "schnorr", 2, 9, SCHNORR_ALT), 2, nq=42)
_sub("schnorr_2_other", SCHNORR_STATE, _schnorr_run(2, 10, Q28), functools.partial(cpu_air_proof, "schnorr", 2, 10, Q28), 2)
_sub("schnorr_4", SCHNORR_STATE, _schnorr_run(4, 9, Q28), functools.partial(cpu_air_proof, "schnorr", 4, 9, Q28), 2)
@functools.lru_cache(maxsize=None)
def merkle_combine_case(log_b):
    """MerkleAir's constraint stage alone over 2^log_b cosets: inside a proof the stage always runs at the AIR's own constraint-evaluation
    blowup, so only the public entry point reaches one (air, items, log_n) under two values of log_b"""
    O = oracle()
    trace = O.merkle_build_trace(tx_witness(2, 3))
    desc = O.merkle_desc(trace)
    lde = O.lde_columns(O.interpolate_columns(trace.copy()), log_b)
    coefs = tuple(np.asarray(O.random_elements(k, 40 + i), np.uint64) for i, k in enumerate((106, 106, 14, 14)))
    return _frozen(lde)[0], coefs, np.asarray(desc.a_value, np.uint64), desc


def _merkle_combine_run(log_b):
    def run(env):
        b = env.backend
        lde, coefs, a_value, _ = merkle_combine_case(log_b)
        return b.merkle_evaluate_constraints(_dev(b, lde), 3, *coefs, a_value, log_b)
    return run


def _merkle_combine_expect(log_b):
    O = oracle()
    lde, coefs, _, desc = merkle_combine_case(log_b)
    ev = O.air_evaluate_transitions(O.AIR_MERKLE, lde, O.periodic_table(O.merkle_periodic_columns(3), 10, log_b), 106)
    return O.air_combine(desc, lde, ev, *coefs, log_b)


for _lb in (2, 3):
    add("merkle_combine_b%d" % (1 << _lb), "sub_air", AIR_STATE, _merkle_combine_run(_lb), functools.partial(_merkle_combine_expect, _lb))
LOG_N_10 = ["tx_1_d3", "merkle_d3", "schnorr_2", "range_bits_10"]     # four AIRs, four arenas, one plan (rescue_128 is a fifth)


# ---- verification: verdicts as accepted / rejected, against oracle/verifier.py ----------------------------------------------------------------
VERIFY_STATE = {"verify"}


def flipped(proof, at=None):
    bad = bytearray(proof)
    bad[len(bad) // 2 if at is None else at] ^= 0x04
    return bytes(bad)


def _accepts(check, *args, **kw):
    from oracle import verifier as V
    try:
        return bool(check(*args, **kw))
    except V.VerifierError:
        return False


@functools.lru_cache(maxsize=None)
def tx_verify_case():
    """[(proof, initial root, final root)]: two sizes, one of them again with a flipped byte"""
    w1, w2 = tx_witness(1, 3), tx_witness(2, 3)
    p1, p2 = cpu_tx_proof(1, 3, Q42), cpu_tx_proof(2, 3, Q28)
    return [(p2, w2.initial_roots[0], w2.final_root), (flipped(p2), w2.initial_roots[0], w2.final_root), (p1, w1.initial_roots[0], w1.final_root)]


def _tx_verify_run(env):
    case = tx_verify_case()
    return env.backend.tx_verify([c[0] for c in case], np.array([c[1] for c in case]), np.array([c[2] for c in case])) == 0


def _tx_verify_expect():
    from oracle import verifier as V
    return np.array([_accepts(V.verify, *c) for c in tx_verify_case()])


@functools.lru_cache(maxsize=None)
def air_verify_case(small):
    """[(proof, air, 14 public words)]"""
    O = oracle()
    number = np.zeros(14, np.uint64)
    number[0] = O.range_build_trace_bits(RANGE_WORDS[6], 6)[1]
    rng = (cpu_air_proof("range_bits", 6, Q28), 3, number)
    if small:
        return [rng]
    w = tx_witness(2, 3)
    roots = np.concatenate([w.initial_roots[0], w.final_root])
    seed = O.to_mont(np.array(RESCUE_SEED, np.uint64))
    chain = np.concatenate([seed, O.rescue_chain_build_trace(seed, 16)[:7, -1]])
    mk = cpu_air_proof("merkle", 3)
    return [(mk, 1, roots), rng, (flipped(mk), 1, roots), (cpu_air_proof("rescue", 16), 4, chain)]


def _air_verify_run(small):
    def run(env):
        case = air_verify_case(small)
        return env.backend.air_verify([c[0] for c in case], [c[1] for c in case], np.array([c[2] for c in case])) == 0
    return run


def _air_verify_expect(small):
    from oracle import verifier as V
    out = []
    for proof, air, pub in air_verify_case(small):
        if air == 1:
            out.append(_accepts(V.verify_merkle, proof, pub[:7], pub[7:]))
        elif air == 3:
            out.append(_accepts(V.verify_range, proof, int(pub[0])))
        else:
            out.append(_accepts(V.verify_rescue, proof, pub[:7], pub[7:]))
    return np.array(out)


def _schnorr_verify_run(env):
    w = schnorr_witness(2, 9)
    p = cpu_air_proof("schnorr", 2, 9, Q28)
    return env.backend.schnorr_verify([p, flipped(p)], [w, w]) == 0


def _schnorr_verify_expect():
    from oracle import verifier as V
    w = schnorr_witness(2, 9)
    p = cpu_air_proof("schnorr", 2, 9, Q28)
    return np.array([_accepts(V.verify_schnorr, p, w), _accepts(V.verify_schnorr, flipped(p), w)])


add("tx_verify", "verify", VERIFY_STATE, _tx_verify_run, _tx_verify_expect)
add("air_verify", "verify", VERIFY_STATE, _air_verify_run(False), functools.partial(_air_verify_expect, False))
add("air_verify_range", "verify", VERIFY_STATE, _air_verify_run(True), functools.partial(_air_verify_expect, True))
add("schnorr_verify", "verify", VERIFY_STATE, _schnorr_verify_run, _schnorr_verify_expect)


# ---- trace validation: the report against validate_cases.py ----------------------------------------------------------------------------------
VALIDATE_STATE = {"raw_periodic", "val_buf", "val_bytes"}
VALIDATE_CELLS = {VC.TX: (60, 1023), VC.MERKLE: (60, 512), VC.SCHNORR: (3, 700), VC.RANGE: (1, 30), VC.RESCUE: (3, 8)}
VALIDATE_NAMES = {VC.TX: "tx", VC.MERKLE: "merkle", VC.SCHNORR: "schnorr", VC.RANGE: "range", VC.RESCUE: "rescue"}


@functools.lru_cache(maxsize=None)
def validate_case(air, bad):
    """(trace, depth, public words or None, SchnorrAir's statement or None)"""
    O = oracle()
    depth, public, statement = 0, None, None
    if air in (VC.TX, VC.MERKLE):
        w = tx_witness(2, 3)
        trace, depth, public = (O.tx_build_trace(w) if air == VC.TX else O.merkle_build_trace(w)), 3, np.concatenate([w.initial_roots[0], w.final_root])
    elif air == VC.SCHNORR:
        statement = schnorr_witness(2, 9)
        trace = O.schnorr_build_trace(statement)
    elif air == VC.RANGE:
        trace, public = O.range_build_trace(0x123456789ABCDEF), O.to_mont([0x123456789ABCDEF])
    else:
        seed = O.to_mont(np.array(RESCUE_SEED, np.uint64))
        trace = O.rescue_chain_build_trace(seed, 16)
        public = np.concatenate([seed, trace[:7, -1]])
    if bad:
        trace = VC.bump(trace, [VALIDATE_CELLS[air]])
    return _frozen(np.ascontiguousarray(trace))[0], depth, public, statement


def _report(step, constraint, bad_cycles, boundary, codes, frame):
    none = lambda v: -1 if v is None else int(v)
    head = np.array([none(step), none(constraint), bad_cycles] + [none(v) for v in (boundary or (None, None, None))], np.int64)
    return head, np.asarray(codes, np.uint32), np.zeros(0, np.uint64) if frame is None else np.asarray(frame, np.uint64)


def _validate_run(air, bad):
    def run(env):
        trace, depth, public, statement = validate_case(air, bad)
        if statement is not None:
            hold_schnorr(env, 2, 9)
            public = True
        b = env.backend
        r = b.air_validate_trace(air, _dev(b, trace), depth, public, want_cycles=True, want_frame=True)
        return _report(r.step, r.constraint, r.bad_cycles, (r.boundary, r.boundary_register, r.boundary_step), r.cycle_codes, r.frame_values)
    return run


def _validate_expect(air, bad):
    O = oracle()
    trace, depth, public, statement = validate_case(air, bad)
    clean = validate_case(air, False)[0]
    if air == VC.TX and bad:
        assert O.tx_check_trace(clean, 2, 3) == -1
    ref = VC.reference(O, air, trace, depth, statement, clean_trace=clean if (air == VC.TX and bad) else None)
    return _report(ref.step, ref.constraint, ref.bad_cycles, VC.boundary_reference(O, air, trace, public, statement), ref.codes, ref.frame_values)


for _air in (VC.TX, VC.MERKLE, VC.SCHNORR, VC.RANGE, VC.RESCUE):
    for _bad in (False, True):
        add("validate_%s_%s" % (VALIDATE_NAMES[_air], "cell" if _bad else "clean"), "validate",
            VALIDATE_STATE | (SCHNORR_STATE - AIR_STATE if _air == VC.SCHNORR else set()), _validate_run(_air, _bad), functools.partial(_validate_expect, _air, _bad))


# ---- signature checks -------------------------------------------------------------------------------------------------------------------
def sig_case(name):
    if name == "forged":
        return SC.perturbed(SC.generated(2), 1, "s_bit0")
    return SC.generated(int(name))


for _nm in ("1", "9", "forged"):
    add("sig_check_%s" % _nm, "sig", {"sig_buf", "sig_bytes"},
        (lambda nm: lambda env: env.backend.schnorr_check(*sig_case(nm), want_rx=True))(_nm), (lambda nm: lambda: SC.reference(*sig_case(nm)))(_nm))


# ---- the account ledger against LedgerModel ------------------------------------------------------------------------------------------------
LEDGER_STATE = {"wit_buf", "wit_bytes", "wit"}
LEDGER_CASES = {3: (2, 3, 2), 15: (2, 15, 12)}      # ledger_cases: (n_tx, depth, seed)


def _ledger_inputs(depth):
    w = LC.generated(LEDGER_CASES[depth])
    return (w,) + LC.initial_accounts(w)


def _asked(depth, indices):
    """what the openings ask for: every account, an absent leaf, both ends of the tree; ascending and distinct"""
    have = set(int(i) for i in indices)
    absent = next(i for i in range(1 << depth) if i not in have)
    return np.array(sorted(have | {absent, 0, (1 << depth) - 1}), np.uint64)


def _ledger_apply_run(depth, checked):
    def run(env):
        from certificate_stark_amd.backend import to_numpy_u64
        b = env.backend
        w, indices, values = _ledger_inputs(depth)
        led = b.ledger_create(depth)
        try:
            b.ledger_set_accounts(led, indices, values)
            env.resident = None
            at, reason, arrays = b.ledger_apply(led, depth, *SC.transfers(w), check_signatures=checked)
            assert at == -1, "the batch was refused at %d for reason %d" % (at, reason)
            env.resident = ("ledger", depth)
            fields = [arrays[f] for f in w.FIELDS]
            root = b.ledger_root(led)
            trace_roots = to_numpy_u64(b.build_trace()[58:65, ::1023])
            return fields + [root, trace_roots, b.prove(options(Q28))]
        finally:
            b.ledger_destroy(led)
    return run


@functools.lru_cache(maxsize=None)
def _ledger_model_applied(depth):
    w, indices, values = _ledger_inputs(depth)
    m = LM.LedgerModel(depth)
    m.set_accounts(indices, values)
    before = m.copy()
    got = m.apply(*SC.transfers(w))
    assert not isinstance(got, tuple), "the model refuses the batch"
    return before, m, got


def _ledger_apply_expect(depth):
    from oracle import prover as OP
    O = oracle()
    _, m, wm = _ledger_model_applied(depth)
    trace_roots = O.tx_build_trace(wm)[58:65, ::1023]
    return [getattr(wm, f) for f in wm.FIELDS] + [m.root(), trace_roots, OP.prove(wm, Q28)]


def _ledger_open_run(depth):
    def run(env):
        b = env.backend
        w, indices, values = _ledger_inputs(depth)
        ask = _asked(depth, indices)
        led = b.ledger_create(depth)
        try:
            b.ledger_set_accounts(led, indices, values)
            cp = b.ledger_checkpoint(led)
            at, reason, _ = b.ledger_apply(led, depth, *SC.transfers(w), want_witness=False)
            assert at == -1
            env.resident = ("ledger", depth)
            out = []
            for when in (None, cp):       # the current state, then the state under the checkpoint's root
                val, present, paths, root = b.ledger_open_accounts(led, depth, ask, at=when)
                verdicts, folded = b.account_check_paths(ask, paths, root, val, present, want_roots=True)
                mval, mpresent, nodes, mroot = b.ledger_open_multi(led, depth, ask, at=when)
                verdict, bad_at, mfolded, merges = b.account_check_multiproof(depth, ask, nodes, mroot, mval, mpresent)
                out += [val, present, paths, root, verdicts, folded, mval, mpresent, nodes, mroot, np.array([verdict, bad_at, merges]), mfolded]
            out.append(b.ledger_root_at(led, cp))
            r = b.ledger_audit(led)
            out.append(np.array([r.consistent, r.n_bad, r.n_nodes]))
            r = b.ledger_audit(led, cp)
            out.append(np.array([r.consistent, r.n_bad, r.n_nodes]))
            b.ledger_revert(led, cp)
            out += [b.ledger_root(led), b.ledger_get_accounts(led, ask)[0]]
            return out
        finally:
            b.ledger_destroy(led)
    return run


def _ledger_open_expect(depth):
    w, indices, values = _ledger_inputs(depth)
    ask = _asked(depth, indices)
    before, after, _ = _ledger_model_applied(depth)
    out = []
    for m in (after, before):
        val, present = MC.accounts_from_model(m, ask)
        paths = np.array([m._path(int(i)) for i in ask], np.uint64)
        nodes = MC.nodes_from_model(m, ask)
        folded = np.array([m.root()] * len(ask), np.uint64)
        for i, path in zip(ask, paths):        # an honest path folds to the root: said by the plain fold, not assumed
            import ledger_paths_cases as LP
            assert np.array_equal(LP.fold(int(i), path, depth), m.root())
        verdict, bad_at, mfolded, merges = MC.expected_verdict(depth, ask, nodes, m.root(), val, present)
        out += [val, present.astype(bool), paths, m.root(), np.zeros(len(ask), np.uint8), folded, val, present.astype(bool), nodes, m.root(),
                np.array([verdict, bad_at, merges]), mfolded]
    out.append(before.root())
    out.append(np.array([1, 0, after.n_nodes()]))
    out.append(np.array([1, 0, before.n_nodes()]))
    out += [before.root(), MC.accounts_from_model(before, ask)[0]]
    return out


for _d in (3, 15):
    add("ledger_d%d_apply" % _d, "ledger", LEDGER_STATE | TX_STATE, _ledger_apply_run(_d, False), functools.partial(_ledger_apply_expect, _d))
    add("ledger_d%d_checked" % _d, "ledger", LEDGER_STATE | TX_STATE | {"sig_buf", "sig_bytes"}, _ledger_apply_run(_d, True),
        functools.partial(_ledger_apply_expect, _d))
    add("ledger_d%d_open" % _d, "ledger", LEDGER_STATE | {"path_buf", "path_bytes", "multi_buf", "multi_bytes"}, _ledger_open_run(_d),
        functools.partial(_ledger_open_expect, _d))


def _node_count_case():
    _, indices, _ = _ledger_inputs(3)
    ask = _asked(3, indices)
    _, after, _ = _ledger_model_applied(3)
    val, present = MC.accounts_from_model(after, ask)
    nodes = MC.nodes_from_model(after, ask)
    assert len(nodes) > 1
    return ask, val, present, after.root(), [nodes[:-1], np.concatenate([nodes, nodes[:1]]), nodes]


def _node_count_run(env):
    """the checker's side of a wrong node count: one node too few and one too many are verdicts (nothing is launched), between them and
    the honest proof the block of cstark_account_check_multiproof is reused"""
    ask, val, present, root, proofs = _node_count_case()
    out = []
    for nodes in proofs:
        verdict, at, folded, merges = env.backend.account_check_multiproof(3, ask, nodes, root, val, present)
        out += [np.array([verdict, at, merges]), np.zeros(0, np.uint64) if folded is None else folded]
    return out


def _node_count_expect():
    ask, val, present, root, proofs = _node_count_case()
    out = []
    for nodes in proofs:
        verdict, at, folded, merges = MC.expected_verdict(3, ask, nodes, root, val, present)
        out += [np.array([verdict, at, merges]), np.zeros(0, np.uint64) if folded is None else folded]
    assert [int(o[0]) for o in out[::2]] == [MC.NODE_COUNT, MC.NODE_COUNT, MC.VALID]
    return out


add("multiproof_node_count", "ledger", {"multi_buf", "multi_bytes"}, _node_count_run, _node_count_expect)


# ---- refused calls: each raises CstarkError ---------------------------------------------------------------------------------------------------
def _refuse_count(env):
    w = oracle().TxWitness.generate(3, 3, seed=3)
    env.resident = None
    env.backend.upload_witness(w)
    env.resident = ("tx-odd", 3, 3)
    env.backend.prove(options(Q28))


def _refuse_modulus(env):
    env.backend.range_prove_batch(options(Q28), np.array([1, P], np.uint64))


def _refuse_block(env):
    b = env.backend
    b.step_columns(_dev(b, columns(16, 1024)), 1000, 3)


def _refuse_window(env):
    hold_tx(env, 2, 3)
    env.backend.shard_commit(options(Q42), 2, 4)


def _refuse_options(env):
    hold_tx(env, 2, 3)
    env.backend.air_prove(env.backend.AIR_MERKLE, options((42, 2, 0, 0, 0, 4, 256)))       # MerkleAir needs blowup 4


def _refuse_node_count(env):
    import ctypes as C
    b = env.backend
    w, indices, values = _ledger_inputs(3)
    ask = _asked(3, indices)
    need = MC.shape(3, ask)[0]
    assert need > 1
    led = b.ledger_create(3)
    try:
        b.ledger_set_accounts(led, indices, values)
        val, present, nodes, root, n_nodes = np.zeros((len(ask), 14), np.uint64), np.zeros(len(ask), np.uint8), np.zeros((need, 7), np.uint64), np.zeros(7, np.uint64), C.c_uint32(0)
        from certificate_stark_amd._lib import check, u8p
        check(b.lib.cstark_ledger_open_multi(b.ctx, led, C.c_uint64(0), C.c_uint32(len(ask)), b._hptr(ask), b._hptr(val), b._hptr(present, u8p),
                                             b._hptr(nodes), C.c_uint32(need - 1), C.byref(n_nodes), b._hptr(root)))
    finally:
        b.ledger_destroy(led)


def _refuse_size(env):
    """2^25 points: refused before either buffer is looked at"""
    import ctypes as C
    from certificate_stark_amd._lib import check
    b = env.backend
    small = _dev(b, columns(6))
    out = b.empty_u64(1, WIDTH, 64)
    check(b.lib.cstark_lde_columns(b.ctx, b._ptr(small), b._ptr(out), C.c_uint32(WIDTH), C.c_uint32(25), C.c_uint32(0), C.c_uint64(b.field_lde_offset()),
                                   C.c_uint32(0), C.c_uint32(1)))


for _nm, _fn, _touch in (("count", _refuse_count, LEDGER_STATE), ("modulus", _refuse_modulus, set()), ("block", _refuse_block, set()),
                         ("window", _refuse_window, LEDGER_STATE), ("options", _refuse_options, LEDGER_STATE), ("node_count", _refuse_node_count, set()),
                         ("size", _refuse_size, set())):
    add("refused_%s" % _nm, "refused", _touch, _fn, lambda: b"CstarkError", refused=True)

GOOD = [op for op in OPS if not op.refused]
REFUSED = [op for op in OPS if op.refused]
FAMILIES = sorted(set(op.family for op in OPS))


# ---- what a context remembers: every data member of struct cstark_ctx ------------------------------------------------------------------------
# class: "handle" (made at creation, never replaced), "cache" (entries added on first use, found again by `key` -- the fields the lookup
# compares, as the code compares them), "block" (grow-only: freed and allocated anew for a larger request), "staging" (a pinned host
# block or the event that guards its reuse), "host" (a host-side copy or count), "timing".  ops: "family:<name>" or operation names.
def _s(cls, ops, key=None, of=None, note=None):
    return dict(cls=cls, ops=ops, key=key, of=of, note=note)


_TX, _SUB, _SCH = ["family:tx_prove", "ledger_d3_apply"], ["family:sub_air"], ["schnorr_2", "schnorr_4", "validate_schnorr_clean"]
_HOSTCH = ["tx_2_d3_sha3", "tx_2_d3_grind8", "range_bits_6_sha3"]
STATE = {
    "device": _s("handle", ["*"]), "stream": _s("handle", ["*"]), "owns_stream": _s("handle", ["*"]),
    "side": _s("handle", _TX + _SCH), "side2": _s("handle", _TX + _SCH),
    "ev_fork": _s("handle", _TX + _SCH), "ev_join": _s("handle", _TX + _SCH), "ev_join2": _s("handle", _TX + _SCH), "ev_mid": _s("handle", _TX + _SCH),
    "wit_buf": _s("block", _TX + ["merkle_d3", "schnorr_2"] + ["ledger_d%d_%s" % (d, k) for d in (3, 15) for k in ("apply", "checked", "open")], note="shared by the transaction and the Schnorr witness"),
    "wit_bytes": _s("host", _TX, of="wit_buf"),
    "wit": _s("host", _TX + _SCH, note="the view into wit_buf: rebound by every upload and by cstark_ledger_apply"),
    "plans": _s("cache", ["family:transform", "family:tx_prove", "family:sub_air"], key=("log_n",)),
    "cosets": _s("cache", ["family:transform", "family:tx_prove", "family:sub_air"], key=("log_n", "log_b", "offset")),
    "steps": _s("cache", ["step_n16_blk1024", "step2_n16_s127", "family:tx_prove"], key=("log_n", "log_b", "offset", "log_block", "split")),
    "periodic": _s("cache", _TX, key=("depth", "log_n", "log_b")),
    "small_periodic": _s("cache", ["merkle_d3", "schnorr_2", "rescue_16"], key=("air", "depth", "log_n", "log_b")),
    "assert_inv": _s("cache", _SUB, key=("log_n", "log_b", "m", "zc")),
    "air_static": _s("cache", _SUB, key=("air", "n_items", "log_n", "log_b"), note="the Merkle depth is not in the key"),
    "raw_periodic": _s("cache", ["family:validate"], key=("air", "depth")),
    "arena": _s("cache", _TX + _SUB, key=("air", "log_n", "log_b", "log_f", "layer.size()", "open_bytes"),
                note="one entry: replaced unless all of the key matches and open_bytes >= the query count"),
    "schnorr_seed": _s("cache", ["schnorr_2", "schnorr_2_alt"], key=("schnorr_seed_key",), note="one entry"),
    "schnorr_seed_key": _s("cache", ["schnorr_2", "schnorr_2_alt", "schnorr_2_other"], key=("schnorr_seed_key",),
                           note="12 bytes of the option set; zeroed only by cstark_schnorr_witness_upload"),
    "coef_buf": _s("block", _TX, note="one fixed size, allocated on first use"),
    "gfold_j": _s("block", _TX, note="one fixed size, uploaded on first use"),
    "coef_stage": _s("staging", _TX, of="coef_buf"), "coef_ev": _s("staging", _TX, of="coef_buf"),
    "air_coef_buf": _s("block", _SUB), "air_coef_stage": _s("staging", _SUB, of="air_coef_buf"), "air_coef_words": _s("host", _SUB, of="air_coef_buf"),
    "air_coef_ev": _s("staging", _SUB, of="air_coef_buf"),
    "deep_buf": _s("block", _HOSTCH), "deep_stage": _s("staging", _HOSTCH, of="deep_buf"), "deep_words": _s("host", _HOSTCH, of="deep_buf"),
    "deep_ev": _s("staging", _HOSTCH, of="deep_buf"),
    "desc_buf": _s("block", _TX + _SUB), "desc_bytes": _s("host", _TX + _SUB, of="desc_buf"),
    "part_ev": _s("timing", []), "part_timing": _s("timing", []), "part_valid": _s("timing", []),
    "lde_ev": _s("timing", []), "lde_ev_used": _s("timing", []), "lde_units": _s("timing", []),
    "tail_buf": _s("block", _SCH), "tail_bytes": _s("host", _SCH, of="tail_buf"),
    "schnorr_rx": _s("host", _SCH), "schnorr_av_stage": _s("host", _SCH), "schnorr_pub": _s("host", _SCH), "schnorr_s": _s("host", _SCH),
    "verify": _s("block", ["family:verify"], note="the verifier's arena, never shared with the prover's"),
    "ws": _s("block", ["family:transform", "family:tx_prove", "family:sub_air"]), "ws_bytes": _s("host", ["family:transform"], of="ws"),
    "shard_bit37": _s("block", ["shard_2_d3", "shard_4_d7"], note="written by a rank's share of a sharded proof alone, 8 n words"),
    "shard_bit37_words": _s("host", ["shard_2_d3", "shard_4_d7"], of="shard_bit37"),
    "rb_dev": _s("block", ["range_batch_3", "range_batch_40"]), "rb_host": _s("staging", ["range_batch_3", "range_batch_40"], of="rb_dev"),
    "rb_dev_bytes": _s("host", ["range_batch_3"], of="rb_dev"), "rb_host_bytes": _s("host", ["range_batch_3"], of="rb_dev"),
    "sig_buf": _s("block", ["family:sig", "ledger_d3_checked"]), "sig_bytes": _s("host", ["family:sig"], of="sig_buf"),
    "path_buf": _s("block", ["ledger_d3_open", "ledger_d15_open"]), "path_bytes": _s("host", ["ledger_d3_open"], of="path_buf"),
    "multi_buf": _s("block", ["ledger_d3_open", "ledger_d15_open", "multiproof_node_count"]), "multi_bytes": _s("host", ["ledger_d3_open"], of="multi_buf"),
    "val_buf": _s("block", ["family:validate"]), "val_bytes": _s("host", ["family:validate"], of="val_buf"),
}
CLASSES = ("handle", "cache", "block", "staging", "host", "timing")


def ctx_members(text):
    """the data members of struct cstark_ctx, parsed out of the text of csrc/ctx.h"""
    body = re.search(r"struct cstark_ctx \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for statement in body.split(";"):
        statement = re.sub(r"\{[^}]*\}", "", statement)           # brace initialisers
        statement = re.sub(r"\[[^\]]*\]", "", statement)          # array extents
        statement = re.sub(r"<[^>]*>", "", statement).strip()     # template arguments
        if not statement:
            continue
        for declarator in statement.split(","):
            m = re.search(r"(\w+)\s*(=.*)?$", declarator.strip(), re.S)
            assert m, declarator
            names.append(m.group(1))
    return names


def ops_of(spec):
    """the operations a STATE entry names"""
    out = []
    for s in spec:
        if s == "*":
            out += GOOD
        elif s.startswith("family:"):
            out += [op for op in OPS if op.family == s[7:]]
        else:
            out.append(BY_NAME[s])
    return out


# ---- schedules: pure functions of their seeds --------------------------------------------------------------------------------------------
# near-collision pairs (and triples): operations whose keys agree in all but one field, or that share a block under different sizes
PAIRS = {
    "merkle_depth": ["merkle_d3", "merkle_d15"],
    "tx_depth": ["tx_2_d3", "tx_2_d7", "tx_2_d15"],
    "log_n_10": LOG_N_10,
    "blowup": ["tx_2_d3", "tx_2_d3_b16"],
    "sub_air_blowup": ["rescue_16", "rescue_16_b16"],
    "air_static_blowup": ["merkle_combine_b4", "merkle_combine_b8"],
    "lde_blowup": ["lde_n10", "lde_n10_b16", "lde_n10_b2", "lde_n10_b4"],
    "lde_offset": ["lde_n10", "lde_n10_off_one", "lde_n10_off_g8"],
    "step_block": ["step_n16_blk1024", "step_n16_blk512"],
    "step_split": ["step2_n16_s127", "step2_n16_s255"],
    "folding": ["tx_2_d3", "tx_2_d3_f8r128"],
    "queries": ["tx_2_d3", "tx_2_d3_q96", "tx_2_d3_cubic42"],
    "hash": ["tx_2_d3", "tx_2_d3_sha3"],
    "pow_search": ["tx_2_d3_grind8", "tx_2_d3_grind15"],
    "schnorr_seed": ["schnorr_2", "schnorr_2_alt", "schnorr_2_other"],
    "resident_witness": ["tx_2_d3", "ledger_d3_apply"],
}


def pair_schedules(name):
    """A, B, (C, ...) twice over on one context, and the same from the other end: [[names], [names]].  In a set of four or more the
    members that are no neighbours in that cycle follow at the end of the first schedule, so that every member runs directly behind
    every other one"""
    ops = PAIRS[name]
    first, second = ops * 2, ops[::-1] * 2
    have = set(zip(first, first[1:])) | set(zip(second, second[1:]))
    for a in ops:
        for b in ops:
            if a != b and (a, b) not in have:
                first = first + ([b] if first[-1] == a else [a, b])
                have |= set(zip(first, first[1:]))
    return [first, second]


# grow-only block -> (a small request, a larger one, an operation between them that owns another block).  The sizes, as the code asks for
# them: ws 3 x 2^6 x 8 cosets against a 94-column trace of 2^12 rows; wit_buf one transfer at depth 3 against four at depth 7; desc_buf and
# deep_buf a 2-column trace of 2^6 rows against a 94-column one of 2^11 or 2^12; air_coef_buf RangeProofAir's 2 constraints and 2
# assertions against SchnorrAir's 56 and 61; tail_buf 2 against 4 signatures; verify one 64-row range proof against three transaction
# proofs; rb_dev 3 against 40 proofs; sig_buf 1 against 9 signatures; path_buf / multi_buf depth 3 against depth 15; val_buf one cycle of
# 64 rows against two of 1024; shard_bit37 8 x 2^11 against 8 x 2^12 words.  coef_buf and gfold_j have ONE size: their ladders walk
# first use and reuse, not growth.
LADDERS = {
    "ws": ("lde_n6", "tx_4_d7", "sig_check_1"),
    "wit_buf": ("tx_1_d3", "tx_4_d7", "lde_n6"),
    "coef_buf": ("tx_1_d3", "tx_4_d7", "sig_check_1"),
    "gfold_j": ("tx_1_d3", "tx_4_d7", "range_bits_6"),
    "desc_buf": ("range_bits_6", "tx_4_d7", "sig_check_1"),
    "air_coef_buf": ("range_bits_6", "schnorr_2", "lde_n6"),
    "deep_buf": ("range_bits_6_sha3", "tx_2_d3_sha3", "lde_n6"),
    "tail_buf": ("schnorr_2", "schnorr_4", "lde_n6"),
    "verify": ("air_verify_range", "tx_verify", "sig_check_1"),
    "rb_dev": ("range_batch_3", "range_batch_40", "sig_check_1"),
    "sig_buf": ("sig_check_1", "sig_check_9", "lde_n6"),
    "path_buf": ("ledger_d3_open", "ledger_d15_open", "sig_check_1"),
    "multi_buf": ("ledger_d3_open", "ledger_d15_open", "lde_n6"),
    "val_buf": ("validate_range_clean", "validate_tx_clean", "sig_check_1"),
    "shard_bit37": ("shard_2_d3", "shard_4_d7", "sig_check_1"),
}


def ladder_schedule(block):
    small, large, other = LADDERS[block]
    return [small, other, large, other, small]


SHUFFLE_SEEDS = [11, 23, 37, 41, 59, 67]


def shuffle_schedule(seed):
    """a permutation of the whole catalogue, refused calls included, run twice back to back"""
    names = [op.name for op in OPS]
    random.Random(seed).shuffle(names)
    return names * 2


def refusal_schedules():
    """[(G, X, G)]: every refused operation between two runs of three good operations from three other families"""
    out = []
    for k, x in enumerate(REFUSED):
        rng = random.Random(1000 + k)
        for fam in rng.sample([f for f in FAMILIES if f != "refused"], 3):
            g = rng.choice([op for op in GOOD if op.family == fam])
            out.append([g.name, x.name, g.name])
    return out


def log_n_of(name):
    """the trace length an operation works at, read from its expectation: the header of a proof (include/cstark.h: log_n is the word at
    byte 16), or the row count of a transform's coefficient table"""
    want = BY_NAME[name].expectation
    if isinstance(want, bytes):
        return struct.unpack_from("<I", want, 16)[0]
    assert BY_NAME[name].family == "transform", name
    return want[0].shape[-1].bit_length() - 1


def two_context_schedules():
    """two schedules of one length whose operations differ in log_n at every step"""
    a = ["tx_1_d3", "tx_2_d3", "lde_n6", "tx_4_d7", "merkle_d3", "tx_2_d7", "range_bits_6", "step_n16_blk1024", "tx_1_d3", "tx_2_d3"]
    b = ["tx_2_d3", "tx_1_d3", "lde_n14", "tx_2_d7", "schnorr_4", "tx_4_d7", "lde_n10", "rescue_16", "tx_2_d7", "tx_1_d3"]
    return a, b


def first_call_names():
    """the cold starts: every operation of every family is once the very first call of a fresh context, the refused calls among them"""
    return [op.name for op in OPS]


def all_schedules():
    """every schedule the GPU tests run on ONE context, by name: what test_context_history_cpu.py reasons about"""
    out = {}
    for name in PAIRS:
        for k, s in enumerate(pair_schedules(name)):
            out["pair:%s:%d" % (name, k)] = s
    for block in LADDERS:
        out["ladder:%s" % block] = ladder_schedule(block)
    for seed in SHUFFLE_SEEDS:
        out["shuffle:%d" % seed] = shuffle_schedule(seed)
    for k, s in enumerate(refusal_schedules()):
        out["refusal:%d" % k] = s
    for k, s in enumerate(two_context_schedules()):
        out["two_contexts:%d" % k] = s
    for name in first_call_names():
        out["cold:%s" % name] = [name]
    return out


def proof_digest(proof):
    return hashlib.sha256(proof).hexdigest()
