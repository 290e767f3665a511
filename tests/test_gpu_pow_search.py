"""GPU: the proof-of-work searches on chosen seeds and windows -- the chunk kernels k_grind, k_grind_batch (csrc/blake3.hip) and
k_grind_sha3 (csrc/sha3.hip) against a Python scan of the same window, the chunk loop of the prover's grind_nonce (csrc/prove.hip,
grind_search) with small chunks against the sequential search, and the batched range prover on a batch one of whose searches goes
beyond its first chunk.  A whole proof at <= 15 bits finds its nonce in the first chunk of 2^22 and below 2^32: the nonce's high
word, a window that is no multiple of the workgroup, a second chunk, and the batch kernels' rule for seeds that are already served
(found[t] < base) or carry a preset minimum were reached by chance or never."""
import functools

import numpy as np
import pytest

import tail_cases as T

pytestmark = pytest.mark.gpu

# (form of cstark_debug_grind_chunk, hash function): k_grind, k_grind_batch, k_grind_sha3
FORMS = [(0, 0), (1, 0), (2, 1)]
FORM_IDS = ["k_grind", "k_grind_batch", "k_grind_sha3"]


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def dev(oracle, backend):
    return T.Dev(backend)


@functools.lru_cache(maxsize=None)
def scan(seed, base, count, bits, hash_fn):
    """the reference, computed once per window and shared by the forms"""
    return T.pow_scan(seed, base, count, bits, hash_fn)


def chunk(dev, form, seeds, base, count, bits, presets=None):
    """one chunk launch for the seeds (one seed for form 0) -> found[len(seeds)]"""
    presets = [T.NONE64] * len(seeds) if presets is None else presets
    if form == 0:
        assert len(seeds) == 1
        found_t = dev.u64([12345])            # grind_chunk presets the word itself
        assert dev.grind_chunk(0, seeds[0], 1, base, count, bits, found_t) == T.HIP_SUCCESS
    else:
        found_t, seeds_t = dev.u64(presets + [777]), dev.raw(b"".join(seeds))
        assert dev.grind_chunk(form, seeds_t, len(seeds), base, count, bits, found_t) == T.HIP_SUCCESS
        assert dev.get_u64(found_t)[len(seeds):] == [777], "the word behind found[batch] was written"
    return dev.get_u64(found_t)[:len(seeds)]


# the nonce's low word alone, a count that is no multiple of 256, a window across 2^32, one above it, one far above at an odd base
WINDOWS = [(1, 4096), (1, 1000), (2**32 - 512, 1024), (2**32, 512), (2**40 + 3, 777)]


@pytest.mark.parametrize("form,hash_fn", FORMS, ids=FORM_IDS)
def test_windows_against_a_python_scan(dev, form, hash_fn):
    for k, (base, count) in enumerate(WINDOWS):
        seed = T.tagged("pow-window", k)
        want = scan(seed, base, count, 8, hash_fn)
        assert want != T.NONE64                                                  # (a window of >= 512 at 8 bits: e^-2 at worst; pinned seeds)
        assert chunk(dev, form, [seed], base, count, 8) == [want], (base, count)
        assert chunk(dev, form, [seed], base, count, 0) == [base], (base, count)  # 0 bits: every nonce serves
        assert chunk(dev, form, [seed], base, count, 1) == [scan(seed, base, count, 1, hash_fn)], (base, count)


# Steered seeds: i of tagged("pow", i), one set per hash function, found by tail_cases.search("pow", wanted) with the properties
# re-derived below.  Window [7, 307) at 8 bits: two workgroups, the second one padded by 212 lanes.
BASE, COUNT, BITS = 7, 300, 8
ONLY_BEHIND_THE_WINDOW = {0: 6, 1: 1}      # no hit inside, at least one in [307, 519): the padded lanes' nonces
HIT_AT_BASE = {0: 526, 1: 353}
FIRST_HIT_AT_LAST = {0: 1542, 1: 937}
NO_HIT_AT_20_BITS = {0: 0, 1: 0}           # window [1, 301)


@pytest.mark.parametrize("form,hash_fn", FORMS, ids=FORM_IDS)
def test_steered_seeds_at_the_edges_of_a_window(dev, form, hash_fn):
    seed = T.tagged("pow", ONLY_BEHIND_THE_WINDOW[hash_fn])
    T.require(scan(seed, BASE, COUNT, BITS, hash_fn) == T.NONE64 and scan(seed, BASE + COUNT, 512 - COUNT, BITS, hash_fn) != T.NONE64,
              "hits only at indices count .. 511")
    assert chunk(dev, form, [seed], BASE, COUNT, BITS) == [T.NONE64]
    seed = T.tagged("pow", HIT_AT_BASE[hash_fn])
    T.require(scan(seed, BASE, COUNT, BITS, hash_fn) == BASE, "a hit at base")
    assert chunk(dev, form, [seed], BASE, COUNT, BITS) == [BASE]
    seed = T.tagged("pow", FIRST_HIT_AT_LAST[hash_fn])
    T.require(scan(seed, BASE, COUNT, BITS, hash_fn) == BASE + COUNT - 1, "the only hit at base + count - 1")
    assert chunk(dev, form, [seed], BASE, COUNT, BITS) == [BASE + COUNT - 1]
    assert chunk(dev, form, [seed], BASE, COUNT - 1, BITS) == [T.NONE64]         # ... and one nonce fewer misses it
    seed = T.tagged("pow", NO_HIT_AT_20_BITS[hash_fn])
    T.require(scan(seed, 1, 300, 20, hash_fn) == T.NONE64, "no hit at 20 bits")
    assert chunk(dev, form, [seed], 1, 300, 20) == [T.NONE64]


@pytest.mark.parametrize("form,hash_fn", FORMS[1:], ids=FORM_IDS[1:])
def test_batch_forms_with_preset_minima(dev, form, hash_fn):
    """five seeds in one launch: found[t] preset to ~0 | below base (served by an earlier chunk: unchanged) | inside the window above
    the true minimum (lowered) | inside the window below every hit (kept) | far below base (unchanged); then the next chunk on the
    results, which must leave every served seed alone"""
    base, count, bits = 1000, 1000, 8
    seeds = [T.tagged("pow-batch", t) for t in range(5)]
    mins = [scan(s, base, count, bits, hash_fn) for s in seeds]
    T.require(all(base < v < base + count - 1 for v in mins), "every seed has its first hit strictly inside the window")
    presets = [T.NONE64, base - 1, base + count - 1, mins[3] - 1, 5]
    want = [mins[0], base - 1, mins[2], mins[3] - 1, 5]
    got = chunk(dev, form, seeds, base, count, bits, presets)
    assert got == want
    assert chunk(dev, form, seeds, base + count, count, bits, got) == want
    # a seed that is still unserved is searched by the next chunk while its neighbours are skipped
    presets = [mins[0], T.NONE64, mins[2], T.NONE64, 5]
    want = [mins[0], scan(seeds[1], base + count, count, bits, hash_fn), mins[2], scan(seeds[3], base + count, count, bits, hash_fn), 5]
    assert chunk(dev, form, seeds, base + count, count, bits, presets) == want


# The chunk loop: i of tagged("pow", i) whose smallest nonce lies in the first chunk | in a later chunk, not on its first nonce | exactly
# on the first nonce 1 + k chunk of a later chunk.  (hash function, bits, chunk) -> the three i
LOOP_SEEDS = {(0, 12, 512): (4, 3, 42), (0, 12, 1000): (3, 0, 466), (0, 13, 512): (31, 39, 839), (0, 13, 1000): (31, 1, 466),
              (1, 12, 512): (7, 0, 614), (1, 12, 1000): (0, 1, 6683), (1, 13, 512): (15, 0, 435), (1, 13, 1000): (0, 1, 6683)}


@pytest.mark.parametrize("hash_fn,bits,size", sorted(LOOP_SEEDS))
def test_chunk_loop_against_the_sequential_search(dev, hash_fn, bits, size):
    first, later, boundary = (T.tagged("pow", i) for i in LOOP_SEEDS[hash_fn, bits, size])
    want = [T.pow_sequential(s, bits, hash_fn) for s in (first, later, boundary)]
    T.require(want[0] <= size, "smallest nonce in the first chunk")
    T.require(want[1] > size and (want[1] - 1) % size != 0, "smallest nonce inside a later chunk")
    T.require(want[2] > size and (want[2] - 1) % size == 0, "smallest nonce on the first nonce of a later chunk")
    assert [dev.grind_search(s, hash_fn, bits, size) for s in (first, later, boundary)] == want


# The batched range prover searches chunks of 4 << bits nonces for all its proofs at once.  Of the 100 proofs of
# test_gpu_pinned_proofs.py::test_batched_range_proofs_equal_single_proofs, computed with oracle/prover.py: at 13 bits (Blake3) the
# largest nonce is 32434, below the chunk of 32768 -- the second chunk of k_grind_batch never ran; at 12 bits (Sha3) three proofs
# (34, 55, 87) lie in the second chunk of 16384.  The values below were added one by one from 1000 upwards until the CPU prover's nonce
# left the first chunk: 1040 -> 52133 and 1051 -> 38318 (second chunk of 32768); 1075 -> 26030 (second), 1135 -> 37997 (third of 16384).
@pytest.mark.parametrize("opts,values,chunks", [((20, 8, 13, 0, 0, 4, 256), [17, 1040, 0, 1051, 1], [1, 2, 1, 2, 1]),
                                                ((20, 8, 12, 1, 0, 4, 256), [1135, 17, 1075, 0, 1], [3, 1, 2, 1, 1])])
def test_batched_range_prover_beyond_its_first_chunk(oracle, backend, opts, values, chunks):
    """one batch in which some searches end in the first chunk and others in the second or third: every proof equals the single
    prover's and the CPU prover's bytes"""
    from oracle import prover as OP
    from oracle import verifier as V
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import ProofOptions
    numbers = oracle.to_mont(np.array(values, np.uint64))
    want = [OP.prove_air(oracle.AIR_RANGE, int(n), opts) for n in numbers]
    size = 4 << opts[2]
    T.require([(V.parse(p)["nonce"] - 1) // size + 1 for p in want] == chunks, "the chunk every proof's nonce lies in")
    proofs = backend.range_prove_batch(ProofOptions(*opts), numbers)
    assert list(proofs) == want
    for i, n in enumerate(numbers):
        assert proofs[i] == backend.air_prove(Backend.AIR_RANGE, ProofOptions(*opts), int(n)), i
        assert V.verify_range(proofs[i], int(n), options=list(opts))


def test_whole_proof_at_20_bits():
    """a TransactionAir proof at grinding factor 20 against oracle/prover.py (the suite's largest was 15): the CPU prover's sequential
    search ends at nonce 15531 for this witness and takes 1.4 s in all"""
    from oracle import oracle as O
    from oracle import prover as OP
    from oracle import verifier as V
    from certificate_stark_amd.prover import ProofOptions, TransactionExample, TransactionMetadata
    opts = (20, 8, 20, 0, 0, 4, 256)
    w = O.TxWitness.generate(2, 3, seed=79)
    tx = TransactionExample(ProofOptions(*opts), TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS]))
    proof = tx.prove()
    assert proof == OP.prove(w, opts)
    assert V.verify(proof, *tx.pub_inputs(), options=list(opts))


def test_sha3_reference_is_sha3(oracle):
    """the reference of the Sha3 cases is SHA3-256: oracle.digest(., 1) beside hashlib"""
    import hashlib
    for i in (0, 1, 937):
        data = T.tagged("pow", i) + T.le64(2**40 + i)
        assert oracle.digest(data, 1) == hashlib.sha3_256(data).digest()
