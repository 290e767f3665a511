"""Step columns (columns constant over blocks of 1024 rows, as TransactionAir's registers 65..91): coefficients and low-degree
extension through cstark_step_columns against the general path on the same inputs, interpolate_columns + lde_columns, which the
rest of the suite pins to the oracle.  Field arithmetic is exact and both paths write canonical elements: equality is bit for bit.

Sizes: 2^16 and 2^18 (the v4 row kernels, T = 64 and 256 block values per column), 2^20 (the v5 row kernel, T = 1024) -- the
smallest that reach each kernel -- and 2^14, which is no three-step size: there the entry point takes the general path itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK, LOG_B, COLS = 1024, 3, 3
CASES = ["random", "zero", "p_minus_1", "single_transaction", "all_equal"]
SIZES = [14, 16, 18, 20]


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def block_values(case, t, rng, p):
    """[COLS][t] block values (memory form: any value below p is an element)."""
    g = np.zeros((COLS, t), np.uint64)
    if case == "random":
        g[:] = rng.integers(0, p, size=(COLS, t), dtype=np.uint64)
    elif case == "p_minus_1":
        g[:] = p - 1
    elif case == "single_transaction":   # the first, the last, one in the middle
        g[0, 0], g[1, t - 1], g[2, t // 2 + 1] = rng.integers(1, p, size=3, dtype=np.uint64)
    elif case == "all_equal":
        g[0, :], g[1, :], g[2, :] = 1, p - 1, rng.integers(1, p, dtype=np.uint64)
    return g


_tables = {}


def tables(backend, oracle, log_n):
    """The five cases side by side as one table of 15 columns, and its coefficients and cosets by the general path: once per size."""
    if log_n not in _tables:
        n = 1 << log_n
        rng = np.random.default_rng(1000 + log_n)
        g = np.concatenate([block_values(c, n // BLOCK, rng, oracle.P) for c in CASES])
        evals = backend.from_numpy_u64(np.repeat(g, BLOCK, axis=1))
        coeffs = backend.interpolate_columns(evals.clone())
        lde = backend.lde_columns(coeffs, LOG_B)
        _tables[log_n] = (evals, coeffs, lde)
    return _tables[log_n]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("log_n", SIZES)
def test_step_columns_equal_the_general_path(backend, oracle, log_n, case):
    evals, ref_coeffs, ref_lde = tables(backend, oracle, log_n)
    col0 = COLS * CASES.index(case)
    sentinel = -2   # 2^64 - 2 is no element
    coeffs = torch.full_like(ref_coeffs, sentinel)
    lde = torch.full_like(ref_lde, sentinel)
    backend.step_columns(evals.clone(), BLOCK, LOG_B, col0=col0, ncols=COLS, coeffs=coeffs, lde=lde)
    assert torch.equal(coeffs[col0:col0 + COLS], ref_coeffs[col0:col0 + COLS])     # the whole coefficient table
    assert torch.equal(lde[:, col0:col0 + COLS], ref_lde[:, col0:col0 + COLS])     # all eight cosets
    if case == "all_equal":   # a constant column: nothing but c_0
        assert not coeffs[col0:col0 + COLS, 1:].any() and coeffs[col0:col0 + COLS, 0].all()
    # the other columns are not written
    mask = torch.ones(ref_coeffs.shape[0], dtype=torch.bool, device=coeffs.device)
    mask[col0:col0 + COLS] = False
    assert (coeffs[mask] == sentinel).all() and (lde[:, mask] == sentinel).all()


@pytest.mark.parametrize("log_n", [14, 16])
def test_step_columns_coset_range(backend, oracle, log_n):
    evals, ref_coeffs, ref_lde = tables(backend, oracle, log_n)
    _, lde = backend.step_columns(evals.clone(), BLOCK, LOG_B, k0=2, nk=3)
    assert torch.equal(lde, ref_lde[2:5])


def test_step_columns_leave_the_evaluations_intact_on_the_new_path(backend, oracle):
    evals, ref_coeffs, _ = tables(backend, oracle, 16)
    work = evals.clone()
    coeffs, _ = backend.step_columns(work, BLOCK, LOG_B)
    assert torch.equal(work, evals) and torch.equal(coeffs, ref_coeffs)


def test_step_columns_refuse_bad_arguments(backend, oracle):
    from certificate_stark_amd._lib import CstarkError
    evals, _, _ = tables(backend, oracle, 14)
    for kw in (dict(block_len=1000), dict(block_len=0), dict(block_len=1 << 15), dict(block_len=BLOCK, col0=14, ncols=2),
               dict(block_len=BLOCK, k0=6, nk=3)):
        with pytest.raises(CstarkError):
            backend.step_columns(evals.clone(), kw.pop("block_len"), LOG_B, **kw)


def test_transaction_proof_at_64_transactions_keeps_its_bytes():
    """Routing: cstark_tx_prove at 2^16 rows sends registers 65..91 through the step path; the proof is the CPU restatement's, byte
    for byte (witness and expectation of tests/test_gpu_prove.py::test_proof_bytes_equal_the_cpu_restatement)."""
    from oracle import oracle as O
    from oracle import prover as OP
    from certificate_stark_amd.prover import ProofOptions, TransactionExample, TransactionMetadata
    n_tx, depth, opts = 64, 15, (96, 8, 0, 0, 0, 4, 256)
    w = O.TxWitness.generate(n_tx, depth, seed=77 + n_tx)
    meta = TransactionMetadata(*[getattr(w, f) for f in TransactionMetadata.FIELDS])
    tx = TransactionExample(ProofOptions(*opts), meta)
    assert tx.prove() == OP.prove(w, opts)
