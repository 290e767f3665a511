"""Two-level block columns (one value on rows [0, R) of every block of B rows and another on rows [R, B), as TransactionAir's tree-root
registers 58..64 with B = 1024 and R = 8 depth + 7): coefficients and low-degree extension through cstark_step2_columns against the
general path on the same inputs, interpolate_columns + lde_columns, which the rest of the suite pins to the oracle.  Field arithmetic
is exact and both paths write canonical elements: equality is bit for bit, coefficients and all eight cosets.

Sizes: 2^16 and 2^18 (the v4 row kernels), 2^20 once (the v5 row kernel) -- the smallest that reach each kernel -- and 2^14, which is no
three-step size: there the entry point takes the general path itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG_B = 3
COLUMNS = ["random", "random", "random", "random", "u_equals_v", "v_zero", "u_zero", "p_minus_1"]   # the eight columns of every table
SHAPES = ([(16, 1024, r) for r in (1, 127, 255, 1023)] + [(16, 512, r) for r in (1, 127, 255, 511)] +
          [(18, 1024, r) for r in (1, 127, 255, 1023)] + [(20, 1024, 127), (14, 1024, 127)])


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def two_level_table(log_n, block, split, p):
    """[8][n] evaluations (memory form: any value below p is an element) and the [8][t] values u (rows < split) and v (rows >= split)"""
    n = 1 << log_n
    t = n // block
    rng = np.random.default_rng(2000 + 64 * log_n + split + block)
    u = rng.integers(0, p, size=(len(COLUMNS), t), dtype=np.uint64)
    v = rng.integers(0, p, size=(len(COLUMNS), t), dtype=np.uint64)
    for c, kind in enumerate(COLUMNS):
        if kind == "u_equals_v":
            u[c] = v[c]
        elif kind == "v_zero":
            v[c] = 0
        elif kind == "u_zero":
            u[c] = 0
        elif kind == "p_minus_1":
            u[c] = v[c] = p - 1
    rows = np.arange(n) % block < split
    return np.where(rows[None, :], np.repeat(u, block, axis=1), np.repeat(v, block, axis=1))


@pytest.mark.parametrize("log_n,block,split", SHAPES)
def test_step2_columns_equal_the_general_path(backend, oracle, log_n, block, split):
    evals = backend.from_numpy_u64(two_level_table(log_n, block, split, oracle.P))
    ref_coeffs = backend.interpolate_columns(evals.clone())
    ref_lde = backend.lde_columns(ref_coeffs, LOG_B)
    sentinel = -2   # 2^64 - 2 is no element
    for col0, ncols in ((0, 8), (1, 7), (3, 1)):   # column counts 8, 7 and 1
        coeffs = torch.full_like(ref_coeffs, sentinel)
        lde = torch.full_like(ref_lde, sentinel)
        work = evals.clone()
        backend.step2_columns(work, block, split, LOG_B, col0=col0, ncols=ncols, coeffs=coeffs, lde=lde)
        assert torch.equal(coeffs[col0:col0 + ncols], ref_coeffs[col0:col0 + ncols]), (col0, ncols)
        assert torch.equal(lde[:, col0:col0 + ncols], ref_lde[:, col0:col0 + ncols]), (col0, ncols)
        # the other columns are not written
        assert (coeffs[:col0] == sentinel).all() and (coeffs[col0 + ncols:] == sentinel).all()
        assert (lde[:, :col0] == sentinel).all() and (lde[:, col0 + ncols:] == sentinel).all()
        if log_n != 14:   # only rows 0 and `split` of every block are read
            assert torch.equal(work, evals)
    # u = v is a step column: the one-level entry point writes the same
    k = COLUMNS.index("u_equals_v")
    c1, l1 = backend.step_columns(evals.clone(), block, LOG_B, col0=k, ncols=1)
    assert torch.equal(c1[k], ref_coeffs[k]) and torch.equal(l1[:, k], ref_lde[:, k])
    # all values p - 1 is the constant column: nothing but c_0
    k = COLUMNS.index("p_minus_1")
    assert not ref_coeffs[k, 1:].any()


def test_step2_columns_coset_range(backend, oracle):
    evals = backend.from_numpy_u64(two_level_table(16, 1024, 127, oracle.P))
    ref_lde = backend.lde_columns(backend.interpolate_columns(evals.clone()), LOG_B, k0=2, nk=3)
    _, lde = backend.step2_columns(evals.clone(), 1024, 127, LOG_B, k0=2, nk=3)
    assert torch.equal(lde, ref_lde)


def test_step2_columns_refuse_a_split_outside_the_block(backend, oracle):
    from certificate_stark_amd._lib import CstarkError
    for log_n in (14, 16):   # on the general path as on the step path
        evals = backend.from_numpy_u64(two_level_table(log_n, 1024, 127, oracle.P))
        for split in (0, 1024, 1025, 1 << 20):
            with pytest.raises(CstarkError):
                backend.step2_columns(evals.clone(), 1024, split, LOG_B)
