"""cstark_schnorr_public_at (k_vfy_schnorr_public + k_vfy_schnorr_public_sum, csrc/verify.hip): SchnorrAir's 19 public-input columns and
12 sequence-value polynomials at one point z, formed as barycentric sums over the trace domain, against the oracle's evaluation of the
interpolated columns (oracle.interpolate_columns + evaluate_polys_at / evaluate_polys_at_ext), bit for bit.

Sizes: 1 signature (the sequence polynomials are constants), 2 (half a workgroup of the kernel: it holds four signatures), 4 (one full
workgroup), 8 (two workgroups, two partial blocks for the second launch to add).  Operands: statement words 0 and p - 1 beside random
ones, an all-zero statement; z random, an embedded base-field point, the adjoined root, 0, p - 1 in component 0."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0x4180000000000001
SIZES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


class Statement:
    def __init__(self, messages, sig_rx):
        self.n_sig, self.messages, self.sig_rx = messages.shape[0], messages, sig_rx
        self.sig_s = np.zeros((self.n_sig, 32), np.uint8)


@functools.lru_cache(maxsize=None)
def statement(n_sig, kind):
    """random field elements (memory form); "extremes": 0 and p - 1 in the first and last signature, in a public-key word, a word of each
    of the four hash-input rows and an R.x word; "zero": all zero"""
    rng = np.random.default_rng(100 + n_sig)
    msg = rng.integers(0, P, size=(n_sig, 28), dtype=np.uint64)
    rx = rng.integers(0, P, size=(n_sig, 6), dtype=np.uint64)
    if kind == "zero":
        msg[:], rx[:] = 0, 0
    else:
        for t, v in ((0, P - 1), (n_sig - 1, 0)):
            msg[t, [3, 11, 12, 20, 27]] = v
            rx[t, [0, 5]] = v
        msg[0, 0], msg[0, 7], msg[0, 14], msg[0, 21], rx[0, 1] = 0, P - 1, 0, P - 1, 0
    return Statement(msg, rx)


@functools.lru_cache(maxsize=None)
def reference_columns(n_sig, kind):
    """coefficient columns [31][512 n_sig] of the statement: the interpolated public-input columns, then the sequence polynomials"""
    from oracle import oracle as O
    w = statement(n_sig, kind)
    log_n = 9 + n_sig.bit_length() - 1
    cols = np.concatenate([O.interpolate_columns(O.schnorr_aux_columns(w)), O.schnorr_assertion_polys(w, log_n)])
    cols.setflags(write=False)
    return cols


def reference_at(n_sig, kind, z):
    from oracle import oracle as O
    cols = reference_columns(n_sig, kind)
    z = np.asarray(z, np.uint64)
    if z.size == 1:
        return O.evaluate_polys_at(cols, z)[0].reshape(31, 1)
    return O.evaluate_polys_at_ext(cols, z)


def points(m, seed):
    from oracle import oracle as O
    one = int(O.to_mont([1])[0])
    rng = np.random.default_rng(seed)
    r = rng.integers(0, P, size=m, dtype=np.uint64)
    zs = {"random": r, "zero": np.zeros(m, np.uint64), "p-1": np.concatenate([[P - 1], r[1:]]).astype(np.uint64)}
    if m > 1:
        zs["embedded"] = np.concatenate([r[:1], np.zeros(m - 1, np.uint64)]).astype(np.uint64)
        root = np.zeros(m, np.uint64)
        root[1] = one
        zs["adjoined root"] = root
    return zs


@pytest.mark.parametrize("n_sig", SIZES)
def test_public_values_match_the_interpolated_columns(backend, oracle, n_sig):
    for m in (1, 2, 3):
        for name, z in points(m, 7 * n_sig + m).items():
            got = backend.schnorr_public_at(statement(n_sig, "extremes").messages, statement(n_sig, "extremes").sig_rx, z)
            want = reference_at(n_sig, "extremes", z)
            assert got.shape == want.shape == (31, m)
            assert (got == want).all(), (n_sig, m, name, np.argwhere(got != want)[:4].tolist())


def test_one_signature_has_constant_sequence_polynomials(backend, oracle):
    st = statement(1, "extremes")
    for m in (1, 2, 3):
        got = backend.schnorr_public_at(st.messages, st.sig_rx, points(m, 3)["random"])
        assert (got[19:25, 0] == st.sig_rx[0]).all() and (got[25:31, 0] == st.sig_rx[0]).all() and not got[19:, 1:].any()


def test_all_zero_statement(backend, oracle):
    for n_sig in (2, 8):
        st = statement(n_sig, "zero")
        for m in (1, 3):
            z = points(m, 5)["random"]
            got = backend.schnorr_public_at(st.messages, st.sig_rx, z)
            assert not got.any() and (got == reference_at(n_sig, "zero", z)).all()


def test_points_of_the_trace_domain_and_other_misuse(backend, oracle):
    from certificate_stark_amd._lib import CstarkError
    from oracle import verifier as V
    one = int(oracle.to_mont([1])[0])
    st = statement(2, "extremes")
    w = V.to_mont(V.root_of_unity(10))
    for m in (1, 2, 3):
        for z0 in (one, w, V.to_mont(pow(V.root_of_unity(10), 1023, P))):
            with pytest.raises(CstarkError):
                backend.schnorr_public_at(st.messages, st.sig_rx, [z0] + [0] * (m - 1))
    z = points(1, 1)["random"]
    with pytest.raises(CstarkError):   # three signatures: not a trace length
        backend.schnorr_public_at(np.zeros((3, 28), np.uint64), np.zeros((3, 6), np.uint64), z)
    with pytest.raises(CstarkError):
        backend.schnorr_public_at(st.messages, st.sig_rx, [P])
    bad = np.array(st.messages, copy=True)
    bad[1, 27] = P
    with pytest.raises(CstarkError):
        backend.schnorr_public_at(bad, st.sig_rx, z)
    with pytest.raises(CstarkError):
        backend.schnorr_public_at(st.messages, st.sig_rx, np.zeros(4, np.uint64))
