"""The account ledger on the GPU (cstark_ledger_*, prover.Ledger) against the oracle's witness generator: a ledger that holds a case's
initial accounts and applies its transfers must give the generator's eleven arrays bit for bit, leave them resident as an upload would,
compose over batches, and refuse what cannot be applied without changing anything."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as LC

pytestmark = pytest.mark.gpu

P = 2**62 + 2**56 + 2**55 + 1


@pytest.fixture(scope="module")
def backend():
    from certificate_stark_amd.backend import Backend
    b = Backend()
    yield b
    b.close()


def _ledger(backend, w, values=None):
    from certificate_stark_amd.prover import Ledger
    indices, initial = LC.initial_accounts(w)
    led = Ledger(w.depth, backend)
    led.set_accounts(indices, initial if values is None else values)
    return led, indices


def _transfers(w, lo=0, hi=None):
    return tuple(getattr(w, f)[lo:hi] for f in ("s_indices", "r_indices", "deltas", "sig_rx", "sig_s"))


def _assert_batch(m, w, lo=0, hi=None):
    """the eleven arrays of an applied batch against transfers [lo, hi) of the reference"""
    hi = w.n_tx if hi is None else hi
    for f in ("initial_roots", "s_old_values", "r_old_values", "s_indices", "r_indices", "s_paths", "r_paths", "deltas", "sig_rx", "sig_s"):
        assert np.array_equal(getattr(m, f), getattr(w, f)[lo:hi]), f
    assert np.array_equal(m.final_root, w.final_root if hi == w.n_tx else w.initial_roots[hi]), "final_root"
    assert m.n_tx == hi - lo and m.depth == w.depth


def _parity(backend, w):
    led, indices = _ledger(backend, w)
    assert np.array_equal(led.root(), w.initial_roots[0])
    m = led.apply(_transfers(w))
    _assert_batch(m, w)
    assert np.array_equal(led.root(), w.final_root)
    values, present = led.accounts(indices)
    assert present.all() and np.array_equal(values, LC.final_accounts(w, indices))
    led.close()


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_apply_reproduces_the_generator(backend, case):
    _parity(backend, LC.generated(case))


def test_apply_reproduces_the_committed_1024_transfer_witness(backend):
    _parity(backend, LC.golden_1024())


def test_resident_witness_is_the_uploaded_one(backend):
    from certificate_stark_amd.backend import to_numpy_u64
    from certificate_stark_amd.prover import get_example_options
    w = LC.generated((2, 3, 2))
    backend.upload_witness(w)
    trace_ref = to_numpy_u64(backend.build_trace()).copy()
    proof_ref = backend.prove(get_example_options())
    backend.upload_witness(LC.generated((2, 3, 1)))   # another batch is resident when apply runs: apply must replace all of it
    led, _ = _ledger(backend, w)
    backend.resident = object()
    led.apply(_transfers(w), want_witness=False)
    assert backend.resident is None and (backend.n_tx, backend.depth) == (2, 3)
    assert np.array_equal(to_numpy_u64(backend.build_trace()), trace_ref)
    proof = backend.prove(get_example_options())
    assert proof == proof_ref
    assert list(backend.tx_verify([proof], w.initial_roots[0], w.final_root)) == [0]
    led.close()


def test_batches_compose(backend):
    w = LC.generated((16, 3, 3))
    led, _ = _ledger(backend, w)
    first = led.apply(_transfers(w, 0, 8))
    _assert_batch(first, w, 0, 8)
    second = led.apply(_transfers(w, 8, 16))
    _assert_batch(second, w, 8, 16)
    assert np.array_equal(second.initial_roots[0], first.final_root)
    assert np.array_equal(led.root(), w.final_root)
    led.close()


def test_set_accounts(backend, oracle):
    from certificate_stark_amd.prover import Ledger
    w = LC.generated((16, 15, 5))
    indices, initial = LC.initial_accounts(w)
    final = LC.final_accounts(w, indices)
    h = len(indices) // 2
    two = Ledger(15, backend)
    two.set_accounts(indices[:h], initial[:h])
    two.set_accounts(indices[h:], initial[h:])
    one = Ledger(15, backend)
    one.set_accounts(indices, initial)
    assert np.array_equal(one.root(), two.root()) and np.array_equal(one.root(), w.initial_roots[0])
    # an overwrite gives the root of a fresh ledger built from the final values (which is the applied batch's final root)
    one.set_accounts(indices, final)
    fresh = Ledger(15, backend)
    fresh.set_accounts(indices, final)
    assert np.array_equal(one.root(), fresh.root()) and np.array_equal(one.root(), w.final_root)
    values, present = one.accounts(np.concatenate([indices, np.array([LC.absent_index(w, indices)], np.uint64)]))
    assert present[:-1].all() and not present[-1] and np.array_equal(values[:-1], final) and not values[-1].any()
    for led in (one, two, fresh):
        led.close()
    # an empty ledger's root: depth-many merges of the zero digest
    for depth in (1, 3, 7, 15, 31):
        e = np.zeros(7, np.uint64)
        for _ in range(depth):
            out = np.zeros(7, np.uint64)
            oracle.lib().cso_rescue_merge(oracle._p(e.copy()), oracle._p(e.copy()), oracle._p(out))
            e = out
        led = Ledger(depth, backend)
        assert np.array_equal(led.root(), e), depth
        led.close()


def _refusal(name, w, lo, at, oracle):
    """transfers [lo, n) of w with transfer lo + at made unappliable"""
    s, r, d, rx, ss = (a.copy() for a in _transfers(w, lo))
    indices, _ = LC.initial_accounts(w)
    if name == "index":
        r[at] = 1 << w.depth
    elif name == "self":
        r[at] = s[at]
    elif name == "absent":
        s[at] = LC.absent_index(w, indices)
    else:
        d[at] = oracle.to_mont(np.array([P - 1], np.uint64))[0]   # canonical p - 1: above every balance the generator draws
    return s, r, d, rx, ss


@pytest.mark.parametrize("name,reason", [("index", 1), ("self", 2), ("absent", 3), ("balance", 4)])
def test_refusals_change_nothing(backend, oracle, name, reason):
    from certificate_stark_amd.prover import TransferRefused, get_example_options
    w = LC.generated((8, 7, 4))
    led, _ = _ledger(backend, w)
    _assert_batch(led.apply(_transfers(w, 0, 4)), w, 0, 4)
    previous = backend.prove(get_example_options())
    root = led.root()
    with pytest.raises(TransferRefused) as e:
        led.apply(_refusal(name, w, 4, 2, oracle))
    assert (e.value.index, e.value.reason) == (2, reason)
    assert np.array_equal(led.root(), root)
    assert backend.prove(get_example_options()) == previous, "a refused batch changed the resident witness"
    _assert_batch(led.apply(_transfers(w, 4, 8)), w, 4, 8)
    assert np.array_equal(led.root(), w.final_root)
    led.close()


def test_misuse_is_a_negative_status(backend):
    from certificate_stark_amd import CstarkError
    from certificate_stark_amd.backend import Backend
    from certificate_stark_amd.prover import Ledger
    w = LC.generated((2, 3, 2))
    led, indices = _ledger(backend, w)
    lib, none = backend.lib, None
    at, reason = C.c_int32(-1), C.c_int32(0)
    s, r, d, rx, ss = (np.ascontiguousarray(a) for a in _transfers(w))
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    args = [a.ctypes.data_as(u64p) for a in (s, r, d, rx)] + [ss.ctypes.data_as(u8p)]
    assert lib.cstark_ledger_apply(backend.ctx, led._led, C.c_uint32(0), *args, none, C.byref(at), C.byref(reason)) == -1     # n_tx == 0
    assert lib.cstark_ledger_apply(backend.ctx, led._led, C.c_uint32(2), none, *args[1:], none, C.byref(at), C.byref(reason)) == -1   # null array
    assert lib.cstark_ledger_apply(backend.ctx, led._led, C.c_uint32(2), *args, none, none, C.byref(reason)) == -1            # null refused_at
    assert lib.cstark_ledger_apply(backend.ctx, none, C.c_uint32(2), *args, none, C.byref(at), C.byref(reason)) == -1         # null ledger
    assert lib.cstark_ledger_root(backend.ctx, led._led, none) == -1
    assert lib.cstark_ledger_set_accounts(backend.ctx, led._led, C.c_uint32(0), args[0], args[0]) == -1                      # count == 0
    other = Backend()
    assert lib.cstark_ledger_root(other.ctx, led._led, np.zeros(7, np.uint64).ctypes.data_as(u64p)) == -1                    # another context
    assert lib.cstark_ledger_apply(other.ctx, led._led, C.c_uint32(2), *args, none, C.byref(at), C.byref(reason)) == -1
    other.close()
    with pytest.raises(CstarkError):
        led.set_accounts(np.array([1, 1], np.uint64), np.ones((2, 14), np.uint64))      # an index twice
    with pytest.raises(CstarkError):
        led.set_accounts(np.array([8], np.uint64), np.ones((1, 14), np.uint64))         # index >= 2^depth
    with pytest.raises(CstarkError):
        Ledger(4, backend)                                                               # not a depth the witness upload accepts
    # none of it changed the ledger: the batch still gives the reference arrays
    assert np.array_equal(led.root(), w.initial_roots[0])
    _assert_batch(led.apply(_transfers(w)), w)
    led.close()
