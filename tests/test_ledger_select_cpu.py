"""The host half of cstark_ledger_select (csrc/ledger_plan.h) on the CPU: tests/cpp/ledger_select_check.cpp, a stand-alone program built
with AddressSanitizer and UBSan and run directly, prepares every pool of select_cases.py, runs the resumable walk at chunk sizes 1, 3
and n on steered signature verdicts, applies the selection with the host `merge` and prints statuses, selection, messages and root;
they are compared with tests/select_model.py.  The verdicts are steered as real signatures behave: a candidate's signature is valid
iff it is uncorrupted and the message it meets is the one it was signed for in the skeleton."""
import functools
import os
import subprocess

import numpy as np
import pytest

import ledger_model as LM
import select_cases as SC
import select_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, depth) for name in SC.CASES for depth in SC.DEPTHS]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ledger_select") / "ledger_select_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_select_check.cpp")])
    return exe


@functools.lru_cache(maxsize=None)
def fake_keys():
    """reduced words in place of public keys: the host walk never looks at a key"""
    k = np.array([[((12 * a + j + 1) * 0x9E3779B97F4A7C15) % SC.P for j in range(12)] for a in range(SC.N_ACC)], np.uint64)
    k.flags.writeable = False
    return k


def model_of(pool, keys):
    m = LM.LedgerModel(pool.depth)
    m.set_accounts(pool.indices(), pool.values(keys))
    return m


def steered(pool):
    """-> (model, expected Result, sig_rx, verdict bytes, the candidates the model asked sig_ok about): the model's answer under
    signatures that behave as real ones do"""
    clean = model_of(pool, fake_keys())
    s, r, d, _ = pool.skeleton_batch()
    signed = SM.select(clean, s, r, d, len(s), sig_ok=lambda t, m: True).messages
    assert len(signed) == len(s), "the skeleton is appliable"
    keys = fake_keys().copy()
    if pool.off_curve is not None:
        keys[pool.off_curve, 3] = (int(keys[pool.off_curve, 3]) + 1) % SC.P
    model = model_of(pool, keys)
    rx, _ = pool.signatures(np.zeros((len(s), 6), np.uint64), np.zeros((len(s), 32), np.uint8))
    verdicts = np.ones(pool.n, np.uint8)      # a candidate nobody asks about: MISMATCH, so that asking shows
    asked = set()

    def sig_ok(t, m):
        asked.add(t)
        e = pool.entries[t]
        off = pool.off_curve is not None and e.s == pool.leaf(pool.off_curve)
        verdicts[t] = 3 if e.sig == "s_bit255" else 2 if off else 0 if e.src is not None and e.sig == "ok" and np.array_equal(m, signed[e.src]) else 1
        return verdicts[t] == 0

    s, r, d = pool.batch()
    expected = SM.select(model, s, r, d, pool.want, sig_ok=sig_ok, sig_rx=rx, pow2=pool.pow2, known=pool.known() if pool.partial else None)
    return model, expected, rx, verdicts, asked


def run(checker, path, pool, keys, rx, verdicts, check=True):
    s, r, d = pool.batch()
    known = pool.known() if pool.partial else []
    head = np.array([pool.depth, SC.N_ACC, pool.n, pool.want, (1 if check else 0) | (2 if pool.pow2 else 0), len(known)], np.uint64)
    with open(path, "wb") as f:
        for a in (head, pool.indices(), pool.values(keys), np.array(known, np.uint64), s, r, d, rx):
            f.write(np.ascontiguousarray(a, "<u8").tobytes())
        f.write(np.ascontiguousarray(verdicts, np.uint8).tobytes())
    out = subprocess.run([checker, path], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.endswith("ok\n"), out.stdout[-4000:] + out.stderr[-4000:]
    got = {"message": {}}
    for line in out.stdout.splitlines():
        words = line.split()
        if words[0] == "message":
            got["message"][int(words[1])] = np.array([int(w, 16) for w in words[2:]], np.uint64)
        elif words[0] == "root":
            got["root"] = np.array([int(w, 16) for w in words[1:]], np.uint64)
        elif words[0] in ("status", "selected"):
            got[words[0]] = [int(w) for w in words[1:]]
        elif words[0] == "checked":
            got["checked"], got["passes"] = [int(w) for w in words[1:4]], [int(w) for w in words[5:8]]
    return got


@pytest.mark.parametrize("name,depth", CASES, ids=["%s-d%d" % c for c in CASES])
def test_walk_and_plan_give_the_models_selection(checker, name, depth, tmp_path):
    pool = SC.CASES[name](depth)
    model, expected, rx, verdicts, asked = steered(pool)
    SC.check_landmarks(name, expected.status)
    keys = model.accounts(pool.indices())[:, :12]
    got = run(checker, str(tmp_path / "case.bin"), pool, keys, rx, verdicts)
    assert got["status"] == [int(v) for v in expected.status]
    assert got["selected"] == [int(t) for t in expected.selected]
    # the messages of the candidates whose status came from a verdict: APPLIED, or SIGNATURE with a reduced sig_rx
    with_verdict = [t for t in range(pool.n) if expected.status[t] == SM.APPLIED or (expected.status[t] == SM.SIGNATURE and pool.entries[t].sig != "rx_ge_p")]
    assert sorted(got["message"]) == with_verdict
    for t in with_verdict:
        assert np.array_equal(got["message"][t], expected.messages[t]), t
    # the root the applied selection leaves
    if len(expected.selected):
        w = model.apply(*expected.transfers(pool.batch()))
        assert not isinstance(w, tuple), "the model refuses the selection at %r" % (w,)
    assert np.array_equal(got["root"], model.root())
    # one candidate per pass checks exactly the signatures whose verdict the walk needs (it walks with `want` as given: the cut to a
    # power of two comes after it)
    assert got["checked"][0] == len(asked) == got["passes"][0] and set(with_verdict) <= asked
    assert got["passes"][2] <= got["passes"][1] <= got["passes"][0]


@pytest.mark.parametrize("name", ["all_valid", "flipped_s", "cascade", "overdraft", "pow2_11_of_16"])
def test_without_the_signature_test_no_verdict_is_asked_for(checker, name, tmp_path):
    pool = SC.CASES[name](3)
    model = model_of(pool, fake_keys())
    s, r, d = pool.batch()
    expected = SM.select(model, s, r, d, pool.want, pow2=pool.pow2)
    got = run(checker, str(tmp_path / "case.bin"), pool, fake_keys(), np.zeros((pool.n, 6), np.uint64), np.ones(pool.n, np.uint8), check=False)
    assert got["status"] == [int(v) for v in expected.status] and got["selected"] == [int(t) for t in expected.selected]
    assert got["checked"] == [0, 0, 0] and got["passes"] == [0, 0, 0] and not got["message"]
    assert SM.SIGNATURE not in got["status"]


def test_the_library_exports_select_and_the_header_states_the_new_values():
    import re
    from certificate_stark_amd import _lib
    assert hasattr(_lib.load(), "cstark_ledger_select")
    header = open(os.path.join(ROOT, "include", "cstark.h")).read()
    values = dict(re.findall(r"\b(CSTARK_LEDGER_[A-Z_]+) = (\d+)", header))
    assert values["CSTARK_LEDGER_HELD"] == "8" and values["CSTARK_LEDGER_NOT_REACHED"] == "9"
    assert [values["CSTARK_LEDGER_" + k] for k in ("APPLIED", "INDEX_RANGE", "SELF_TRANSFER", "ABSENT", "BALANCE", "SIGNATURE", "UNKNOWN", "KEY")] == list("01234567")
    flags = dict(re.findall(r"#define (CSTARK_SELECT_[A-Z0-9_]+) (\d+)u", header))
    assert flags == {"CSTARK_SELECT_CHECK_SIGNATURES": "1", "CSTARK_SELECT_POW2": "2", "CSTARK_SELECT_APPLY": "4"}
    from certificate_stark_amd.prover import Ledger
    assert (Ledger.HELD, Ledger.NOT_REACHED) == (8, 9) == (SM.HELD, SM.NOT_REACHED)
