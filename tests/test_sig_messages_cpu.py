"""The message builder of csrc/ledger_plan.h on the CPU: tests/cpp/ledger_messages_check.cpp (a stand-alone program, built with
AddressSanitizer and UBSan and run directly) asks plan_apply for the messages a batch's transfers sign, compares them with the walk of
sig_cases.tx_messages, and verifies every signature against its message with the host arithmetic of hostgadgets.h."""
import subprocess

import numpy as np
import pytest

import ledger_cases as LC
import sig_cases as SC


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return SC.build_messages_checker(tmp_path_factory.mktemp("ledger_messages"))


def _run(checker, path):
    out = subprocess.run([checker, path], capture_output=True, text=True)
    return out.returncode, out.stdout + out.stderr


@pytest.mark.parametrize("case", [(1, 3, 1), (16, 3, 3), (32, 3, 9), (4, 31, 6)], ids=LC.case_id)
def test_plan_builds_the_signed_messages(checker, case, tmp_path):
    path = str(tmp_path / "case.bin")
    SC.write_messages_case(path, LC.generated(case))
    rc, text = _run(checker, path)
    n = case[0]
    assert rc == 0 and "refused_at -1, %d messages, %d signatures valid on the host" % (n, n) in text, text


def test_a_refused_batch_gives_the_messages_before_the_refusal(checker, oracle, tmp_path):
    w = LC.generated((16, 3, 3))
    s, r, d, rx, ss = (a.copy() for a in SC.transfers(w))
    d[9] = oracle.to_mont(np.array([SC.P - 1], np.uint64))[0]
    path = str(tmp_path / "case.bin")
    SC.write_messages_case(path, w, (s, r, d, rx, ss), SC.tx_messages(w, 9), (9, 4))
    rc, text = _run(checker, path)
    assert rc == 0 and "refused_at 9, 9 messages, 9 signatures valid on the host" in text, text


def test_checker_is_live(checker, tmp_path):
    """a message built from the state before the BATCH, or a flipped scalar bit, does not pass"""
    w = LC.generated((16, 3, 3))
    stale = SC.tx_messages(w).copy()
    moved = SC.nonce_moved(w)[0]
    first = int(np.flatnonzero(w.s_indices == w.s_indices[moved])[0])
    stale[moved, 25] = w.s_old_values[first, 13]
    path = str(tmp_path / "case.bin")
    SC.write_messages_case(path, w, messages=stale)
    rc, text = _run(checker, path)
    assert rc == 1 and "messages[%d][25] differs" % moved in text, text
    SC.write_messages_case(path, w, SC.flipped(w, 7))
    rc, text = _run(checker, path)
    assert rc == 0 and "16 messages, 15 signatures valid on the host" in text, text
