"""The checkpoints of csrc/ledger_plan.h and plan_audit on the CPU: tests/cpp/ledger_checkpoint_check.cpp (a stand-alone program, built
with AddressSanitizer and UBSan and run directly) runs scripted interleavings of set_accounts, apply, checkpoint, revert, release and
open-at on a host pool with the host `merge`, against plain copies of (index, pool) taken at checkpoint time, and audits every state."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ledger_checkpoint") / "ledger_checkpoint_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ledger_checkpoint_check.cpp")])
    return exe


def test_checkpoints_keep_every_state_and_every_state_audits_clean(checker):
    out = subprocess.run([checker], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert re.findall(r"^ok: depth (\d+), \d+ states opened and audited", out.stdout, flags=re.M) == ["1", "3", "15", "31"], out.stdout


def test_the_debug_header_is_served_by_the_debug_library_only():
    """include/cstark_debug_ledger.h: its one name is exported by libcstark_debug.so and not by the product library"""
    from certificate_stark_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cstark_debug_ledger.h")).read()
    names = set(re.findall(r"\b(cstark_debug_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert names == {"cstark_debug_ledger_xor_word"}
    lib, dbg = L.load(), L.load_debug()
    assert all(hasattr(dbg, n) and not hasattr(lib, n) for n in names)
    for n in ("checkpoint", "revert", "release", "root_at", "open_accounts_at", "audit"):
        assert hasattr(lib, "cstark_ledger_" + n), n
