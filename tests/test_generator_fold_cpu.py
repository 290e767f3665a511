"""csrc/generator_fold.h on the CPU: the fold table of the generator addition against the mixed addition it replaces."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_fold_equals_the_mixed_addition(tmp_path):
    """csrc/generator_fold.h alone (g++, host code only): the quadratic forms derived from the mixed-addition formula give the same 18
    components as the formula itself with G, and the three folded functionals equal the sums over the outputs for random
    coefficients -- on 1200 random triples of F_p6 (off the curve) and on triples of 0, 1 and p - 1
    (tests/cpp/generator_fold_check.cpp)."""
    exe = str(tmp_path / "generator_fold_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "generator_fold_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: 1829 triples checked"), out.stdout + out.stderr
