"""The arithmetic of the model stages (csrc/vag_stage_plan.h) under the host sanitizers: tests/stage_plan_check.cpp is built with the
system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer linked in, and run as a child process.  The program holds every
decision -- the capacities of a planned-ahead call and whether a call may be planned ahead, the verdict at its end and the growth of
the lattice margin, the dynamics family of every combination of reverse shock, dynamics class, spreading, magnetar and
VAG_DYN_GENERAL, the refill threshold and its three hooks, the rows per wavefront of the pair solver, the byte layout of d_dynrec
and the grouping of a batch by flags -- to literals worked out by hand from the functions the arithmetic was moved out of, every
threshold at its value and on each side; here: exit status 0 and one "ok" line per case.  No device, no library, nothing loaded
into this process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
CASES = ["capacities", "verdict", "margin", "dynamics family", "refill", "pair_rows_per_wave", "d_dynrec layout", "grouping"]
STATIC = ["-static-libasan", "-static-libubsan"]  # g++ links its sanitizer runtimes dynamically unless told; clang++ statically, and knows no such flag


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.fixture(scope="module")
def compile_cmd(tmp_path_factory):
    """[compiler, flags...] that link the sanitizer runtimes into a binary, or a skip when the compiler cannot link a sanitized
    hello-world at all."""
    cxx = os.environ.get("CXX", "c++")
    d = tmp_path_factory.mktemp("hello")
    (d / "hello.cpp").write_text('#include <cstdio>\nint main() { std::puts("hello"); return 0; }\n')
    out = ""
    for extra in (STATIC, []):
        try:
            built = run([cxx] + FLAGS + extra + [str(d / "hello.cpp"), "-o", str(d / "hello")])
        except OSError as e:
            pytest.skip(f"{cxx} cannot be run: {e}")
        if built.returncode == 0:
            return [cxx] + FLAGS + extra
        out = built.stdout
    pytest.skip(f"{cxx} cannot link a hello-world with {FLAGS[3]}: {out[-300:]}")


def test_the_stage_arithmetic_holds_its_thresholds_under_asan_and_ubsan(compile_cmd, tmp_path):
    exe = tmp_path / "stage_plan_check"
    built = run(compile_cmd + ["-Wall", "-Wextra", os.path.join(ROOT, "tests", "stage_plan_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = run([str(exe)])
    assert ran.returncode == 0, ran.stdout
    lines = ran.stdout.splitlines()
    for case in CASES:
        assert f"ok {case}" in lines, (case, ran.stdout)
    assert not any(ln.startswith("FAIL") for ln in lines), ran.stdout
