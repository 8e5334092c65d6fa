"""The host side of a likelihood request (csrc/vag_fit_request.h: the scans, the miss halves of the four blocks hashed in place,
FitRequest, fit_request_prepare) under the host
sanitizers: tests/fit_request_check.cpp is built with the system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer linked
in, and run as a child process.  The program compares every layout offset and every staged double and int32 with values written down
from the documented layouts, on heap inputs of exactly the advertised lengths; here: exit status 0 and one "ok" line per case.  No
device, no library, nothing loaded into this process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SCANS = ("lim", "noise", "tmpl", "counts", "index", "fold", "cov")
BLOCKS = ("fit", "sky", "pol", "vis")  # hashed in place: a scan, and a miss half of row checks and a fill
CASES = [f"{s}_scan layout" for s in SCANS] + [f"{b} block layout" for b in BLOCKS] + ["block hashes", "scan keys"] + \
        ["fit_request_prepare empty blocks", "fit_request_prepare full request"] + \
        [f"{s}_scan refusal" for s in SCANS] + [f"{b} block refusals" for b in BLOCKS] + ["block columns", "pass list"]
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


def test_the_scans_lay_out_what_the_layouts_document_under_asan_and_ubsan(compile_cmd, tmp_path):
    exe = tmp_path / "fit_request_check"
    built = run(compile_cmd + [os.path.join(ROOT, "tests", "fit_request_check.cpp"), "-o", str(exe)])
    assert built.returncode == 0, built.stdout
    ran = run([str(exe)])
    assert ran.returncode == 0, ran.stdout
    lines = ran.stdout.splitlines()
    for case in CASES:
        assert f"ok {case}" in lines, (case, ran.stdout)
    assert not any(ln.startswith("FAIL") for ln in lines), ran.stdout
