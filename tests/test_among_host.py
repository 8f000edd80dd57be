"""The host arithmetic of candidate-set refinement (csrc/fme_among_host.h) on a CPU: the slot and list
checks with every refusal, the pick rule with ties, empties and duplicates, the k-best insertion with
equal values, the host form's batch check and the entry points' argument checks, against naive
definitions in tests/cpp/test_among_host.cpp.  The program is built stand-alone with AddressSanitizer +
UndefinedBehaviorSanitizer (no Python in the sanitized process)."""
import os
import re
import subprocess

from conftest import ROOT
from test_surface_host import _compiler

SRC = os.path.join(ROOT, "tests", "cpp", "test_among_host.cpp")
INC = os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc")


def test_among_host_against_naive_definitions(tmp_path):
    exe = str(tmp_path / "test_among_host")
    cxx = _compiler()
    # the sanitizer runtimes linked statically (clang's default), so the program needs no preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, *static, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                            "-I", INC, "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:halt_on_error=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = run.stdout + run.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert run.returncode == 0, out[-4000:]
    m = re.search(r"among host ok: (\d+) cases", out)
    assert m, out[-2000:]
    # the constants, 256 slot values, 24 + 4000 lists, 2 + 4000 picks, 3000 + 2 insertions, 7 batch checks, 31 requests
    assert int(m.group(1)) == 1 + 256 + 4024 + 4002 + 3002 + 7 + 31, out[-2000:]
