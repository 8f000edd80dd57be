"""The host arithmetic of fme_skip_estimate (csrc/fme_skip_host.h) on a CPU: the chroma weighting
with its truncation, the CU's distortion in UInt arithmetic, calcRdCost, the requests' expansion
into SSE tasks, the masked strict minimum and the "none" result, against naive transcriptions of
TComRdCost.cpp / TEncSearch.cpp / TEncCu.cpp in tests/cpp/test_skip_host.cpp.  The program is built
stand-alone with AddressSanitizer + UndefinedBehaviorSanitizer (no Python in the sanitized
process) and with the library's -ffp-contract=off."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_skip_host.cpp")
INC = os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    raise AssertionError("no C++ compiler found")


def test_skip_host_against_naive_definitions(tmp_path):
    exe = str(tmp_path / "test_skip_host")
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
    m = re.search(r"skip host ok: (\d+) cases", out)
    assert m, out[-2000:]
    # 10 + 4000 weighting cases, 1 wrap-around, 20000 requests, 12 validity cases
    assert int(m.group(1)) == 10 + 4000 + 1 + 20000 + 12, out[-2000:]
