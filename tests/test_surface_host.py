"""The host arithmetic of the cost surface (csrc/fme_surface_host.h) on a CPU: the index <-> offset
maps against FME_SURF_INDEX and the NN class map, the 24 PU shapes, the replay of
xPatternRefinement's two stages in the H-then-Q visiting orders, the pick and probe rule and the
regret record, against naive transcriptions in tests/cpp/test_surface_host.cpp.  The program is
built stand-alone with AddressSanitizer + UndefinedBehaviorSanitizer (no Python in the sanitized
process)."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_surface_host.cpp")
INC = os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    raise AssertionError("no C++ compiler found")


def test_surface_host_against_naive_definitions(tmp_path):
    exe = str(tmp_path / "test_surface_host")
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
    m = re.search(r"surface host ok: (\d+) cases", out)
    assert m, out[-2000:]
    # 49 + 81 + 9 map cases, 65536 shapes + 256 probes, 20000 surfaces, 1 constructed tie
    assert int(m.group(1)) == 49 + 81 + 9 + 65536 + 256 + 20000 + 1, out[-2000:]
