"""The predInterSearch producers' host arithmetic (csrc/fme_pi_host.h) on a CPU: the bit counts, the
search-job builder, the AMVP choice, xCheckBestMVP and the m_integerMv2Nx2N dependency levels with
their launch order, against naive definitions in tests/cpp/test_pi_host.cpp.  The program is built
stand-alone with AddressSanitizer + UndefinedBehaviorSanitizer (no Python in the sanitized process)."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_pi_host.cpp")
INC = os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    raise AssertionError("no C++ compiler found")


def test_shape_list_matches_synth():
    """The program's copy of ALL_PU_SIZES is the package's list."""
    from nnfme import synth
    text = open(SRC).read()
    body = text[text.index("kShapes[][2] = {"):text.index("};", text.index("kShapes[][2] = {"))]
    got = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", body)]
    assert got == [tuple(s) for s in synth.ALL_PU_SIZES]


def test_pi_host_against_naive_definitions(tmp_path):
    exe = str(tmp_path / "test_pi_host")
    cxx = _compiler()
    # the sanitizer runtimes linked statically (clang's default), so the program needs no preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, *static, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
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
    m = re.search(r"pi host ok: (\d+) cases", out)
    assert m, out[-2000:]
    # 65547 bit counts, 2 x 24 shapes x 5 places x 3 ranges x 6 = 4320 search jobs, 203 streams, 4000 MVP checks
    assert int(m.group(1)) == 65547 + 4320 + 203 + 4000, out[-2000:]
