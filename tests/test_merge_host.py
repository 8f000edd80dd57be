"""The host arithmetic of fme_merge_estimate (csrc/fme_merge_host.h) on a CPU: the merge-index bits,
getCost, the bi-pred restriction, the requests' expansion into prediction-error tasks, the strict
minima and the uiMRGCost < uiMECost choice, against naive transcriptions of TEncSearch.cpp in
tests/cpp/test_merge_host.cpp.  The program is built stand-alone with AddressSanitizer +
UndefinedBehaviorSanitizer (no Python in the sanitized process)."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_merge_host.cpp")
INC = os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    raise AssertionError("no C++ compiler found")


def test_shape_list_matches_synth():
    """The program's PU shapes are the package's ALL_PU_SIZES."""
    from nnfme import synth
    text = open(SRC).read()
    body = text[text.index("kShapes[][2] = {"):text.index("};", text.index("kShapes[][2] = {"))]
    got = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", body)]
    assert sorted(got) == sorted(tuple(s) for s in synth.ALL_PU_SIZES) and len(got) == 24


def test_merge_host_against_naive_definitions(tmp_path):
    exe = str(tmp_path / "test_merge_host")
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
    m = re.search(r"merge host ok: (\d+) cases", out)
    assert m, out[-2000:]
    # 25 bit counts, 4000 costs, 4 x 8 x 8 = 256 restriction cases, 20000 requests, 10 validity cases
    assert int(m.group(1)) == 25 + 4000 + 256 + 20000 + 10, out[-2000:]
