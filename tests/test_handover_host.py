"""The hand-over between overlapped batches (csrc/fme_overlap_host.h) on a CPU: over sequences of
12 batches on one, two and three streams in rotation and on streams drawn at random from three,
plain and with a featured batch, an abandoned batch or an integer search at each position, every
pair of batches is checked from the plans alone: what they share (a slot's perm / cls and records,
a ring entry, a counter block) is reused only behind a wait or in stream order, every block is
zeroed between uses, a serialised batch runs beside nothing and the tails run in batch order
(tests/cpp/test_handover_host.cpp).  The program is built stand-alone with AddressSanitizer +
UndefinedBehaviorSanitizer (no Python in the sanitized process)."""
import os
import re
import subprocess

from conftest import ROOT
from test_merge_host import _compiler

SRC = os.path.join(ROOT, "tests", "cpp", "test_handover_host.cpp")
INC = os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc")


def test_handover_planner(tmp_path):
    exe = str(tmp_path / "test_handover_host")
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
    m = re.search(r"handover host ok: (\d+) cases", out)
    assert m and int(m.group(1)) > 0, out[-2000:]
