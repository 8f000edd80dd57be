"""The NN-direct entry points (include/fme_direct.h) at the ABI: libfme_amd.so exports them, the new
status bit is a bit of its own, and the argument checks refuse what they must before anything touches
a device.  The checks that need a context (n == 0, nn_mode 0) run the entry points' own check
function (csrc/fme_direct_host.h direct_request) in a small program here, and the entry points
themselves in tests/test_gpu_direct.py."""
import os
import re
import subprocess

from conftest import ROOT
from nnfme import abi, direct, runtime
from test_abi import header_functions


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_the_direct_entry_points():
    names = sorted(set(re.findall(r"\b(fme_[a-z0-9_]+)\s*\(", _header("fme_direct.h"))))
    assert names == sorted(direct.DIRECT_SYMBOLS) and len(names) == 4
    lib = runtime.load_library()
    for n in names:
        assert hasattr(lib, n), n
    # additional exports: fme.h and the counted ABI are as they were
    assert not set(names) & set(runtime.ABI_SYMBOLS) and not set(names) & set(header_functions())
    assert lib.fme_abi_version() == runtime.ABI_VERSION
    direct.bind(lib)
    assert lib._fme_direct_bound and direct.bind(lib) is lib


def test_status_bit_collides_with_no_other():
    bits = {}
    for h in ("fme.h", "fme_direct.h"):
        for name, val in re.findall(r"#define\s+(FME_RES_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", _header(h)):
            bits[name] = int(val, 16)
    assert set(bits) == {"FME_RES_NN_STALE", "FME_RES_NN_UNINIT", "FME_RES_REJECTED", "FME_RES_NN_DIRECT"}
    assert bits["FME_RES_NN_DIRECT"] == direct.RES_NN_DIRECT == 0x04
    vals = list(bits.values())
    assert all(v and v & (v - 1) == 0 for v in vals) and len(set(vals)) == len(vals)   # single, distinct bits
    assert bits["FME_RES_NN_DIRECT"] < 1 << 16                                         # fits fme_result.status
    assert (bits["FME_RES_NN_STALE"], bits["FME_RES_NN_UNINIT"], bits["FME_RES_REJECTED"]) == (
        abi.RES_NN_STALE, abi.RES_NN_UNINIT, abi.RES_REJECTED)


def test_null_and_negative_arguments_rejected():
    lib = direct.bind(runtime.load_library())
    one = (abi.JOB_DTYPE.itemsize + abi.RESULT_DTYPE.itemsize) * b"\0"
    for f in (lib.fme_refine_direct, lib.fme_refine_direct_device, lib.fme_refine_direct_mv_device):
        assert f(None, None, None, 1, None) == abi.E_INVALID
        assert b"bad argument" in lib.fme_last_error()
        assert f(None, one, one, 1, None) == abi.E_INVALID     # no context
        assert f(None, None, None, 0, None) == abi.E_INVALID   # n == 0 still needs one
        assert f(None, one, one, -1, None) == abi.E_INVALID
    assert lib.fme_refine_direct_last_ms(None, None) == abi.E_INVALID


def test_request_check_of_the_entry_points(tmp_path):
    """direct_request as the entry points call it: n == 0 is accepted (they return 0), nn_mode 0 is
    FME_E_STATE, a bad argument FME_E_INVALID."""
    src = tmp_path / "req.cpp"
    src.write_text('#include <cstdio>\n#include "fme_direct_host.h"\nint main() { int c = 0, j = 0, o = 0;\n'
                   'std::printf("%d %d %d %d %d %d", fme::direct_request(&c, &j, &o, 3, 1), fme::direct_request(&c, &j, &o, 0, 1),\n'
                   'fme::direct_request(&c, &j, &o, 3, 0), fme::direct_request(&c, nullptr, &o, 3, 2),\n'
                   'fme::direct_request(&c, &j, &o, -2, 1), fme::direct_request(nullptr, &j, &o, 3, 1)); return 0; }\n')
    exe = str(tmp_path / "req")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc"), str(src), "-o", exe],
                   check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [0, 1, abi.E_STATE, abi.E_INVALID, abi.E_INVALID, abi.E_INVALID]
