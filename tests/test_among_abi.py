"""The candidate-set entry points (include/fme_among.h) at the ABI: libfme_amd.so exports them, the
three constants are what the header says, the new status bit is a bit of its own, and the argument
checks refuse what they must before anything touches a device.  The entry points themselves run in
tests/test_gpu_among.py."""
import os
import re
import subprocess

from conftest import ROOT
from nnfme import abi, among, direct, predictor, runtime
from test_abi import header_functions


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_the_among_entry_points():
    names = sorted(set(re.findall(r"\b(fme_[a-z0-9_]+)\s*\(", _header("fme_among.h"))))
    assert names == sorted(among.AMONG_SYMBOLS) and len(names) == 9
    lib = runtime.load_library()
    for n in names:
        assert hasattr(lib, n), n
    # additional exports: the other headers and the counted ABI are as they were
    assert not set(names) & set(runtime.ABI_SYMBOLS) and not set(names) & set(header_functions())
    assert not set(names) & set(direct.DIRECT_SYMBOLS) and not set(names) & set(predictor.EXTERN_SYMBOLS)
    assert lib.fme_abi_version() == runtime.ABI_VERSION
    among.bind(lib)
    assert lib._fme_among_bound and among.bind(lib) is lib


def test_constants_of_the_header(tmp_path):
    """The three constants as a C compiler sees include/fme_among.h, against the mirror's."""
    src = tmp_path / "k.c"
    src.write_text('#include <stdio.h>\n#include "fme_among.h"\nint main(void) {\n'
                   '  printf("%d %u %u", (int)FME_AMONG_MAX, (unsigned)FME_AMONG_EMPTY, (unsigned)FME_RES_NN_AMONG);\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "k")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [8, 0xFF, 0x10] == [among.AMONG_MAX, among.AMONG_EMPTY, among.RES_NN_AMONG]
    assert among.AMONG_STATUS == 0x04 | 0x08 | 0x10 and among.TOPK_STATUS == 0x04 | 0x10


def test_status_bit_collides_with_no_other():
    bits = {}
    for h in ("fme.h", "fme_direct.h", "fme_extern.h", "fme_among.h"):
        for name, val in re.findall(r"#define\s+(FME_RES_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", _header(h)):
            bits[name] = int(val, 16)
    assert set(bits) == {"FME_RES_NN_STALE", "FME_RES_NN_UNINIT", "FME_RES_REJECTED", "FME_RES_NN_DIRECT",
                         "FME_RES_NN_EXTERN", "FME_RES_NN_AMONG"}
    assert bits["FME_RES_NN_AMONG"] == among.RES_NN_AMONG == 0x10
    vals = list(bits.values())
    assert all(v and v & (v - 1) == 0 for v in vals) and len(set(vals)) == len(vals)   # single, distinct bits
    assert bits["FME_RES_NN_AMONG"] < 1 << 16                                          # fits fme_result.status


def test_null_k_and_negative_arguments_rejected():
    """No device is needed: a null context, null arrays, k = 0 and 9 and n < 0 are refused first."""
    lib = among.bind(runtime.load_library())
    one = 64 * b"\0"
    for f in (lib.fme_refine_among, lib.fme_refine_among_device, lib.fme_refine_among_mv_device):
        assert f(None, None, None, None, 8, None, None, 1, None) == abi.E_INVALID
        assert b"bad argument" in lib.fme_last_error()
        assert f(None, one, None, one, 8, one, None, 1, None) == abi.E_INVALID    # no context
        assert f(None, None, None, None, 8, None, None, 0, None) == abi.E_INVALID # n == 0 still needs one
        assert f(None, one, one, one, 8, one, one, -1, None) == abi.E_INVALID
        for k in (0, 9, -1):
            assert f(None, one, one, one, k, one, one, 1, None) == abi.E_INVALID
    assert lib.fme_nn_rank_device(None, None, None, 8, 1, None) == abi.E_INVALID
    assert lib.fme_nn_rank_device(None, one, one, 8, -1, None) == abi.E_INVALID
    for k in (0, 9):
        assert lib.fme_nn_rank_device(None, one, one, k, 1, None) == abi.E_INVALID
    for f in (lib.fme_refine_topk, lib.fme_refine_topk_device, lib.fme_refine_topk_mv_device):
        assert f(None, None, None, 4, None, None, 1, None) == abi.E_INVALID
        assert b"bad argument" in lib.fme_last_error()
        assert f(None, one, one, 4, None, None, -1, None) == abi.E_INVALID
        for k in (0, 9):
            assert f(None, one, one, k, None, None, 1, None) == abi.E_INVALID
    assert lib.fme_refine_among_status(None) == abi.E_INVALID
    assert lib.fme_among_last_ms(None, None) == abi.E_INVALID


def test_request_checks_of_the_entry_points(tmp_path):
    """The checks as the entry points call them (csrc/fme_among_host.h): n == 0 is accepted, k outside
    1..8, a missing array or n < 0 is FME_E_INVALID, bound NN rows FME_E_STATE; the ranking and the top-K
    batch need nn_mode 1 with weights (nn_mode 0: FME_E_STATE, nn_mode 2: FME_E_UNSUPPORTED)."""
    src = tmp_path / "req.cpp"
    src.write_text('#include <cstdio>\n#include "fme_among_host.h"\nint main() { int c = 0, j = 0, l = 0, o = 0, r = 0;\n'
                   'std::printf("%d %d %d %d %d %d %d %d ", fme::among_request(&c, &j, &l, 8, &o, 3, false),\n'
                   'fme::among_request(&c, nullptr, nullptr, 1, nullptr, 0, false), fme::among_request(&c, &j, nullptr, 8, &o, 3, false),\n'
                   'fme::among_request(&c, &j, &l, 8, &o, -2, false), fme::among_request(nullptr, &j, &l, 8, &o, 3, false),\n'
                   'fme::among_request(&c, &j, &l, 8, &o, 3, true), fme::among_request(&c, &j, &l, 0, &o, 3, false),\n'
                   'fme::among_request(&c, &j, &l, 9, &o, 3, false));\n'
                   'std::printf("%d %d %d %d %d ", fme::among_rank_request(&c, &r, &l, 3, 5, 1, true),\n'
                   'fme::among_rank_request(&c, &r, &l, 3, 0, 1, true), fme::among_rank_request(&c, &r, &l, 3, 5, 0, false),\n'
                   'fme::among_rank_request(&c, &r, &l, 3, 5, 2, false), fme::among_rank_request(&c, &r, &l, 3, 5, 1, false));\n'
                   'std::printf("%d %d %d %d %d", fme::among_topk_request(&c, &j, &o, 4, 5, false, 1, true),\n'
                   'fme::among_topk_request(&c, &j, &o, 4, 0, false, 1, true), fme::among_topk_request(&c, &j, &o, 4, 5, true, 1, true),\n'
                   'fme::among_topk_request(&c, &j, &o, 4, 5, false, 0, false), fme::among_topk_request(&c, &j, &o, 4, 5, false, 2, false));\n'
                   'return 0; }\n')
    exe = str(tmp_path / "req")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc"), str(src), "-o", exe],
                   check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [0, 1, abi.E_INVALID, abi.E_INVALID, abi.E_INVALID, abi.E_STATE, abi.E_INVALID, abi.E_INVALID,
                   0, 1, abi.E_STATE, abi.E_UNSUPPORTED, abi.E_STATE,
                   0, 1, abi.E_STATE, abi.E_STATE, abi.E_UNSUPPORTED]
