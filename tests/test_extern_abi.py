"""The external-predictor entry points (include/fme_extern.h) at the ABI: libfme_amd.so exports them,
fme_nn_row is the 64-byte layout the header declares, the new status bit is a bit of its own, and the
argument checks refuse what they must before anything touches a device.  The checks that need a
context (n == 0, bound rows) run the entry points' own check functions (csrc/fme_extern_host.h) in a
small program here, and the entry points themselves in tests/test_gpu_extern.py."""
import os
import re
import subprocess

from conftest import ROOT
from nnfme import abi, direct, predictor, runtime
from test_abi import header_functions


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_the_extern_entry_points():
    names = sorted(set(re.findall(r"\b(fme_[a-z0-9_]+)\s*\(", _header("fme_extern.h"))))
    assert names == sorted(predictor.EXTERN_SYMBOLS) and len(names) == 7
    lib = runtime.load_library()
    for n in names:
        assert hasattr(lib, n), n
    # additional exports: fme.h, fme_direct.h and the counted ABI are as they were
    assert not set(names) & set(runtime.ABI_SYMBOLS) and not set(names) & set(header_functions())
    assert not set(names) & set(direct.DIRECT_SYMBOLS)
    assert lib.fme_abi_version() == runtime.ABI_VERSION
    predictor.bind(lib)
    assert lib._fme_extern_bound and predictor.bind(lib) is lib


def test_status_bit_collides_with_no_other():
    bits = {}
    for h in ("fme.h", "fme_direct.h", "fme_extern.h"):
        for name, val in re.findall(r"#define\s+(FME_RES_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", _header(h)):
            bits[name] = int(val, 16)
    assert set(bits) == {"FME_RES_NN_STALE", "FME_RES_NN_UNINIT", "FME_RES_REJECTED", "FME_RES_NN_DIRECT",
                         "FME_RES_NN_EXTERN"}
    assert bits["FME_RES_NN_EXTERN"] == predictor.RES_NN_EXTERN == 0x08
    vals = list(bits.values())
    assert all(v and v & (v - 1) == 0 for v in vals) and len(set(vals)) == len(vals)   # single, distinct bits
    assert bits["FME_RES_NN_EXTERN"] < 1 << 16                                         # fits fme_result.status


def test_row_layout_of_the_header(tmp_path):
    """sizeof and offsetof as a C compiler sees include/fme_extern.h, against NN_ROW_DTYPE."""
    src = tmp_path / "row.c"
    fields = ("e", "c", "pu_h", "pu_w", "mv_int_x", "mv_int_y", "n_emi", "writes", "status", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fme_extern.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(fme_nn_row));\n' +
                   "".join(f'  printf(" %zu", offsetof(fme_nn_row, {f}));\n' for f in fields) +
                   '  printf(" %u", (unsigned)FME_RES_NN_EXTERN);\n  return 0;\n}\n')
    exe = str(tmp_path / "row")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    d = predictor.NN_ROW_DTYPE
    assert got[0] == 64 == d.itemsize
    assert got[1:-1] == [0, 32, 36, 40, 44, 46, 48, 49, 50, 52] == [d.fields[f][1] for f in fields]
    assert got[-1] == 0x08


def test_null_and_negative_arguments_rejected():
    lib = predictor.bind(runtime.load_library())
    one = 64 * b"\0"
    for f in (lib.fme_nn_inputs, lib.fme_nn_inputs_device):
        assert f(None, None, None, 1, None) == abi.E_INVALID
        assert b"bad argument" in lib.fme_last_error()
        assert f(None, one, one, 1, None) == abi.E_INVALID     # no context
        assert f(None, None, None, 0, None) == abi.E_INVALID   # n == 0 still needs one
        assert f(None, one, one, -1, None) == abi.E_INVALID
    for f in (lib.fme_refine_at, lib.fme_refine_at_device, lib.fme_refine_at_mv_device):
        assert f(None, None, None, None, None, 1, None) == abi.E_INVALID
        assert b"bad argument" in lib.fme_last_error()
        assert f(None, one, None, one, one, 1, None) == abi.E_INVALID
        assert f(None, None, None, None, None, 0, None) == abi.E_INVALID
        assert f(None, one, one, one, one, -1, None) == abi.E_INVALID
    assert lib.fme_refine_at_status(None) == abi.E_INVALID
    assert lib.fme_extern_last_ms(None, None) == abi.E_INVALID


def test_request_checks_of_the_entry_points(tmp_path):
    """The checks as the entry points call them: n == 0 is accepted (they return 0), a missing array
    or n < 0 is FME_E_INVALID, bound NN rows FME_E_STATE."""
    src = tmp_path / "req.cpp"
    src.write_text('#include <cstdio>\n#include "fme_extern_host.h"\nint main() { int c = 0, j = 0, r = 0, k = 0, o = 0;\n'
                   'std::printf("%d %d %d %d %d %d ", fme::extern_inputs_request(&c, &j, &r, 3, false),\n'
                   'fme::extern_inputs_request(&c, nullptr, nullptr, 0, false), fme::extern_inputs_request(&c, &j, nullptr, 3, false),\n'
                   'fme::extern_inputs_request(&c, &j, &r, -2, false), fme::extern_inputs_request(nullptr, &j, &r, 3, false),\n'
                   'fme::extern_inputs_request(&c, &j, &r, 3, true));\n'
                   'std::printf("%d %d %d %d %d %d", fme::extern_at_request(&c, &j, &k, &o, 3, false),\n'
                   'fme::extern_at_request(&c, nullptr, nullptr, nullptr, 0, false), fme::extern_at_request(&c, &j, nullptr, &o, 3, false),\n'
                   'fme::extern_at_request(&c, &j, &k, &o, -2, false), fme::extern_at_request(nullptr, &j, &k, &o, 3, false),\n'
                   'fme::extern_at_request(&c, &j, &k, &o, 3, true)); return 0; }\n')
    exe = str(tmp_path / "req")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "hm16.9-nn_fme_amd", "csrc"), str(src), "-o", exe],
                   check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == 2 * [0, 1, abi.E_INVALID, abi.E_INVALID, abi.E_INVALID, abi.E_STATE]
