"""include/fme_merge.h against the built library and the numpy mirrors (nnfme/merge.py): every
declared function is exported, the three records have the dtypes' layout (a gcc probe), null
arguments are refused, and include/fme.h still declares its 61 functions (CPU only)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from nnfme import merge, runtime
from test_abi import header_functions

HEADER = os.path.join(ROOT, "include", "fme_merge.h")


def merge_header_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fme_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_merge_header():
    lib = runtime.load_library()
    names = merge_header_functions()
    assert names == sorted(merge.MERGE_SYMBOLS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    merge.bind(lib)
    assert not set(names) & set(runtime.ABI_SYMBOLS)


def test_fme_h_unchanged_surface():
    assert len(header_functions()) == 61
    assert set(header_functions()) == set(runtime.ABI_SYMBOLS)
    assert runtime.load_library().fme_abi_version() == 18


def test_null_arguments_rejected():
    lib = merge.bind(runtime.load_library())
    assert lib.fme_pred_error(None, None, None, 1, None) == -1
    assert lib.fme_pred_error_device(None, None, None, 1, None) == -1
    assert lib.fme_pred_error_invalid_count(None) == -1
    assert lib.fme_pred_error_last_ms(None, None) == -1
    assert lib.fme_merge_estimate(None, None, None, 1, None) == -1
    assert b"fme_merge_estimate" in lib.fme_last_error()


def _probe_lines(dt, cname):
    out = [f'  printf("{cname} size %zu\\n", sizeof({cname}));']
    for name in dt.names:
        out.append(f'  printf("{cname} {name} %zu\\n", offsetof({cname}, {name}));')
    return out


def test_struct_layouts_match_dtypes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    records = [(merge.PE_TASK_DTYPE, "fme_pe_task"), (merge.MERGE_CAND_DTYPE, "fme_merge_cand"),
               (merge.MERGE_REQ_DTYPE, "fme_merge_req"), (merge.MERGE_RES_DTYPE, "fme_merge_res")]
    body = ["#include <stddef.h>", "#include <stdio.h>", '#include "fme_merge.h"', "int main(void) {"]
    for dt, cname in records:
        body += _probe_lines(dt, cname)
    body += ['  printf("flags %u %u %d\\n", FME_PE_LOSSLESS, FME_MRG_HAS_ME, FME_MRG_MAX_CAND);', "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(body) + "\n")
    exe = str(tmp_path / "probe")
    # plain C: the header is usable from C callers
    b = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                       capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stdout + b.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=30, check=True).stdout
    got = {}
    for line in out.splitlines():
        a, b_, c = line.split(" ", 2)
        got[(a, b_)] = c
    for dt, cname in records:
        assert int(got[(cname, "size")]) == dt.itemsize, cname
        for name in dt.names:
            assert int(got[(cname, name)]) == dt.fields[name][1], (cname, name)
    assert got[("flags", str(merge.PE_LOSSLESS))] == f"{merge.MRG_HAS_ME} {merge.MRG_MAX_CAND}"
