"""include/fme_skip.h against the built library and the numpy mirrors (nnfme/skip.py): every
declared function is exported and outside the counted ABI, the records have the dtypes' layout (a
gcc -std=c99 probe), and null arguments are refused (CPU only)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from nnfme import merge, runtime, skip

HEADER = os.path.join(ROOT, "include", "fme_skip.h")


def skip_header_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fme_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_skip_header():
    lib = runtime.load_library()
    names = skip_header_functions()
    assert names == sorted(skip.SKIP_SYMBOLS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    skip.bind(lib)
    assert not set(names) & set(runtime.ABI_SYMBOLS)
    assert not set(names) & set(merge.MERGE_SYMBOLS)


def test_null_arguments_rejected():
    lib = skip.bind(runtime.load_library())
    assert lib.fme_pred_sse(None, None, None, 1, None) == -1
    assert lib.fme_pred_sse_device(None, None, None, 1, None) == -1
    assert lib.fme_pred_sse_invalid_count(None) == -1
    assert lib.fme_pred_sse_last_ms(None, None) == -1
    assert lib.fme_skip_estimate(None, None, None, None, 1, None) == -1
    assert b"fme_skip_estimate" in lib.fme_last_error()


def _probe_lines(dt, cname):
    out = [f'  printf("{cname} size %zu\\n", sizeof({cname}));']
    for name in dt.names:
        out.append(f'  printf("{cname} {name} %zu\\n", offsetof({cname}, {name}));')
    return out


def test_struct_layouts_match_dtypes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    records = [(skip.SSE_TASK_DTYPE, "fme_sse_task"), (skip.SKIP_PARAMS_DTYPE, "fme_skip_params"),
               (skip.SKIP_REQ_DTYPE, "fme_skip_req"), (skip.SKIP_RES_DTYPE, "fme_skip_res")]
    body = ["#include <stddef.h>", "#include <stdio.h>", '#include "fme_skip.h"', "int main(void) {"]
    for dt, cname in records:
        body += _probe_lines(dt, cname)
    body += ['  printf("consts %u %d\\n", FME_SKIP_NONE, FME_MRG_MAX_CAND);', "  return 0;", "}"]
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
    assert got[("consts", str(skip.SKIP_NONE))] == str(merge.MRG_MAX_CAND)
    # fme_sse_task is fme_pe_task's layout
    assert [skip.SSE_TASK_DTYPE.fields[n][1] for n in skip.SSE_TASK_DTYPE.names] == \
        [merge.PE_TASK_DTYPE.fields[n][1] for n in merge.PE_TASK_DTYPE.names]
