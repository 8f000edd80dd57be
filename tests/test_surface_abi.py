"""include/fme_surface.h against the built library and the numpy mirrors (nnfme/surface.py): every
declared function is exported and outside the counted ABI, the records have the dtypes' layout (a
gcc -std=c99 probe), and bad arguments are refused (CPU only)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from nnfme import merge, runtime, skip, surface

HEADER = os.path.join(ROOT, "include", "fme_surface.h")


def surface_header_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fme_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_surface_header():
    lib = runtime.load_library()
    names = surface_header_functions()
    assert names == sorted(surface.SURFACE_SYMBOLS) and len(names) == 4
    for n in names:
        assert hasattr(lib, n), n
    surface.bind(lib)
    assert not set(names) & set(runtime.ABI_SYMBOLS)
    assert not set(names) & (set(merge.MERGE_SYMBOLS) | set(skip.SKIP_SYMBOLS))
    assert lib.fme_abi_version() == 18   # fme.h keeps its functions and its version


def test_bad_arguments_rejected():
    lib = surface.bind(runtime.load_library())
    assert lib.fme_cost_surface(None, None, None, None, None, 1, None) == -1
    assert b"fme_cost_surface" in lib.fme_last_error()
    assert lib.fme_cost_surface_device(None, None, None, None, None, 1, None) == -1
    assert lib.fme_cost_surface_invalid_count(None) == -1
    assert lib.fme_cost_surface_last_ms(None, None) == -1


def test_struct_layouts_match_dtypes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    records = [(surface.SURFACE_DTYPE, "fme_surface"), (surface.PICK_DTYPE, "fme_surface_pick")]
    body = ["#include <stddef.h>", "#include <stdio.h>", '#include "fme_surface.h"', "int main(void) {"]
    for dt, cname in records:
        body.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for name in dt.names:
            body.append(f'  printf("{cname} {name} %zu\\n", offsetof({cname}, {name}));')
    body += ['  printf("consts %d %u %d\\n", FME_SURF_POINTS, FME_SURF_NO_PROBE, FME_SURF_INDEX(-3, -3) + FME_SURF_INDEX(3, 3));',
             "  return 0;", "}"]
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
    assert got[("consts", str(surface.POINTS))] == f"{surface.NO_PROBE} 48"
