"""The C++ adapter (include/fme_hm.hpp) at bit depth 10: SearchConfig::bitDepth = 10, Pel and
16-bit picture planes, CtuRowBatcher rows with bi-pred keys, xPatternSearchFracDIF through the
resident server's 10-bit instance, NN_pred, InterSearchP and the error paths against the CPU
oracle at cfg.bit_depth = 10 (tests/cpp/test_hm_adapter10.cpp), and MotionCompensator's 16-bit
planes (setPictureYuv16 / setPictureYuv(Pel) / run16) against a mc10_* golden handed to the driver
as raw little-endian files."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, mc10_golden_cases
from nnfme.abi import MC_JOB_DTYPE

pytestmark = pytest.mark.gpu


def test_cpp_hm_adapter_main10(tmp_path):
    exe = os.path.join(ROOT, "hm16.9-nn_fme_amd", "host", "test_hm_adapter10")
    assert os.path.exists(exe), "build it with __graft_entry__.build() (make host-test)"
    g = load_golden(mc10_golden_cases()[0])
    assert int(g["bit_depth"][0]) == 10 and g["ref_y"].dtype == np.uint16
    refs, h, w = g["ref_y"].shape
    jobs = np.ascontiguousarray(g["jobs"], dtype=MC_JOB_DTYPE)
    assert MC_JOB_DTYPE.itemsize == 24
    np.array([refs, w, h, len(jobs), int(g["fill"][0])], dtype="<i4").tofile(tmp_path / "meta.bin")
    jobs.tofile(tmp_path / "jobs.bin")
    for name in ("ref_y", "ref_cb", "ref_cr", "pred_y", "pred_cb", "pred_cr"):
        np.ascontiguousarray(g[name], dtype="<u2").tofile(tmp_path / (name + ".bin"))
    p = subprocess.run([exe, "--mc10", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "hm adapter main10 ok" in p.stdout
    assert f"{len(jobs)} PU motion compensations" in p.stdout, p.stdout
