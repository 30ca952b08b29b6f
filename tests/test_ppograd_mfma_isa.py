"""The matrix-core translation unit of the PPO gradient (csrc/pbg_ppograd_mfma.hip) compiled from this tree with the
Makefile's HIPFLAGS: both kernels are there, neither holds a register copy under a partial EXEC
(tests/test_isa_exec_copies.py's check, which lists the units of SHARED_OBJS; this unit is linked through MFMA_OBJS),
both use the float32 matrix instruction and neither uses scratch."""
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_uninit  # noqa: E402

KERNELS = ("ppograd_mfma_kernelILb1E", "ppograd_mfma_kernelILb0E")


def test_the_makefile_links_and_reports_the_unit():
    mk = open(os.path.join(REPO, "pybullet-gym_amd", "Makefile")).read()
    assert "MFMA_OBJS = $(OBJ)/ppograd_mfma.o" in mk
    link = [ln for ln in mk.split("\n") if "$$(SHARED_OBJS)" in ln or ln.startswith("TRACE_REST =")]
    assert len(link) == 2 and all("MFMA_OBJS)" in ln for ln in link), link
    assert mk.count("-c -o /dev/null csrc/pbg_ppograd_mfma.hip") == 1   # make policy-report


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
def test_the_kernels_have_no_partial_exec_copies_use_the_matrix_cores_and_no_scratch(tmp_path):
    out = tmp_path / "ppograd_mfma.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                           "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(REPO, "pybullet-gym_amd", "csrc", "pbg_ppograd_mfma.hip")], stderr=subprocess.DEVNULL)
    names = isa_uninit.kernels(str(out))
    for want in KERNELS:
        assert sum(want in k for k in names) == 1, (want, names)
    assert len(names) == len(KERNELS), names
    text = out.read_text()
    for k in names:
        assert isa_uninit.exec_copies(isa_uninit.parse(str(out), k)) == [], k
        body = text[text.index(f"\n{k}:"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert "v_mfma_f32_16x16x4_f32" in body, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), k
