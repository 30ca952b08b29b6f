"""What the ISA of the PPO gradient's matrix-core unit (csrc/pbg_ppograd_mfma.hip) must show beyond
tests/test_isa_exec_copies.py's table, which holds its kernel list, the partial-EXEC copy check and its place in the
Makefile: both kernels use the float32 matrix instruction and neither uses scratch.  CPU only (hipcc cross-compiles
gfx950)."""
import re
import shutil

import pytest

from test_isa_exec_copies import compile_unit, isa_uninit


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
def test_the_kernels_use_the_matrix_cores_and_no_scratch(tmp_path):
    out = compile_unit(tmp_path, "ppograd_mfma")
    names = isa_uninit.kernels(str(out))
    assert len(names) == 2, names
    text = out.read_text()
    for k in names:
        body = text[text.index(f"\n{k}:"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert "v_mfma_f32_16x16x4_f32" in body, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), k
