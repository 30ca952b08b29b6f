"""What the permutation unit's ISA (csrc/pbg_perm.hip) must show beyond tests/test_isa_exec_copies.py's table, which
holds its kernel list, the partial-EXEC copy check and its place in the Makefile.  CPU only (hipcc cross-compiles
gfx950)."""
import shutil

import pytest

from test_isa_exec_copies import compile_unit


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
def test_the_perm_fill_has_scalar_round_keys(tmp_path):
    """The fill's two Philox blocks are scalar multiplies: the round keys are computed once per wave on scalar
    registers, not per element."""
    text = compile_unit(tmp_path, "perm").read_text()
    fill = text[text.index("perm_fill_kernel"):text.index("perm_advance_kernel")]
    assert "s_mul_hi_u32" in fill and "v_mul_hi_u32" not in fill
