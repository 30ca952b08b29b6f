"""The permutation unit (csrc/pbg_perm.hip) under tests/test_isa_exec_copies.py's ISA check, and its place in the
Makefile: it is linked into every library variant through PERM_OBJS, beside SHARED_OBJS.  CPU only (hipcc cross-compiles
gfx950)."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_uninit  # noqa: E402

PERM_KERNELS = ["perm_fill_kernel", "perm_advance_kernel", "perm_set_kernel", "lr_linear_kernel"]


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
def test_perm_kernels_have_no_partial_exec_copies_and_scalar_round_keys(tmp_path):
    """Compiled from this tree with the Makefile's HIPFLAGS: every kernel of the unit is there, none copies a live
    register inside a divergent region's join block, and the fill's two Philox blocks are scalar multiplies (the round
    keys are computed once per wave on scalar registers, not per element)."""
    out = tmp_path / "perm.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                           "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(REPO, "pybullet-gym_amd", "csrc", "pbg_perm.hip")], stderr=subprocess.DEVNULL)
    names = isa_uninit.kernels(str(out))
    for want in PERM_KERNELS:
        assert sum(want in k for k in names) == 1, (want, names)
    assert len(names) == len(PERM_KERNELS), names
    for k in names:
        assert isa_uninit.exec_copies(isa_uninit.parse(str(out), k)) == [], k
    text = out.read_text()
    fill = text[text.index("perm_fill_kernel"):text.index("perm_advance_kernel")]
    assert "s_mul_hi_u32" in fill and "v_mul_hi_u32" not in fill


def test_the_perm_unit_is_linked_into_every_library_variant():
    mk = open(os.path.join(REPO, "pybullet-gym_amd", "Makefile")).read()
    assert "PERM_OBJS = $(OBJ)/perm.o" in mk.split("\n")
    link = next(ln for ln in mk.split("\n") if ln.startswith("$(3):"))
    assert "$$(SHARED_OBJS) $$(PERM_OBJS)" in link
    assert "csrc/pbg_perm.hip" in mk[mk.index("policy-report:"):mk.index("devtest:")]
