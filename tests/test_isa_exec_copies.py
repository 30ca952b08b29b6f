"""The float64 quad miscompile's bug class, checked on the ISA.

Round 5's default-schedule build of team_step_kernel<F64<Ant>,16> copied two live-through doubles
into AGPRs inside a divergent region's join block, before the `s_or_b64 exec, exec, sN` that restores
the region's lanes; lanes outside the region then read stale registers (found on the GPU by
register-file poisoning, tools/vgpr_poison_probe.py).  tools/isa_uninit.py --exec-copies flags that
pattern; these tests pin the checker on a synthetic reproducer and run it over the product's float64
quad kernels and over every translation unit of the learner compiled from this tree.  CPU only (hipcc
cross-compiles gfx950).
"""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_uninit  # noqa: E402

KERNEL = "_Z6kernelv"
FAULTY = f"""{KERNEL}:                  ; @{KERNEL}
; %bb.0:
	v_mov_b32_e32 v240, v1
	v_mov_b32_e32 v241, v2
	v_cmp_gt_f64_e32 vcc, 0, v[4:5]
	s_and_saveexec_b64 s[18:19], vcc
	s_cbranch_execz .LBB0_2
; %bb.1:
	v_add_f64 v[6:7], v[6:7], v[240:241]
.LBB0_2:
	v_accvgpr_write_b32 a54, v240
	v_accvgpr_write_b32 a55, v241
	s_or_b64 exec, exec, s[18:19]
	v_accvgpr_read_b32 v8, a54
	v_accvgpr_read_b32 v9, a55
	v_add_f64 v[6:7], v[6:7], v[8:9]
	s_endpgm
.Lfunc_end0:
"""
# the same copies after the EXEC restore (every lane copies): correct code
FIXED = FAULTY.replace("""	v_accvgpr_write_b32 a54, v240
	v_accvgpr_write_b32 a55, v241
	s_or_b64 exec, exec, s[18:19]
""", """	s_or_b64 exec, exec, s[18:19]
	v_accvgpr_write_b32 a54, v240
	v_accvgpr_write_b32 a55, v241
""")
# a value computed inside the region and copied there is the region's own business (not flagged)
INSIDE = FAULTY.replace("""; %bb.1:
	v_add_f64 v[6:7], v[6:7], v[240:241]
""", """; %bb.1:
	v_add_f64 v[240:241], v[6:7], v[240:241]
""")

# the spill form: a live-through value stored to a scratch slot under the region's EXEC, reloaded after
SPILL = FAULTY.replace("""	v_accvgpr_write_b32 a54, v240
	v_accvgpr_write_b32 a55, v241
	s_or_b64 exec, exec, s[18:19]
	v_accvgpr_read_b32 v8, a54
	v_accvgpr_read_b32 v9, a55
""", """	scratch_store_dwordx2 off, v[240:241], off offset:16 ; 8-byte Folded Spill
	s_or_b64 exec, exec, s[18:19]
	scratch_load_dwordx2 v[8:9], off, off offset:16 ; 8-byte Folded Reload
""")


def _check(tmp_path, text):
    p = tmp_path / "k.s"
    p.write_text(text)
    return isa_uninit.exec_copies(isa_uninit.parse(str(p), KERNEL))


def test_checker_flags_the_round5_pattern(tmp_path):
    hits = _check(tmp_path, FAULTY)
    assert [h[1] for h in hits] == ["v_accvgpr_write_b32 a54, v240", "v_accvgpr_write_b32 a55, v241"]


def test_checker_flags_the_spill_form(tmp_path):
    hits = _check(tmp_path, SPILL)
    assert len(hits) == 1 and hits[0][1].startswith("scratch_store_dwordx2 off, v[240:241]")


def test_checker_passes_copies_after_the_exec_restore(tmp_path):
    assert _check(tmp_path, FIXED) == []
    assert _check(tmp_path, INSIDE) == []


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
@pytest.mark.parametrize("robot", ["Ant", "AntMuJoCo"])
def test_product_float64_quad_kernel_has_no_partial_exec_copies(tmp_path, robot):
    """The product's float64 quad translation unit (Makefile T64FLAGS), compiled from this tree."""
    out = tmp_path / f"team64_{robot}.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                           "-DPBG_TEAM64_TU", f"-DPBG_ROBOT={robot}", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(REPO, "pybullet-gym_amd", "csrc", "pbg_robot.hip")],
                          stderr=subprocess.DEVNULL)
    names = [k for k in isa_uninit.kernels(str(out)) if "team_step_kernel" in k]
    assert names, "no quad kernel in the ISA"
    for k in names:
        assert isa_uninit.exec_copies(isa_uninit.parse(str(out), k)) == [], k


# the learner's translation units (Makefile LEARNER_UNITS) and the kernels each must hold, by a substring of the
# mangled name: 43 in all.  A unit added to the Makefile must be added here.
LEARNER_UNITS = {
    "policy": [f"actor_kernelILi{mode}ELb{sample}E" for sample in (0, 1) for mode in (0, 1, 2)] +
              ["book_kernelILb0E", "book_kernelILb1E"],
    "population": ["noise_kernel", "perturb_kernel", "grad_kernel", "fitness_kernel", "copy_rows_kernel"],
    "obsnorm": ["obs_stats_update_kernel", "obs_stats_finalize_kernel"],
    "actnoise": ["action_noise_fill_kernel", "gae_kernel"],
    "ppograd": ["ppograd_tiles_kernelILb1E", "ppograd_tiles_kernelILb0E", "ppograd_reduce_kernel"],
    "ppoopt": ["adv_norm_kernel", "ppoopt_sumsq_kernel", "ppoopt_step_kernel", "ppoopt_reset_kernel"],
    "perm": ["perm_fill_kernel", "perm_advance_kernel", "perm_set_kernel", "lr_linear_kernel"],
    "ppograd_mfma": ["ppograd_mfma_kernelILb1E", "ppograd_mfma_kernelILb0E"],
    "obsslots": ["obs_stats_slots_kernelILb0E", "obs_stats_slots_kernelILb1E"],
    "trunc": ["gae_trunc_kernel", "actor_where_kernelILi0E", "actor_where_kernelILi1E"],
    "retstats": ["ret_walk_kernel", "ret_finalize_kernel", "ret_copy_kernel", "ret_reset_kernel", "ret_apply_kernelILb0E",
                 "ret_apply_kernelILb1E"],
    "ppogate": ["ppo_gate_kernel", "ppo_gate_reset_kernel"],
}


def compile_unit(tmp_path, unit):
    """csrc/pbg_<unit>.hip's device ISA, compiled from this tree with the Makefile's HIPFLAGS: the file's path."""
    out = tmp_path / f"{unit}.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                           "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(REPO, "pybullet-gym_amd", "csrc", f"pbg_{unit}.hip")],
                          stderr=subprocess.DEVNULL)
    return out


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
@pytest.mark.parametrize("unit", list(LEARNER_UNITS))
def test_learner_kernels_have_no_partial_exec_copies(tmp_path, unit):
    """Every learner unit -- the actors, the population's and the statistics' kernels, the noise fill, GAE, the PPO
    gradient on both paths (whose register path runs into the AGPR half), the optimiser step, the permutations,
    truncation, the return statistics and the KL gate: every kernel of the unit is there and none copies a live
    register inside a divergent region's join block."""
    out = compile_unit(tmp_path, unit)
    names = isa_uninit.kernels(str(out))
    for want in LEARNER_UNITS[unit]:
        assert sum(want in k for k in names) == 1, (want, names)
    assert len(names) == len(LEARNER_UNITS[unit]), names
    for k in names:
        assert isa_uninit.exec_copies(isa_uninit.parse(str(out), k)) == [], k


def test_the_learner_units_are_the_makefiles():
    """The table above is the Makefile's LEARNER_UNITS, and that list is what every library variant links
    (LIB_RULES, TRACE_REST) and what `make policy-report` covers."""
    mk = open(os.path.join(REPO, "pybullet-gym_amd", "Makefile")).read().split("\n")
    units = next(ln for ln in mk if ln.startswith("LEARNER_UNITS :=")).split(":=")[1].split()
    assert sorted(units) == sorted(LEARNER_UNITS) and len(units) == len(set(units)) == 12
    assert sum(len(v) for v in LEARNER_UNITS.values()) == 43
    assert "LEARNER_OBJS := $(LEARNER_UNITS:%=$(OBJ)/%.o)" in mk
    link = next(ln for ln in mk if ln.startswith("$(3):"))
    assert link.split()[-2:] == ["$(1)/capi.o", "$$(LEARNER_OBJS)"]
    rest = next(ln for ln in mk if ln.startswith("TRACE_REST ="))
    assert rest.split()[-2:] == ["$(OBJ)/capi.o", "$(LEARNER_OBJS)"]
    report = subprocess.run(["make", "-n", "-C", os.path.join(REPO, "pybullet-gym_amd"), "policy-report"],
                            capture_output=True, text=True, check=True).stdout
    for u in units:
        assert report.count(f"-Rpass-analysis=kernel-resource-usage -c -o /dev/null csrc/pbg_{u}.hip") == 1, u


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc absent")
def test_round5_source_reproduces_the_faulting_copies(tmp_path):
    """The real instance: the round-5 source (commit 4428492, stored as
    tests/golden/r05_quad_source.tar.gz) on the default schedule has the split
    copies of a54 / a55 / a180 / a181 before the region's EXEC restore -- the registers the GPU
    register-file bisection found (profiles/r06_f64_quad_miscompile/register_bisect.txt) -- and the
    trackers build it shipped with has none (tools/repro_r05_miscompile.sh)."""
    out = subprocess.run(["bash", os.path.join(REPO, "tools", "repro_r05_miscompile.sh"), str(tmp_path / "w")],
                         capture_output=True, text=True, timeout=800).stdout
    default, trackers = out.split("trackers.s:")
    for reg in ("a54, v", "a55, v", "a180, v", "a181, v"):
        assert f"v_accvgpr_write_b32 {reg}" in default, (reg, out)
    assert trackers.strip().startswith("0 copies"), out
