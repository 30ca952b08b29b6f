"""The robot registry: robots.SPECS is the one place a robot's id, struct name, env id and key are written;
the generated header, the bindings' maps, the package's ENV_IDS and the env-class registry must all agree
with it (no GPU needed)."""
import ctypes
import os
import re

import pytest

import oracle
import pybulletgym_amd
from pybulletgym_amd import _native, codegen, envs, robots


def test_ids_are_dense():
    assert sorted(s.robot_id for s in robots.SPECS.values()) == list(range(len(robots.SPECS)))
    assert [s.robot_id for s in robots.BY_ID] == list(range(len(robots.SPECS)))
    for field in ("struct", "env_id", "key"):
        assert len({getattr(s, field) for s in robots.BY_ID}) == len(robots.BY_ID), field


def test_committed_header_matches_the_specs():
    src = open(codegen.HEADER).read()
    want = [(s.struct, s.robot_id, s.env_id, s.key) for s in robots.BY_ID]
    # the structs, in file order, with the id each carries
    structs = re.findall(r"^struct (\w+) \{\n  static constexpr int robot_id = (\d+);", src, re.M)
    assert [(n, int(i)) for n, i in structs] == [w[:2] for w in want]
    # the X-macro rows and the count
    macro = src[src.index("#define PBG_ROBOTS(X)"):]
    rows = re.findall(r'^  X\((\w+), (\d+), "([^"]+)", "([^"]+)"\)', macro, re.M)
    assert [(n, int(i), e, k) for n, i, e, k in rows] == want
    assert re.search(r"^#define PBG_N_ROBOTS (\d+)$", macro, re.M).group(1) == str(len(want))


@pytest.mark.skipif(not os.path.exists(_native.LIB_PATH), reason="libpbg_amd.so not built")
def test_library_knows_exactly_the_specs_names():
    L = _native.lib()
    p, iw, ow = _native.SimParams(), ctypes.c_int(), ctypes.c_int()
    for s in robots.BY_ID:
        for name in (s.env_id, s.key):
            assert L.pbg_default_sim_params(name.encode(), ctypes.byref(p)) == 0, name
            assert p.frame_skip == s.frame_skip and p.timestep == s.timestep, name
            assert L.pbg_pack_record_sizes(name.encode(), ctypes.byref(iw), ctypes.byref(ow)) == 0, name
            assert ow.value >= s.obs_dim, name
    for name in ("NoSuchEnv-v0", "", "Ant", "antt", "AntPyBulletEnv-v1", robots.BY_ID[0].struct):
        assert L.pbg_default_sim_params(name.encode(), ctypes.byref(p)) == -2, name  # PBG_E_ENV
        assert L.pbg_pack_record_sizes(name.encode(), ctypes.byref(iw), ctypes.byref(ow)) == -2, name
        assert b"unknown env id" in L.pbg_last_error()


def test_every_list_derives_from_the_specs():
    env_ids = [s.env_id for s in robots.BY_ID]
    assert set(envs.ENV_CLASSES) == set(env_ids) and len(envs.ENV_CLASSES) == len(env_ids)
    for env_id, cls in envs.ENV_CLASSES.items():
        assert cls.env_id == env_id
    assert _native.ROBOT_IDS == {s.env_id: s.robot_id for s in robots.BY_ID}
    assert oracle.ROBOT_IDS == {s.key: s.robot_id for s in robots.BY_ID}
    assert oracle.ENV_KEYS == {s.env_id: s.key for s in robots.BY_ID}
    assert pybulletgym_amd.ENV_IDS == tuple(env_ids)
