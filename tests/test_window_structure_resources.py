"""The window structure's kernels (mtr_amd/csrc/window_structure.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code
object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  No kernel spills and none takes private scratch memory: a lane's
previous row - four register arrays of the bucket's width - and its structure stay in registers, which is the whole point of one window per lane.
LDS appears only in the task kernel, at exactly the declared size (one start per key).  The lanes kernel runs one wavefront per workgroup, so its
launch assumes nothing but that a wavefront fits the 512 registers a lane can have; what each instantiation takes decides the wavefronts per SIMD
(DESIGN.md 7i-13's table): at most 128 registers for <8, narrow> (four), at most 256 for <16, narrow> and <8, wide> (two), and for <32, narrow>
and <16, wide> one wavefront at the least - no spill, no scratch and at most 512."""
import os
import re

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

LDS = {"mtr_k_ws_check": 0, "mtr_k_ws_bases": 0, "mtr_k_ws_tasks": 5 * 16 * 4, "mtr_k_ws_lanes": 0, "mtr_k_ws_output": 0}
INSTANCES = {"mtr_k_ws_lanes": 5}
LANES_VGPRS = {"ILi8ELb0EE": 128, "ILi16ELb0EE": 256, "ILi32ELb0EE": 512, "ILi8ELb1EE": 256, "ILi16ELb1EE": 512}      # <UB, WIDE> as mangled: the registers its wavefronts per SIMD allow


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", sorted(LDS))
def test_no_scratch_no_spills_and_the_declared_lds(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == INSTANCES.get(stem, 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs, {k['group_segment_fixed_size']} bytes of LDS, {k['private_segment_fixed_size']} of scratch")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == LDS[stem], k
        if stem != "mtr_k_ws_lanes":
            assert k["vgpr_count"] <= 64, k


def test_each_lanes_instantiation_within_the_registers_of_its_wavefronts_per_simd(kernels):
    found = {k["name"]: k for k in _find(kernels, "mtr_k_ws_lanes")}
    for tag, limit in LANES_VGPRS.items():
        k = [v for name, v in found.items() if tag in name]
        assert len(k) == 1, (tag, sorted(found))
        assert k[0]["vgpr_count"] + (k[0].get("agpr_count") or 0) <= limit, k[0]


def test_the_kernels_are_the_ones_listed():
    src = open(os.path.join(os.path.dirname(LIB), "csrc", "window_structure.hip.inc")).read()
    assert sorted(set(re.findall(r"__global__[^\n]*\bvoid (mtr_k_\w+)\(", src))) == sorted(LDS)
