"""The window edits' kernels (mtr_amd/csrc/window_edits.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code object
out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  No kernel spills and none takes private scratch memory.  The rows kernel
runs one wavefront per workgroup.  <8, narrow>, <16, narrow> and <8, wide> keep the previous row in register arrays as their mtr_k_ws_lanes twins
do, declare no LDS and are held to their twins' classes: 128, 256 and 256 registers.  <32, narrow> and <16, wide> left their twins' class of 512
downwards (DESIGN.md 7i-16's table): the previous row in LDS at exactly the declared size - 32 columns x 64 lanes x 16 bytes, and 16 x 64 x 28 -
the column loops not unrolled, at most 128 registers."""
import os
import re

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

KERNELS = ["mtr_k_we_groups", "mtr_k_we_rows", "mtr_k_we_count", "mtr_k_we_emit", "mtr_k_we_output"]
INSTANCES = {"mtr_k_we_rows": 5}
ROWS_VGPRS = {"ILi8ELb0EE": 128, "ILi16ELb0EE": 256, "ILi32ELb0EE": 128, "ILi8ELb1EE": 256, "ILi16ELb1EE": 128}      # <UB, WIDE> as mangled
ROWS_LDS = {"ILi8ELb0EE": 0, "ILi16ELb0EE": 0, "ILi32ELb0EE": 32 * 64 * 16, "ILi8ELb1EE": 0, "ILi16ELb1EE": 16 * 64 * 28}
WS_TWIN = {"ILi8ELb0EE": 128, "ILi16ELb0EE": 256, "ILi32ELb0EE": 512, "ILi8ELb1EE": 256, "ILi16ELb1EE": 512}
LEFT_ITS_CLASS = {"ILi32ELb0EE", "ILi16ELb1EE"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", KERNELS)
def test_no_scratch_no_spills_and_the_declared_lds(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == INSTANCES.get(stem, 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs, {k['group_segment_fixed_size']} bytes of LDS, {k['private_segment_fixed_size']} of scratch")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == (0 if stem != "mtr_k_we_rows" else [v for tag, v in ROWS_LDS.items() if tag in k["name"]][0]), k
        if stem != "mtr_k_we_rows":
            assert k["vgpr_count"] <= 64, k


def test_each_rows_instantiation_within_the_registers_of_its_class(kernels):
    found = {k["name"]: k for k in _find(kernels, "mtr_k_we_rows")}
    for tag, limit in ROWS_VGPRS.items():
        k = [v for name, v in found.items() if tag in name]
        assert len(k) == 1, (tag, sorted(found))
        assert k[0]["vgpr_count"] + (k[0].get("agpr_count") or 0) <= limit, k[0]
        assert (limit == WS_TWIN[tag]) != (tag in LEFT_ITS_CLASS), tag


def test_the_kernels_are_the_ones_listed():
    src = open(os.path.join(os.path.dirname(LIB), "csrc", "window_edits.hip.inc")).read()
    assert sorted(set(re.findall(r"__global__[^\n]*\bvoid (mtr_k_\w+)\(", src))) == sorted(KERNELS)
    assert all(name.startswith("mtr_k_we_") for name in KERNELS)
