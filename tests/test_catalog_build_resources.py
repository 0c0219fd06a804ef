"""The kernels that build a prepared catalogue (mtr_amd/csrc/catalog_build.hip.inc) against the resources their launches assume (CPU; reads the
gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  No kernel takes scratch or spills - the slot kernel's
per-lane pattern lives in LDS for that reason, fbv_masks' four masks in registers; LDS is what the kernels declare statically (the launches
pass none): 64 lanes x 68 bytes of pattern codes, and 256 counters of the sort's two kernels; the VGPRs are at the numbers the build shows."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

# stem -> (LDS bytes the kernel declares, VGPRs of the build)
KERNELS = {"mtr_k_catb_check": (0, 15), "mtr_k_catb_slots": (64 * 68, 35), "mtr_k_catb_count": (256 * 4, 12), "mtr_k_catb_fill": (256 * 4, 29),
           "mtr_k_catb_flags": (0, 8), "mtr_k_catb_compact": (0, 9), "mtr_k_catb_table": (0, 10), "mtr_k_catb_motifs": (0, 20)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", sorted(KERNELS))
def test_no_scratch_no_spills_lds_as_declared_and_the_vgprs_of_the_build(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == 1, (stem, found)
    k = found[0]
    lds, vgprs = KERNELS[stem]
    print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs, {k['group_segment_fixed_size']} bytes of LDS")
    assert k["private_segment_fixed_size"] == 0, k
    assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
    assert k["group_segment_fixed_size"] <= lds, k
    assert k["vgpr_count"] <= vgprs, k


def test_these_are_all_the_build_kernels(kernels):
    assert sorted(n for n in kernels if "mtr_k_catb_" in n) == sorted(k["name"] for s in KERNELS for k in _find(kernels, s))
