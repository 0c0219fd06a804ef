"""The known-motif search's kernels (mtr_amd/csrc/motif_search.hip.inc) against the resources their launches assume (CPU; reads the gfx950
code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  Every instantiation of the lane kernel and the pack kernel:
no scratch, no spills, four wavefronts per SIMD by registers, the LDS budget of the report kernels (tests/test_report_motif_resources.py).
The wave kernel is mtr_k_dp_test with another task source: it may take no more of anything than that kernel does."""
import os

import pytest

from tests.test_kernel_resources import LDS_PER_CU, LIB, READELF, _find, _kernels

BUCKETS = (4, 8, 16, 32)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def test_every_bucket_of_the_lane_kernel_is_built(kernels):
    names = [k["name"] for k in _find(kernels, "mtr_k_motif_lanes")]
    assert sorted(names) == sorted(f"_Z17mtr_k_motif_lanesILi{b}EEv15MotifSearchArgs" for b in BUCKETS), names


@pytest.mark.parametrize("stem", ["mtr_k_motif_lanes", "mtr_k_motif_pack"])
def test_lane_and_pack_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    found = _find(kernels, stem)
    assert found, stem
    for k in found:
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 10240, k


def test_the_wave_kernel_takes_no_more_than_mtr_k_dp_test(kernels):
    (wave,), (dp_test,) = _find(kernels, "mtr_k_motif_waves"), _find(kernels, "mtr_k_dp_test")
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "group_segment_fixed_size"):
        assert wave.get(key, 0) <= dp_test.get(key, 0), (key, wave, dp_test)
    assert wave["group_segment_fixed_size"] <= LDS_PER_CU // 16 and wave["vgpr_count"] <= 128
