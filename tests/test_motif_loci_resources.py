"""The locus search's kernels (mtr_amd/csrc/motif_loci.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code object out
of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  Every instantiation of the windowed lane kernel: no scratch, no spills, no LDS,
four wavefronts per SIMD by registers (the host gives them 16 wavefronts per CU) and no more registers than the search's own lane kernel of the
same bucket plus the window's few.  The service kernels: no scratch, no LDS.  The wave kernel is mtr_k_motif_waves with another task source."""
import os

import pytest

from tests.test_kernel_resources import LDS_PER_CU, LIB, READELF, _find, _kernels

BUCKETS = (4, 8, 16, 32)
SERVICE = ("mtr_k_loci_init", "mtr_k_loci_bin", "mtr_k_loci_groups", "mtr_k_loci_scatter", "mtr_k_loci_split", "mtr_k_loci_count", "mtr_k_loci_starts",
           "mtr_k_loci_place")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def test_every_bucket_of_the_lane_kernel_is_built(kernels):
    names = [k["name"] for k in _find(kernels, "mtr_k_motif_loci_lanes")]
    assert sorted(names) == sorted(f"_Z22mtr_k_motif_loci_lanesILi{b}EEv8LociArgs" for b in BUCKETS), names


def test_the_lane_kernels_have_no_scratch_no_lds_and_the_registers_the_launch_assumes(kernels):
    search = {k["name"]: k for k in _find(kernels, "mtr_k_motif_lanes")}
    for b in BUCKETS:
        (k,) = [k for k in _find(kernels, "mtr_k_motif_loci_lanes") if f"ILi{b}E" in k["name"]]
        (s,) = [v for n, v in search.items() if f"ILi{b}E" in n]
        print(f"mtr_k_motif_loci_lanes<{b}>: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs; mtr_k_motif_lanes<{b}>: {s['vgpr_count']} VGPRs")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == 0, k
        assert k["vgpr_count"] <= 128, k                                   # 16 wavefronts per CU = four per SIMD
        assert k["vgpr_count"] <= s["vgpr_count"] + 8, (k, s)              # the window: its first base, the task, the interval


@pytest.mark.parametrize("stem", SERVICE)
def test_the_service_kernels_have_no_scratch_and_no_lds(kernels, stem):
    found = [k for k in _find(kernels, stem)]
    assert len(found) == 1, (stem, found)
    (k,) = found
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0 and k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 64, k


def test_the_wave_kernel_takes_no_more_than_the_searchs(kernels):
    (wave,), (search,) = _find(kernels, "mtr_k_motif_loci_waves"), _find(kernels, "mtr_k_motif_waves")
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size"):
        assert wave.get(key, 0) <= search.get(key, 0), (key, wave, search)
    assert wave["vgpr_count"] <= max(search["vgpr_count"], 128) and wave["group_segment_fixed_size"] <= LDS_PER_CU // 16
