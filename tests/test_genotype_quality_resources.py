"""The genotype quality's kernels (mtr_amd/csrc/genotype_quality.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code
object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  No kernel spills and none takes private scratch memory - the score
kernel keeps nothing per cell; mtr_k_gq_score, one wavefront per workgroup in all four instantiations (four alignments per wavefront, two, one
with one pair of diagonals per lane, one with two), stays within 128 VGPRs (four wavefronts per SIMD) and uses no LDS, and neither does any
other kernel of the file; and the file's kernels are exactly the ones listed."""
import os
import re

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

LDS = {"mtr_k_gq_check": 0, "mtr_k_gq_tasks": 0, "mtr_k_gq_score": 0, "mtr_k_gq_locus": 0}
INSTANCES = {"mtr_k_gq_score": 4}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("gq"))


@pytest.mark.parametrize("stem", sorted(LDS))
def test_no_scratch_no_spills_no_lds_and_four_wavefronts_per_simd(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == INSTANCES.get(stem, 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs, {k['group_segment_fixed_size']} bytes of LDS, {k['private_segment_fixed_size']} of scratch")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == LDS[stem], k
        assert k["vgpr_count"] <= 128, k


def test_the_kernels_are_the_ones_listed():
    src = open(os.path.join(os.path.dirname(LIB), "csrc", "genotype_quality.hip.inc")).read()
    assert sorted(set(re.findall(r"__global__[^\n]*\bvoid (mtr_k_\w+)\(", src))) == sorted(LDS)
