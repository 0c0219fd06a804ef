"""The sequence allele calls' kernels (mtr_amd/csrc/seq_calls.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code
object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  No kernel spills and none takes private scratch memory - the
distance kernel keeps nothing per cell; mtr_k_seq_dist, one wavefront per workgroup in all four instantiations (four alignments per wavefront,
two, one with one pair of diagonals per lane, one with two), stays within 128 VGPRs (four wavefronts per SIMD) and uses no LDS; LDS appears only in
the split, at exactly the declared size - the locus' 128 x 128 distance bytes; and the file's kernels are exactly the ones listed."""
import os
import re

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

LDS = {"mtr_k_seq_check": 0, "mtr_k_seq_members": 0, "mtr_k_seq_loci": 0, "mtr_k_seq_tasks": 0, "mtr_k_seq_dist": 0, "mtr_k_seq_split": 128 * 128}
INSTANCES = {"mtr_k_seq_dist": 4}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("sq"))


@pytest.mark.parametrize("stem", sorted(LDS))
def test_no_scratch_no_spills_the_declared_lds_and_four_wavefronts_per_simd(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == INSTANCES.get(stem, 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs, {k['group_segment_fixed_size']} bytes of LDS, {k['private_segment_fixed_size']} of scratch")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == LDS[stem], k
        assert k["vgpr_count"] <= 128, k


def test_the_kernels_are_the_ones_listed():
    src = open(os.path.join(os.path.dirname(LIB), "csrc", "seq_calls.hip.inc")).read()
    assert sorted(set(re.findall(r"__global__[^\n]*\bvoid (mtr_k_\w+)\(", src))) == sorted(LDS)
