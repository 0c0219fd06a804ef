"""The qualities' and the weighted consensus' kernels (mtr_amd/csrc/quality.hip.inc, consensus_quality.hip.inc) against the resources their launches
assume (CPU; reads the gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_consensus_resources.py does).  No kernel spills and none
takes private scratch memory; LDS appears only in the emission, at exactly the declared size (one int32 per wavefront of its workgroup of 256
lanes); every kernel stays within 128 VGPRs; both alignments and both emissions are instantiated, as both gathers are; and the files' kernels
are exactly the ones listed."""
import os
import re

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

LDS = {"mtr_k_qual_gather": 0, "mtr_k_win_qual": 0, "mtr_k_cq_align": 0, "mtr_k_cq_emit": (256 // 64) * 4}
INSTANCES = {"mtr_k_qual_gather": 2, "mtr_k_cq_align": 2, "mtr_k_cq_emit": 2}
FILES = {"quality.hip.inc": ["mtr_k_qual_gather", "mtr_k_win_qual"], "consensus_quality.hip.inc": ["mtr_k_cq_align", "mtr_k_cq_emit"]}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("cq"))


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


@pytest.mark.parametrize("name", sorted(FILES))
def test_the_kernels_are_the_ones_listed(name):
    src = open(os.path.join(os.path.dirname(LIB), "csrc", name)).read()
    assert sorted(set(re.findall(r"__global__[^\n]*\bvoid (mtr_k_\w+)\(", src))) == sorted(FILES[name])
