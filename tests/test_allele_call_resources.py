"""The allele calls' kernels (mtr_amd/csrc/allele_call.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code object
out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  No kernel takes scratch or spills; LDS appears in the two kernels that
declare it, at exactly the declared size - the rank's chunk of AL_TILE = 256 keys of 8 bytes, the split's two int64 per wavefront of its
workgroup of 256 lanes; every kernel stays within 128 VGPRs (workgroups of 256 lanes, launched without a bound on the wavefronts per CU: four
wavefronts per SIMD at the least); and the file's kernels are exactly the five listed."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

LDS = {"mtr_k_allele_count": 0, "mtr_k_allele_offsets": 0, "mtr_k_allele_fill": 0, "mtr_k_allele_rank": 256 * 8, "mtr_k_allele_split": (256 // 64) * 2 * 8}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", sorted(LDS))
def test_no_scratch_no_spills_the_declared_lds_and_four_wavefronts_per_simd(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == 1, (stem, found)
    k = found[0]
    print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs, {k['group_segment_fixed_size']} bytes of LDS")
    assert k["private_segment_fixed_size"] == 0, k
    assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
    assert k["group_segment_fixed_size"] == LDS[stem], k
    assert k["vgpr_count"] <= 128, k


def test_the_kernels_are_the_five_listed(kernels):
    src = open(os.path.join(os.path.dirname(LIB), "csrc", "allele_call.hip.inc")).read()
    import re
    assert sorted(re.findall(r"__global__[^\n]*\bvoid (mtr_k_\w+)\(", src)) == sorted(LDS)
    assert sorted(n for n in kernels if "mtr_k_allele" in n) == sorted(k["name"] for s in LDS for k in _find(kernels, s))
    assert not [n for n in kernels if "allele" in n and "geno" in n]
