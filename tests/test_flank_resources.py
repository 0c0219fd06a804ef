"""The flank search's and the genotype's kernels (mtr_amd/csrc/flank_search.hip.inc, genotype.hip.inc) against the resources their launches assume
(CPU; reads the gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  Both instantiations of the scan are
built; the scan, the pack, the pairing and the output kernels take no scratch, spill nothing, use no LDS and at most 128 VGPRs (the host gives
the scan 16 wavefronts per CU).  The genotype aligns through the locus search's own kernels: it adds no DP kernel."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

KERNELS = ("mtr_k_flank_lanes", "mtr_k_flank_pack", "mtr_k_geno_pair", "mtr_k_geno_out")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def test_both_words_of_the_scan_are_built(kernels):
    names = [k["name"] for k in _find(kernels, "mtr_k_flank_lanes")]
    assert sorted(names) == sorted(f"_Z17mtr_k_flank_lanesI{w}Ev9FlankArgs" for w in ("j", "m")), names        # (unsigned int, unsigned long)


@pytest.mark.parametrize("stem", KERNELS)
def test_no_scratch_no_spills_no_lds_and_four_wavefronts_per_simd(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == (2 if stem == "mtr_k_flank_lanes" else 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == 0, k
        assert k["vgpr_count"] <= 128, k


def test_the_genotype_adds_no_dp_kernel(kernels):
    assert not [n for n in kernels if "geno" in n and ("lanes" in n or "waves" in n)]
    assert sorted(n for n in kernels if "mtr_k_geno" in n) == sorted(k["name"] for s in ("mtr_k_geno_pair", "mtr_k_geno_out") for k in _find(kernels, s))
