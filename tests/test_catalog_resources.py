"""The catalogue genotype's kernels (mtr_amd/csrc/catalog.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code object
out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  Both instantiations of the candidates' flank scan are built; no kernel
takes scratch or spills, none declares LDS - the filter and the table are read through the caches - and each stays within 128 VGPRs.  The
catalogue aligns through the locus search's own kernels: it adds no DP kernel.  mtr_k_cat_rows_check is the allele calls' check of a row list."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

KERNELS = ("mtr_k_cat_scan", "mtr_k_cat_cands", "mtr_k_cat_flank", "mtr_k_cat_pair", "mtr_k_cat_out", "mtr_k_cat_rows_check")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def test_both_words_of_the_flank_scan_are_built(kernels):
    names = [k["name"] for k in _find(kernels, "mtr_k_cat_flank")]
    assert sorted(names) == sorted(f"_Z15mtr_k_cat_flankI{w}Ev12CatFlankArgs" for w in ("j", "m")), names        # (unsigned int, unsigned long)


@pytest.mark.parametrize("stem", KERNELS)
def test_no_scratch_no_spills_no_lds_and_at_most_128_vgprs(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == (2 if stem == "mtr_k_cat_flank" else 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == 0, k                     # no kernel of the catalogue declares LDS
        assert k["vgpr_count"] <= 128, k


def test_these_are_all_the_catalogue_kernels_and_none_is_a_dp_kernel(kernels):
    assert sorted(n for n in kernels if "mtr_k_cat_" in n) == sorted(k["name"] for s in KERNELS for k in _find(kernels, s))
    assert not [n for n in kernels if "mtr_k_cat_" in n and ("lanes" in n or "waves" in n)]
