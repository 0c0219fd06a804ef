"""The kernels of the partial genotype at catalogue scale (mtr_amd/csrc/partial_catalog.hip.inc) against the resources their launches assume (CPU;
reads the gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  Both instantiations of the candidates' flank
scan and all four buckets of the per-lane-motif extension are built; no kernel takes scratch or spills, none declares LDS; each stays within 128
VGPRs (four wavefronts per SIMD), the extension's bucket of 32 - three arrays of 32 registers before any temporary - within 256 (two)."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

KERNELS = ("mtr_k_ptc_cands", "mtr_k_ptc_tasks", "mtr_k_ptc_flank", "mtr_k_ptc_pair", "mtr_k_ptc_ext", "mtr_k_ptc_out")
COUNT = {"mtr_k_ptc_flank": 2, "mtr_k_ptc_ext": 4}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def _bucket(k):
    return int(k["name"].split("mtr_k_ptc_extILi")[1].split("E")[0])


def test_both_words_of_the_flank_scan_and_all_four_buckets_of_the_extension_are_built(kernels):
    names = [k["name"] for k in _find(kernels, "mtr_k_ptc_flank")]
    assert sorted(names) == sorted(f"_Z15mtr_k_ptc_flankI{w}Ev12PtcFlankArgs" for w in ("j", "m")), names        # (unsigned int, unsigned long)
    names = [k["name"] for k in _find(kernels, "mtr_k_ptc_ext")]
    assert sorted(names) == sorted(f"_Z13mtr_k_ptc_extILi{ub}EEv10PtcExtArgs" for ub in (4, 8, 16, 32)), names


@pytest.mark.parametrize("stem", KERNELS)
def test_no_scratch_no_spills_no_lds_and_the_register_bounds(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == COUNT.get(stem, 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == 0, k
        assert k["vgpr_count"] <= (256 if stem == "mtr_k_ptc_ext" and _bucket(k) == 32 else 128), k


def test_these_are_all_the_kernels_of_the_call(kernels):
    assert sorted(n for n in kernels if "mtr_k_ptc_" in n) == sorted(k["name"] for s in KERNELS for k in _find(kernels, s))
    assert not [n for n in kernels if "Ptc" in n and "mtr_k_ptc_" not in n]
