"""The partial genotype's kernels (mtr_amd/csrc/partial.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code object
out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does).  All four buckets of the extension are built; every kernel takes no
scratch, spills nothing and uses no LDS; the pairing, the output kernel and the buckets up to 16 stay within 128 VGPRs (four wavefronts per
SIMD), the bucket of 32 - three arrays of 32 registers before any temporary - within 256 (two)."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, _find, _kernels

KERNELS = ("mtr_k_partial_pair", "mtr_k_ext_lanes", "mtr_k_partial_out")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def _bucket(k):
    return int(k["name"].split("mtr_k_ext_lanesILi")[1].split("E")[0])


def test_all_four_buckets_of_the_extension_are_built(kernels):
    names = [k["name"] for k in _find(kernels, "mtr_k_ext_lanes")]
    assert sorted(names) == sorted(f"_Z15mtr_k_ext_lanesILi{ub}EEv14PartialExtArgs" for ub in (4, 8, 16, 32)), names


@pytest.mark.parametrize("stem", KERNELS)
def test_no_scratch_no_spills_no_lds_and_the_register_bounds(kernels, stem):
    found = _find(kernels, stem)
    assert len(found) == (4 if stem == "mtr_k_ext_lanes" else 1), (stem, found)
    for k in found:
        print(f"{k['name']}: {k['vgpr_count']} VGPRs, {k.get('sgpr_count')} SGPRs")
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k["group_segment_fixed_size"] == 0, k
        assert k["vgpr_count"] <= (256 if stem == "mtr_k_ext_lanes" and _bucket(k) == 32 else 128), k


def test_the_partial_genotype_adds_exactly_these_kernels(kernels):
    ours = sorted(n for n in kernels if "partial" in n or "ext_lanes" in n)
    assert ours == sorted(k["name"] for s in KERNELS for k in _find(kernels, s)), ours
