"""The report kernels (mtr_amd/csrc/chain.hip.inc) against the resources their launches assume (CPU; reads the gfx950 code object
out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does): one 64-lane workgroup per read, no scratch, no spills."""
import pytest

from tests.test_kernel_resources import READELF, LIB, _find, _kernels

STEMS = ["mtr_k_chain", "mtr_k_chain_sets", "mtr_k_report_pack"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    import os
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", STEMS)
def test_report_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    for k in _find(kernels, stem):
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 10240, k
