"""The motif catalogue's kernels (mtr_amd/csrc/report_motif.hip.inc) against the resources their launches assume (CPU; reads the gfx950
code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does): no scratch, no spills, the budget of the report kernels
(tests/test_report_resources.py).  The two kernels that run unit_motif() stage sixteen units of 512 bytes in LDS."""
import pytest

from tests.test_kernel_resources import READELF, LIB, _find, _kernels

STEMS = ["mtr_k_unit_motif", "mtr_k_unit_motif_rows", "mtr_k_motif_insert", "mtr_k_motif_leader", "mtr_k_motif_groups"]


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
def test_motif_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    found = _find(kernels, stem)
    assert found, stem
    for k in found:
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 10240, k


def test_the_staging_kernels_use_the_lds_they_are_written_for(kernels):
    for stem in ("mtr_k_unit_motif", "mtr_k_unit_motif_rows"):
        assert all(k["group_segment_fixed_size"] == 16 * 512 for k in _find(kernels, stem)), stem
