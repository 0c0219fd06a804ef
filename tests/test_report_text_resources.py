"""The kernels of mtr_report_text_device (mtr_amd/csrc/report_text.hip.inc) against the resources their launches assume (CPU; reads
the gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does): no scratch, no spills, four wavefronts per
SIMD by registers, sixteen workgroups per CU by LDS."""
import os

import pytest

from tests.test_kernel_resources import READELF, LIB, _find, _kernels

# stem -> instances in the library: the size pass and the writing pass are the two instances of one template
STEMS = {"mtr_k_text_lines": 2, "mtr_k_text_rows": 2, "mtr_k_text_align": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", sorted(STEMS))
def test_report_text_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    hits = _find(kernels, stem)
    assert len(hits) == STEMS[stem], (stem, sorted(kernels))
    for k in hits:
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 10240, k
