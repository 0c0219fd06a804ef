"""The kernels of mtr_report_alignments_device (mtr_amd/csrc/report_align.hip.inc) against the resources their launches assume (CPU; reads
the gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does): no scratch, no spills, four wavefronts per
SIMD by registers, sixteen workgroups per CU by LDS."""
import os

import pytest

from tests.test_kernel_resources import READELF, LIB, _find, _kernels

STEMS = ["mtr_k_align_sizes", "mtr_k_scan_offsets", "mtr_k_align_tasks", "mtr_k_align_render"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


@pytest.mark.parametrize("stem", STEMS)
def test_report_alignment_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    hits = _find(kernels, stem) if stem != "mtr_k_scan_offsets" else [v for k, v in kernels.items() if "mtr_k_scan_offsets" in k]
    assert len(hits) >= (2 if stem == "mtr_k_scan_offsets" else 1), (stem, sorted(kernels))      # the scan: its int32 and int64 instances
    for k in hits:
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 10240, k
