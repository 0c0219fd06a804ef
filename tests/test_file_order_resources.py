"""The kernels of file-order mode for device input (mtr_amd/csrc/file_order.hip.inc) against the resources of the service kernels
(CPU; reads the gfx950 code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does): no scratch, no spills, at
most 128 VGPRs, no LDS (a binary search over global arrays needs none)."""
import os
import re

import pytest

from tests.test_kernel_resources import READELF, LIB, ROOT, _find, _kernels

# stem -> instances in the library
STEMS = {"mtr_k_file_tail": 1, "mtr_k_file_after": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def test_every_kernel_of_the_file_is_listed():
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "file_order.hip.inc")).read()
    assert set(re.findall(r"__global__[^;{]*?\bvoid\s+(mtr_k_\w+)\s*\(", src)) == set(STEMS)


@pytest.mark.parametrize("stem", sorted(STEMS))
def test_file_order_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    hits = _find(kernels, stem)
    assert len(hits) == STEMS[stem], (stem, sorted(kernels))
    for k in hits:
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] == 0, k
