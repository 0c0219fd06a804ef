"""The kernels of mtr_parse_fastq_device (mtr_amd/csrc/fastq.hip.inc) against the resources their launches assume (CPU; reads the gfx950
code object out of mtr_amd/libmtr_hip.so as tests/test_kernel_resources.py does): no scratch, no spills, four wavefronts per SIMD by
registers, at most 10 KB of LDS a workgroup."""
import os
import re

import pytest

from tests.test_kernel_resources import READELF, LIB, ROOT, _find, _kernels

# stem -> instances in the library: mtr_k_fastq_tile is one template with two modes (line table and stops, bases)
STEMS = {"mtr_k_fastq_lines": 1, "mtr_k_fastq_scan_lines": 1, "mtr_k_fastq_tile": 2, "mtr_k_fastq_records": 1, "mtr_k_fastq_finish": 1,
         "mtr_k_fastq_reads": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    if not os.path.exists(LIB):
        import mtr_amd.build
        mtr_amd.build.build()
    return _kernels(tmp_path_factory.mktemp("co"))


def test_every_kernel_of_the_file_is_listed():
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "fastq.hip.inc")).read()
    assert set(re.findall(r"__global__[^;{]*?\bvoid\s+(mtr_k_\w+)\s*\(", src)) == set(STEMS)


@pytest.mark.parametrize("stem", sorted(STEMS))
def test_fastq_kernels_have_no_scratch_and_fit_their_budget(kernels, stem):
    hits = _find(kernels, stem)
    assert len(hits) == STEMS[stem], (stem, sorted(kernels))
    for k in hits:
        assert k["private_segment_fixed_size"] == 0, k
        assert k.get("vgpr_spill_count", 0) == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 10240, k
