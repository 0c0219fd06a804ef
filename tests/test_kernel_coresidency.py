"""What DESIGN.md 4.11 kept of the co-residency work, read out of the built gfx950 code object (CPU; like tests/test_kernel_resources.py).

For a DP wavefront (128 VGPRs) to run beside the sixteen wavefronts per CU of a latency-bound kernel of another batch, that kernel must leave it 128 registers per
SIMD (at most 96 allocated) AND LDS: the chip hands LDS out in granules of 1 280 bytes (profiles/coresidency_probe.md), so a kernel of 10 080 bytes takes eight
granules, sixteen such wavefronts take the CU's 128, and only arena kernels of at most seven granules (8 960 bytes) leave room.

KEPT, and asserted here:   the register bound of mtr_k_walks and mtr_k_polish; mtr_k_revise_quads with only the LDS it uses; the DP kernels' side of the sum rule.
LEFT OUT, and not asserted: mtr_k_walks_k (112 allocated VGPRs) and mtr_k1_ranges (112): no register work was done on them, because the probe showed that registers are
                            not what keeps the DP wavefronts out; the arena kernels' side of the sum rule (sixteen wavefronts of SEVEN granules), which needs 1 120 bytes
                            out of an arena whose k-mer table alone is 8 192."""
import pytest

from tests.test_kernel_resources import LDS_PER_CU, _find, kernels  # noqa: F401  (the fixture)

LDS_GRANULE = 1280                    # measured: profiles/coresidency_probe.md
LATENCY_BOUND_KEPT = ["mtr_k_walks", "mtr_k_polish"]
LATENCY_BOUND_LEFT_OUT = ["mtr_k_walks_k", "mtr_k1_ranges"]
DP_KERNELS = ["mtr_k_dp2_quads", "mtr_k_revise_quads"]
PARENT_SPILLS = {"mtr_k_dp2_quads": 26, "mtr_k_revise_quads": 33}


def _alloc(n, granule):
    return -(-n // granule) * granule


@pytest.mark.parametrize("stem", LATENCY_BOUND_KEPT)
def test_latency_bound_kernels_leave_a_dp_wavefront_its_registers(kernels, stem):
    """four of them per SIMD leave 128 of the 512 registers: at most 96 allocated (the allocation granule is 8)"""
    for k in _find(kernels, stem):
        assert _alloc(k["vgpr_count"], 8) <= 96, k


@pytest.mark.parametrize("stem", DP_KERNELS)
def test_dp_kernels_take_only_the_lds_they_use(kernels, stem):
    for k in _find(kernels, stem):
        assert k["group_segment_fixed_size"] <= 2048, k


def test_sum_rule_on_the_dp_kernels_side(kernels):
    """four wavefronts of the largest DP kernel fit beside sixteen arena wavefronts of seven granules each"""
    largest = max(k["group_segment_fixed_size"] for stem in DP_KERNELS for k in _find(kernels, stem))
    assert 16 * 7 * LDS_GRANULE + 4 * _alloc(largest, LDS_GRANULE) <= LDS_PER_CU, largest


def test_the_kernels_left_out_are_still_the_ones_named(kernels):
    """the day one of them fits (96 registers, seven granules of LDS) it moves to the kept list and this file's header changes with DESIGN.md 4.11"""
    for stem in LATENCY_BOUND_LEFT_OUT + LATENCY_BOUND_KEPT:
        for k in _find(kernels, stem):
            assert k["group_segment_fixed_size"] <= LDS_PER_CU // 16, k        # sixteen of its own per CU, as before
            assert _alloc(k["vgpr_count"], 8) <= 128, k


def test_no_more_scratch_and_spills_than_the_parent(kernels):
    for k in _find(kernels, "mtr_k1_ranges"):
        assert k["private_segment_fixed_size"] <= 120, k
    for stem, limit in PARENT_SPILLS.items():
        for k in _find(kernels, stem):
            assert k["vgpr_spill_count"] <= limit, k
