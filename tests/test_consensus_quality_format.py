"""The qualities' entries on the CPU (no library call that needs a GPU): include/mtr_hip.h declares them and its defines are the Python mirror's
and the shared header's, MTR_ABI_VERSION stays 5, the library exports them, Engine's new keywords are trailing ones, and join_window_qualities
does what its docstring says."""
import inspect
import os
import re

import numpy as np
import pytest

import mtr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
ENTRIES = ("mtr_keep_qualities", "mtr_attach_qualities_device", "mtr_qualities_resident", "mtr_extract_window_qualities_device", "mtr_allele_consensus_quality_device")


def _define(text, name):
    m = re.search(rf"^#define {name}\s+(.+?)\s*(?://.*)?$", text, re.M)
    assert m, name
    return m.group(1)


def test_the_header_declares_the_entries_and_the_abi_version_stays():
    assert _define(HEADER, "MTR_ABI_VERSION") == "5"
    for name in ENTRIES:
        assert re.search(rf"^mtr_status {name}\(", HEADER, re.M), name
        assert name in mtr_amd.EXPORTS
    assert "the qualities as output are not supported" not in HEADER
    assert '"quality-weighted allele consensus"' in open(os.path.join(ROOT, "mtr_amd", "csrc", "banded_align.h")).read()


def test_the_defines_are_the_mirrors():
    assert int(_define(HEADER, "MTR_QUAL_MAX")) == mtr_amd.QUAL_MAX == 93 and int(_define(HEADER, "MTR_CONSQ_MAX_CAP")) == mtr_amd.CONSQ_MAX_CAP == 93
    shared = open(os.path.join(ROOT, "mtr_amd", "csrc", "banded_align.h")).read()
    assert int(_define(shared, "BAQ_MAX_CAP")) == mtr_amd.CONSQ_MAX_CAP
    assert _define(shared, "BAQ_TAB") == "(BA_TAB + BA_INS_SLOTS)" and _define(shared, "BA_TAB") == "(4 + 1 + 4 * BA_INS_SLOTS)"      # 25 and 21 int32 a position
    assert int(_define(open(os.path.join(ROOT, "mtr_amd", "csrc", "quality.hip.inc")).read(), "QL_MAX")) == mtr_amd.QUAL_MAX


def test_the_library_exports_the_entries():
    lib = mtr_amd.load_library()
    assert lib.mtr_abi_version() == 5
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_the_new_keywords_are_trailing_and_off_by_default():
    up = inspect.signature(mtr_amd.Engine.upload_fastq_device).parameters
    assert list(up)[1:] == ["buf", "file_state", "more", "keep_quality"] and up["keep_quality"].default is False
    walk = inspect.signature(mtr_amd.Engine.walk_fastq_device).parameters
    assert list(walk)[1:] == ["buf", "window_bytes", "file_state", "keep_quality"] and walk["keep_quality"].default is False
    cq = inspect.signature(mtr_amd.Engine.allele_consensus_quality).parameters
    assert list(cq)[1:] == ["sg", "windows", "qual", "calls", "band_extra", "qual_cap"] and (cq["band_extra"].default, cq["qual_cap"].default) == (16, 40)
    assert mtr_amd.GenotypeWindows._fields == ("off", "bases")


def test_join_window_qualities_concatenates_and_checks_the_lengths():
    parts = [np.array([1, 2, 3], np.uint8), np.zeros(0, np.uint8), np.array([9], np.uint8)]
    wins = [mtr_amd.GenotypeWindows(np.array([0, 2, 3], np.int64), np.zeros(3, np.uint8)), mtr_amd.GenotypeWindows(np.array([0], np.int64), np.zeros(0, np.uint8)),
            mtr_amd.GenotypeWindows(np.array([0, 1], np.int64), np.zeros(1, np.uint8))]
    joined = mtr_amd.join_windows(wins)
    got = mtr_amd.join_window_qualities(parts, joined)
    assert got.dtype == np.uint8 and got.tolist() == [1, 2, 3, 9] and mtr_amd.join_window_qualities(parts).tolist() == [1, 2, 3, 9]
    torch = pytest.importorskip("torch")
    assert torch.equal(mtr_amd.join_window_qualities([torch.from_numpy(p) for p in parts]), torch.tensor([1, 2, 3, 9], dtype=torch.uint8))
    with pytest.raises(mtr_amd.MtrError, match="3 qualities for windows of 4 bases"):
        mtr_amd.join_window_qualities(parts[:2], joined)
    with pytest.raises(mtr_amd.MtrError, match="nothing to join"):
        mtr_amd.join_window_qualities([])
