"""Reads in device memory (mtr_upload_batch_device, Engine.upload_device) on the CPU: the header declares the entry point, the
library exports it and refuses a null context, the Python argument checks refuse bad tensors and plans before the library is
called, and the packing kernel keeps to registers (no scratch, no spills)."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mtr_amd
from mtr_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-readelf", shutil.which("llvm-readelf")) if p and os.path.exists(p)), None)


@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return mtr_amd.load_library()


def test_header_declares_device_upload():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtr_hip.h")).read(), flags=re.S)
    assert re.search(r"^#define MTR_TEXT_ASCII 0\b", hdr, flags=re.M)
    assert re.search(r"^#define MTR_TEXT_CODES 1\b", hdr, flags=re.M)
    decl = re.search(r"mtr_status\s+mtr_upload_batch_device\s*\(([^)]*)\)", hdr)
    assert decl, "mtr_upload_batch_device is not declared"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 8 and "d_text" in args[1] and "text_kind" in args[6] and "wait_stream" in args[7], args


def test_library_exports_device_upload(lib):
    assert "mtr_upload_batch_device" in mtr_amd.EXPORTS
    assert hasattr(lib, "mtr_upload_batch_device")
    assert lib.mtr_abi_version() == 5


def test_null_context_is_bad_arg(lib):
    offs = np.zeros(1, np.int64)
    lens = np.full(1, 16, np.int32)
    st = lib.mtr_upload_batch_device(None, C.c_void_p(0x1000), 16, offs.ctypes.data, lens.ctypes.data, 1, mtr_amd.TEXT_ASCII, None)
    assert st == 2                                                          # MTR_ERR_BAD_ARG


# ---- the Python checks, made before the library is called ----------------------------------------------------------------
def _torch():
    return pytest.importorskip("torch")


def test_args_refuse_a_cpu_tensor():
    torch = _torch()
    text = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        mtr_amd.device_input_args(text, [0, 10], [10, 20], 0)


def test_args_refuse_a_wrong_dtype():
    torch = _torch()
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        mtr_amd.device_input_args(torch.zeros(64, dtype=torch.int32), [0], [10], 0)
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        mtr_amd.device_input_args(np.zeros(64, np.uint8), [0], [10], 0)


def test_args_refuse_a_non_contiguous_tensor():
    torch = _torch()
    with pytest.raises(mtr_amd.MtrError, match="contiguous"):
        mtr_amd.device_input_args(torch.zeros(128, dtype=torch.uint8)[::2], [0], [10], 0)
    with pytest.raises(mtr_amd.MtrError, match="1-D"):
        mtr_amd.device_input_args(torch.zeros(8, 8, dtype=torch.uint8), [0], [10], 0)


def test_args_refuse_offsets_and_lens_that_do_not_match():
    torch = _torch()
    text = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(mtr_amd.MtrError, match="same, non-zero length"):
        mtr_amd.device_input_args(text, [0, 10, 20], [10, 10], 0)
    with pytest.raises(mtr_amd.MtrError, match="same, non-zero length"):
        mtr_amd.device_input_args(text, [], [], 0)
    with pytest.raises(mtr_amd.MtrError, match="integer"):
        mtr_amd.device_input_args(text, [0.5], [10], 0)
    with pytest.raises(mtr_amd.MtrError, match="read 1: length 0"):
        mtr_amd.device_input_args(text, [0, 10], [10, 0], 0)


def test_args_refuse_a_read_past_the_end_of_the_text():
    torch = _torch()
    text = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(mtr_amd.MtrError, match="read 1: bytes 60 .. \\+5 outside the text of 64 bytes"):
        mtr_amd.device_input_args(text, np.array([0, 60]), np.array([10, 5]), 0)
    with pytest.raises(mtr_amd.MtrError, match="read 0: bytes -1"):
        mtr_amd.device_input_args(text, torch.tensor([-1]), torch.tensor([5]), 0)


def test_args_accept_cpu_tensors_and_numpy_as_the_plan():
    """offsets / lens may be numpy arrays or CPU tensors of any integer type: converted to int64 / int32 (the text check comes last)"""
    torch = _torch()
    text = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):           # the plan passed; only the CPU text is refused
        mtr_amd.device_input_args(text, torch.tensor([0, 32], dtype=torch.int32), np.array([32, 32], np.int64), 0)
    assert mtr_amd._host_ints(torch.tensor([0, 32]), np.int64, "offsets").dtype == np.int64
    assert mtr_amd._host_ints(np.array([1, 2], np.int64), np.int32, "lens").dtype == np.int32
    with pytest.raises(mtr_amd.MtrError, match="does not fit int32"):
        mtr_amd._host_ints(np.array([1 << 40]), np.int32, "lens")


# ---- the packing kernel's resources (read as tests/test_kernel_resources.py reads them) --------------------------------------
def _code_object(tmp_path):
    blob = open(mbuild.LIB, "rb").read()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert at >= 0, "no offload bundle in libmtr_hip.so"
    n = struct.unpack_from("<Q", blob, at + 24)[0]
    p = at + 32
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", blob, p)
        p += 24
        triple = blob[p:p + tl].decode()
        p += tl
        if "gfx950" in triple:
            out = tmp_path / "mtr_gfx950.co"
            out.write_bytes(blob[at + off:at + off + size])
            return str(out)
    raise AssertionError("no gfx950 code object in libmtr_hip.so")


def _kernels(co):
    txt = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, {}
    for line in txt.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip("'\"")
        if key in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "name"):
            if key in cur:
                if "name" in cur:
                    out[cur["name"]] = cur
                cur = {}
            cur[key] = val if key == "name" else int(val)
    if "name" in cur:
        out[cur["name"]] = cur
    return out


def test_pack_kernel_uses_no_scratch_and_no_lds(lib, tmp_path):
    if READELF is None:
        pytest.skip("llvm-readelf not found")
    stem = "mtr_k_pack_text"
    hits = [v for k, v in _kernels(_code_object(tmp_path)).items() if k.startswith(f"_Z{len(stem)}{stem}")]
    assert len(hits) == 2, hits                                             # the ASCII and the codes kernel
    for k in hits:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
        assert k["group_segment_fixed_size"] == 0, k
