"""A FASTA file in device memory (mtr_parse_fasta_device / mtr_upload_fasta_device / mtr_fasta_index, Engine.parse_fasta_device /
upload_fasta_device) on the CPU: the header declares the entry points and keeps its ABI version, the library exports them and
refuses a null context, the Python mirror's structures have the header's layout, and the argument checks refuse bad tensors before
the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
from mtr_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mtr_parse_fasta_device", "mtr_upload_fasta_device", "mtr_fasta_index")


@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return mtr_amd.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtr_hip.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_and_keeps_its_version():
    hdr = _header()
    assert re.search(r"^#define MTR_ABI_VERSION 5\b", hdr, flags=re.M)
    for k, name in enumerate(("EOF", "EMPTY", "BADCHAR", "TOOLONG")):
        assert re.search(rf"^#define MTR_FASTA_END_{name} {k}\b", hdr, flags=re.M), name
    args = {name: [a.strip() for a in re.search(rf"mtr_status\s+{name}\s*\(([^)]*)\)", hdr).group(1).split(",")] for name in NAMES}
    assert [a.split()[-1].lstrip("*") for a in args["mtr_parse_fasta_device"]] == ["ctx", "d_fasta", "n_bytes", "wait_stream", "dst", "info"]
    assert [a.split()[-1].lstrip("*") for a in args["mtr_upload_fasta_device"]] == ["ctx", "d_fasta", "n_bytes", "wait_stream", "info"]
    assert [a.split()[-1].lstrip("*") for a in args["mtr_fasta_index"]] == ["ctx", "lens", "id_off", "ids"]
    info = re.search(r"typedef struct mtr_fasta_info \{(.*?)\} mtr_fasta_info;", hdr, re.S).group(1)
    assert re.sub(r"\s+", " ", info).strip() == "int32_t n_reads, end, bad_char, reserved; int64_t end_pos, n_bases, id_bytes;"
    dst = re.search(r"typedef struct mtr_fasta_dst \{(.*?)\} mtr_fasta_dst;", hdr, re.S).group(1)
    assert re.findall(r"(\w+)\s*[;,]", dst) == ["text", "offsets", "lens", "ids", "id_off", "cap_text", "cap_reads", "cap_id_bytes"]


def test_the_mirror_has_the_headers_layout():
    assert set(NAMES) <= set(mtr_amd.EXPORTS)
    assert [f[0] for f in mtr_amd.CFastaInfo._fields_] == ["n_reads", "end", "bad_char", "reserved", "end_pos", "n_bases", "id_bytes"]
    assert C.sizeof(mtr_amd.CFastaInfo) == 40 and mtr_amd.CFastaInfo.end_pos.offset == 16
    assert [f[0] for f in mtr_amd.CFastaDst._fields_] == ["text", "offsets", "lens", "ids", "id_off", "cap_text", "cap_reads", "cap_id_bytes"]
    assert C.sizeof(mtr_amd.CFastaDst) == 64
    assert mtr_amd.Fasta._fields == ("text", "offsets", "lens", "ids", "end", "bad_char", "end_pos")
    assert mtr_amd.FASTA_END == {0: "eof", 1: "empty", 2: "bad", 3: "toolong"}
    src = open(os.path.join(ROOT, "mtr_amd", "csrc", "fasta.hip.inc")).read()
    assert re.search(rf"^#define MTR_FASTA_TILE_BYTES {mtr_amd.FASTA_TILE_BYTES}\b", src, flags=re.M)


def test_library_exports_the_entry_points(lib):
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.mtr_abi_version() == 5


def test_null_context_is_bad_arg(lib):
    info = mtr_amd.CFastaInfo()
    assert lib.mtr_parse_fasta_device(None, C.c_void_p(0x1000), 16, None, None, C.byref(info)) == 2      # MTR_ERR_BAD_ARG
    assert lib.mtr_upload_fasta_device(None, C.c_void_p(0x1000), 16, None, C.byref(info)) == 2
    assert lib.mtr_fasta_index(None, None, None, None) == 2


# ---- the Python checks, made before the library is called ----------------------------------------------------------------
def _torch():
    return pytest.importorskip("torch")


def _engine_without_a_library():
    e = mtr_amd.Engine.__new__(mtr_amd.Engine)                  # no context: the checks must raise before anything is called
    e.h, e.lib, e.device = None, None, 0
    return e


@pytest.mark.parametrize("method", ["parse_fasta_device", "upload_fasta_device"])
def test_methods_refuse_bad_buffers_before_the_library_is_called(method):
    torch = _torch()
    call = getattr(_engine_without_a_library(), method)
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        call(np.zeros(64, np.uint8))
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        call(b">r\nACGT\n")
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        call(torch.zeros(64, dtype=torch.int8))
    with pytest.raises(mtr_amd.MtrError, match="contiguous"):
        call(torch.zeros(128, dtype=torch.uint8)[::2])
    with pytest.raises(mtr_amd.MtrError, match="1-D"):
        call(torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        call(torch.zeros(64, dtype=torch.uint8))


def test_args_refuse_a_tensor_on_another_device():
    torch = _torch()
    meta = torch.empty(64, dtype=torch.uint8, device="meta")
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor, got a tensor on meta"):
        mtr_amd.fasta_input_args(meta, 0)

    class OnGpu1:                                                # what the device check looks at, without a second GPU
        type, index = "cuda", 1

        def __str__(self):
            return "cuda:1"

    class Buf(torch.Tensor):
        device = OnGpu1()

    buf = torch.zeros(64, dtype=torch.uint8).as_subclass(Buf)
    with pytest.raises(mtr_amd.MtrError, match="buf is on cuda:1, the engine on cuda:0"):
        mtr_amd.fasta_input_args(buf, 0)
