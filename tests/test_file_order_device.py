"""File-order mode for reads in device memory (mtr_upload_batch_device_in_file, mtr_upload_fasta_device_in_file,
mtr_file_state_skip_device, mtr_test_file_tail) on the CPU: the headers declare the entry points, EXPORTS names them, the library
exports them at ABI 5 and refuses null arguments, and the Python argument checks refuse bad tensors before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtr_amd
from mtr_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtr_upload_batch_device_in_file", "mtr_upload_fasta_device_in_file", "mtr_file_state_skip_device", "mtr_test_file_tail"]
BAD_ARG = 2


@pytest.fixture(scope="module")
def lib():
    mbuild.build()
    return mtr_amd.load_library()


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _args(hdr, fn):
    decl = re.search(r"mtr_status\s+" + fn + r"\s*\(([^)]*)\)", hdr)
    assert decl, f"{fn} is not declared"
    return [a.strip() for a in decl.group(1).split(",")]


def test_headers_declare_the_entry_points():
    hdr = _header("mtr_hip.h")
    for fn in ("mtr_upload_batch_device_in_file", "mtr_file_state_skip_device"):
        a = _args(hdr, fn)
        assert len(a) == 9 and "mtr_ctx" in a[0] and "mtr_file_state" in a[1] and "d_text" in a[2] and "text_kind" in a[7] and "wait_stream" in a[8], a
    a = _args(hdr, "mtr_upload_fasta_device_in_file")
    assert len(a) == 6 and "mtr_file_state" in a[1] and "d_fasta" in a[2] and "wait_stream" in a[4] and "mtr_fasta_info" in a[5], a
    a = _args(_header("mtr_hip_test.h"), "mtr_test_file_tail")
    assert len(a) == 4 and "uint16_t **" in a[1] and "int64_t **" in a[2] and "uint8_t **" in a[3], a
    assert re.search(r"^#define MTR_ABI_VERSION 5\b", hdr, flags=re.M)
    # the sentences that said the device path had no file-order mode are gone
    full = open(os.path.join(ROOT, "include", "mtr_hip.h")).read()
    assert "no device variant" not in full and "no FASTA variant" not in full


def test_library_exports_the_entry_points(lib):
    for fn in NEW:
        assert fn in mtr_amd.EXPORTS, fn
        assert hasattr(lib, fn), fn
        assert getattr(lib, fn).argtypes is not None, fn
    assert lib.mtr_abi_version() == 5


def test_null_arguments_are_bad_arg(lib):
    offs, lens = np.zeros(1, np.int64), np.full(1, 16, np.int32)
    fs = mtr_amd.FileState()
    info = mtr_amd.CFastaInfo()
    text = C.c_void_p(0x1000)
    assert lib.mtr_upload_batch_device_in_file(None, fs.h, text, 16, offs.ctypes.data, lens.ctypes.data, 1, mtr_amd.TEXT_ASCII, None) == BAD_ARG
    assert lib.mtr_upload_batch_device_in_file(None, None, text, 16, offs.ctypes.data, lens.ctypes.data, 1, mtr_amd.TEXT_ASCII, None) == BAD_ARG
    assert lib.mtr_file_state_skip_device(None, fs.h, text, 16, offs.ctypes.data, lens.ctypes.data, 1, mtr_amd.TEXT_ASCII, None) == BAD_ARG
    assert lib.mtr_upload_fasta_device_in_file(None, fs.h, text, 16, None, C.byref(info)) == BAD_ARG
    assert lib.mtr_upload_fasta_device_in_file(None, None, text, 16, None, C.byref(info)) == BAD_ARG
    tl, to, af = C.POINTER(C.c_uint16)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_uint8)()
    assert lib.mtr_test_file_tail(None, C.byref(tl), C.byref(to), C.byref(af)) == BAD_ARG
    fs.close()


def test_the_keyword_and_the_methods_exist():
    import inspect
    for fn in (mtr_amd.Engine.upload_device, mtr_amd.Engine.process_device, mtr_amd.Engine.upload_fasta_device):
        p = inspect.signature(fn).parameters
        assert "file_state" in p and p["file_state"].default is None, fn
    assert list(inspect.signature(mtr_amd.FileState.skip_device).parameters) == ["self", "engine", "text", "offsets", "lens", "codes"]
    assert inspect.signature(mtr_amd.FileState.skip_device).parameters["codes"].default is False
    assert callable(mtr_amd.Engine.test_file_tail)


# ---- the Python checks, made before the library is called: an engine that has no context behind it would crash in the library ------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _engine_without_context():
    e = object.__new__(mtr_amd.Engine)
    e.lib, e.h, e.device, e.n_reads = _NoLibrary(), None, 0, 0
    return e


def _state_without_library():
    fs = object.__new__(mtr_amd.FileState)
    fs.lib, fs.h = _NoLibrary(), None
    return fs


def test_upload_device_in_file_refuses_bad_text_before_the_library():
    torch = pytest.importorskip("torch")
    e, fs = _engine_without_context(), _state_without_library()
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):           # text not on the engine's device
        e.upload_device(torch.zeros(64, dtype=torch.uint8), [0, 10], [10, 20], file_state=fs)
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        e.upload_device(torch.zeros(64, dtype=torch.int32), [0], [10], file_state=fs)
    with pytest.raises(mtr_amd.MtrError, match="torch.Tensor"):
        e.process_device(np.zeros(64, np.uint8), [0], [10], file_state=fs)
    with pytest.raises(mtr_amd.MtrError, match="read 1: bytes 60"):
        e.upload_device(torch.zeros(64, dtype=torch.uint8), [0, 60], [10, 5], codes=True, file_state=fs)


def test_skip_device_refuses_bad_text_before_the_library():
    torch = pytest.importorskip("torch")
    e, fs = _engine_without_context(), _state_without_library()
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        fs.skip_device(e, torch.zeros(64, dtype=torch.uint8), [0], [10])
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        fs.skip_device(e, torch.zeros(64, dtype=torch.float32), [0], [10])
    with pytest.raises(mtr_amd.MtrError, match="same, non-zero length"):
        fs.skip_device(e, torch.zeros(64, dtype=torch.uint8), [0, 1], [10])


def test_upload_fasta_device_in_file_refuses_a_bad_buffer_before_the_library():
    torch = pytest.importorskip("torch")
    e, fs = _engine_without_context(), _state_without_library()
    with pytest.raises(mtr_amd.MtrError, match="GPU tensor"):
        e.upload_fasta_device(torch.zeros(64, dtype=torch.uint8), fs)
    with pytest.raises(mtr_amd.MtrError, match="torch.uint8"):
        e.upload_fasta_device(torch.zeros(64, dtype=torch.int8), file_state=fs)
