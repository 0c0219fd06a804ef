"""mtr_amd.format_report against the command line's own formatting (CPU): report lines built from canned Report columns must be
what mtr_amd/host/print.c prints for the same records, the ratio text coming from mtrh_format_ratio in libmtr_host.so."""
import ctypes as C
import os

import numpy as np

import mtr_amd
from tests import host_util as hu

# (rep_start, rep_end, repeat_len, period, copies, matches, mismatches, insertions, deletions, unit); 0-origin positions
CANNED = [
    (0, 29, 30, 3, 10, 30, 0, 0, 0, "ACG"),
    (5, 24, 20, 2, 10, 13, 3, 2, 2, "AT"),
    (10, 16, 7, 1, 7, 1, 6, 0, 0, "T"),                 # 1 / 7 = 0.142857 14...: rounds at the sixth decimal
    (3, 41, 39, 13, 3, 2, 30, 4, 3, "ACGTACGTACGTA"),   # 2 / 39
    (100, 9999, 9900, 4, 2475, 8191, 1000, 500, 209, "GATC"),
    (7, 7, 0, 0, 0, 5, 0, 0, 0, ""),                    # repeat_len 0: inf
    (7, 7, 0, 0, 0, 0, 0, 0, 0, ""),                    # 0 / 0: nan
    (0, 999, 1000, 500, 2, 998, 1, 1, 0, "ACGT" * 125),  # period 500
    (12, 70, 59, 5, 11, 51, 6, 1, 1, "CCATG"),
    (1, 2000, 2000, 7, 285, 1999, 1, 0, 0, "AACCGGT"),  # 0.9995: half-way cases of the decimal expansion
    (0, 65, 66, 2, 33, 65, 1, 0, 0, "GT"),
]


def _report(rows, read_of, n_reads):
    import torch

    n = len(rows)
    fields = np.zeros((n, 14), np.int32)
    for k, r in enumerate(rows):
        fields[k, :9] = r[:9]
        fields[k, 9:13] = (3, 2, 5, 7)
    units = b"".join(r[9].encode() for r in rows)
    unit_off = np.zeros(n + 1, np.int64)
    unit_off[1:] = np.cumsum([len(r[9]) for r in rows])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = fields[:, 5].astype(np.float32) / fields[:, 2].astype(np.float32)
    counts = np.bincount(np.array(read_of, np.int64), minlength=n_reads).astype(np.int32)
    return mtr_amd.Report(torch.from_numpy(counts), torch.from_numpy(np.array(read_of, np.int32)), torch.arange(n, dtype=torch.int32),
                          torch.from_numpy(fields), torch.from_numpy(ratio), torch.from_numpy(unit_off),
                          torch.from_numpy(np.frombuffer(units, np.uint8).copy()))


def test_format_report_equals_the_command_lines_report_lines():
    hu.build_host()
    host = C.CDLL(os.path.join(hu.HOST, "libmtr_host.so"))
    host.mtrh_format_ratio.argtypes = [C.c_int, C.c_int, C.c_char_p]
    host.mtrh_format_ratio.restype = C.c_int
    read_of = [0, 0, 1, 1, 1, 2, 3, 3, 3, 5, 5]            # read 4 reports nothing
    ids = ["r0", "second read", "r2 x=1", "r3", "r4", ">r5"]
    lens = [120, 90, 10000, 7, 66, 2100]
    got = mtr_amd.format_report(ids, lens, _report(CANNED, read_of, len(ids)))
    want = []
    for k, r in enumerate(CANNED):
        buf = C.create_string_buffer(64)
        n = host.mtrh_format_ratio(r[5], r[2], buf)
        cols = [str(lens[read_of[k]]), str(r[0] + 1), str(r[1] + 1), *(str(v) for v in r[2:6]), buf.raw[:n].decode(), *(str(v) for v in r[6:9]), r[9]]
        want.append(f"{ids[read_of[k]]}\t" + "\t".join(cols) + "\n")
    assert got == "".join(want).encode()
    assert b"\tinf\t" in got and b"nan\t" in got and b"\t0.142857\t" in got


def test_format_report_of_an_empty_report():
    rep = _report([], [], 1)
    assert mtr_amd.format_report(["a"], [5], rep) == b""
