"""mtr_amd.format_report(..., alignments=...) against mTR -a's recorded output (CPU): the committed <name>.a.stdout files of tests/golden
(the unmodified reference) are parsed back into per-repeat rows, handed over as Report + ReportAlignments columns, and must come out
byte for byte.  alignment_block_port is mtr_amd/host/print.c: alignment_block in Python (the GPU tests check the device's rows with it)."""
import os

import numpy as np
import pytest

import mtr_amd
from tests import golden_util as gu

W = 50                                                        # MTRH_ALIGN_WIDTH


def alignment_block_port(codes, L, after, f, unit: bytes, ops_tb, end_pos, end_col) -> bytes:
    """print.c: alignment_block - ops_tb one byte per column, LAST column first; f the 14 header ints; returns the printed block"""
    out = f"\nmatch gain = {f[10]}, mismatch penalty = {f[11]}, indel penalty = {f[12]}\n\n".encode()
    U, n = int(f[3]), len(ops_tb)
    if U <= 0 or n <= 0:
        return out
    a_in, a_sym, a_rep = bytearray(n), bytearray(n), bytearray(n)
    p, j = int(end_pos), int(end_col)
    for q in range(n):
        c = ops_tb[q]
        code = codes[p] if 0 <= p < L else (after[p - L] if L <= p < L + 2 else 0)
        xb, ub = b"ACGT"[code & 3], unit[j - 1]
        if c == 1:
            a_in[q], a_sym[q], a_rep[q] = xb, 0x7c, ub
            p -= 1; j -= 1
        elif c == 2:
            a_in[q], a_sym[q], a_rep[q] = xb, 0x20, ub
            p -= 1; j -= 1
        elif c == 3:
            a_in[q], a_sym[q], a_rep[q] = 0x2d, 0x20, ub
            j -= 1
        else:
            a_in[q], a_sym[q], a_rep[q] = xb, 0x20, 0x2d
            p -= 1
        if j == 0:
            j = U
    s = n - 1
    while s >= 0:
        e = s - W if s - W >= -1 else -1
        for row in (a_in, a_sym, a_rep):
            out += bytes(row[e + 1:s + 1][::-1]) + b"\n"
        out += b"\n"
        s -= W
    return out


def parse_a_stdout(data: bytes):
    """-> (ids, lens, rows): rows = per repeat (read index, report-line columns, (G, M, D), (read row, symbol row, unit row))"""
    lines = data.split(b"\n")
    assert lines[-1] == b""
    ids, lens, rows, i = [], [], [], 0
    while i < len(lines) - 1:
        cols = lines[i].split(b"\t")
        assert len(cols) == 13 and lines[i + 1] == b"" and lines[i + 3] == b"", (i, lines[i])
        sc = lines[i + 2].decode()
        g, m, d = (int(part.rsplit("=", 1)[1]) for part in sc.split(","))
        if not ids or ids[-1] != cols[0]:
            ids.append(cols[0]); lens.append(int(cols[1]))
        i += 4
        a, b, c = b"", b"", b""
        while i < len(lines) - 1 and b"\t" not in lines[i]:
            assert lines[i + 3] == b"" and len(lines[i]) == len(lines[i + 1]) == len(lines[i + 2]) > 0, i
            a += lines[i]; b += lines[i + 1]; c += lines[i + 2]
            i += 4
        rows.append((len(ids) - 1, cols, (g, m, d), (a, b, c)))
    return ids, lens, rows


def columns_from_rows(rows, n_reads):
    """Report + ReportAlignments (numpy columns) of parsed rows"""
    n = len(rows)
    fields = np.zeros((n, 14), np.int32)
    read = np.zeros(n, np.int32)
    units, texts = [], []
    for k, (rd, cols, gmd, text) in enumerate(rows):
        v = [int(x) for x in cols[2:8]] + [int(x) for x in cols[9:12]]
        fields[k, :9] = (v[0] - 1, v[1] - 1, v[2], v[3], v[4], v[5], v[6], v[7], v[8])
        fields[k, 10:13] = gmd
        read[k] = rd
        units.append(cols[12]); texts.append(text)
    unit_off = np.zeros(n + 1, np.int64); unit_off[1:] = np.cumsum([len(u) for u in units])
    col_off = np.zeros(n + 1, np.int64); col_off[1:] = np.cumsum([len(t[0]) for t in texts])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = fields[:, 5].astype(np.float32) / fields[:, 2].astype(np.float32)
    rep = mtr_amd.Report(np.bincount(read, minlength=n_reads).astype(np.int32), read, np.arange(n, dtype=np.int32), fields, ratio, unit_off,
                         np.frombuffer(b"".join(units), np.uint8))
    text = np.stack([np.frombuffer(b"".join(t[r] for t in texts), np.uint8) for r in range(3)]) if n else np.zeros((3, 0), np.uint8)
    ops = np.where(text[0] == 0x2d, 3, np.where(text[2] == 0x2d, 4, np.where(text[1] == 0x7c, 1, 2))).astype(np.uint8)
    return rep, mtr_amd.ReportAlignments(col_off, ops, text, np.zeros((n, 2), np.int32))


@pytest.mark.parametrize("name", ["edge", "3_5", "synth_c2", "10_50"])
def test_format_report_reproduces_the_recorded_a_output(name):
    want = open(os.path.join(gu.GOLDEN, f"{name}.a.stdout"), "rb").read()
    ids, lens, rows = parse_a_stdout(want)
    assert len(rows) > 0 and sum(len(r[3][0]) for r in rows) > 100
    rep, al = columns_from_rows(rows, len(ids))
    assert mtr_amd.format_report(ids, lens, rep, alignments=al) == want
    # without the alignments: the report lines alone, which is what the reference prints without -a
    assert mtr_amd.format_report(ids, lens, rep) == open(os.path.join(gu.GOLDEN, f"{name}.default.stdout"), "rb").read()
    assert mtr_amd.format_report(ids, lens, rep, None) == mtr_amd.format_report(ids, lens, rep)


def _hand_made(n_cols, seed):
    """a repeat of n_cols columns with every kind of column: (fields, unit, traceback ops, end_pos, end_col, read codes)"""
    rng = np.random.RandomState(seed)
    unit = b"ACGGT"
    ops_fw = rng.choice([1, 1, 1, 2, 3, 4], size=n_cols).astype(np.uint8)
    rows = int((ops_fw != 3).sum())
    codes = rng.randint(0, 4, size=rows + 7).astype(np.uint8)
    f = [3, 3 + rows - 1, rows, len(unit), 0, int((ops_fw == 1).sum()), int((ops_fw == 2).sum()), int((ops_fw == 4).sum()), int((ops_fw == 3).sum()), 3, 2, 1, 4, 0]
    end_col = 1 + (int((ops_fw != 4).sum()) + 2 - 1) % len(unit) if n_cols else 0        # the path starts at unit column 3
    return f, unit, ops_fw[::-1].copy(), 3 + rows - 1, end_col, codes


def test_block_boundaries_and_a_repeat_without_columns():
    made = [_hand_made(n, 10 + n) for n in (50, 51, 100, 0, 1, 149)]
    want, rows = b"", []
    codes = np.concatenate([m[5] for m in made])
    base = np.cumsum([0] + [len(m[5]) for m in made])
    L = len(codes)
    for k, (f, unit, ops_tb, end_pos, end_col, _) in enumerate(made):
        f = list(f); f[0] += int(base[k]); f[1] += int(base[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.float32(f[5]) / np.float32(f[2])                # (0 / 0 for the repeat without columns: the host's "-nan")
        line = f"hand\t{L}\t{f[0] + 1}\t{f[1] + 1}\t{f[2]}\t{f[3]}\t{f[4]}\t{f[5]}\t{mtr_amd._c_float_text(ratio)}"
        line += f"\t{f[6]}\t{f[7]}\t{f[8]}\t{unit.decode()}\n"
        block = alignment_block_port(codes, L, (0, 0), f, unit, ops_tb, end_pos + int(base[k]), end_col)
        want += line.encode() + block
        body = block.split(b"\n")[3:]                               # behind the scores line and its two empty lines
        text = tuple(b"".join(body[r::4]) for r in range(3))
        assert len(text[0]) == len(ops_tb)
        assert block.count(b"\n") == 3 + 4 * ((len(ops_tb) + W - 1) // W)
        rows.append((0, line.encode().rstrip(b"\n").split(b"\t"), (f[10], f[11], f[12]), text))
    rep, al = columns_from_rows(rows, 1)
    assert np.array_equal(al.ops, np.concatenate([m[2][::-1] for m in made]))
    assert al.col_off.tolist() == [0, 50, 101, 201, 201, 202, 351]
    assert mtr_amd.format_report(["hand"], [L], rep, alignments=al) == want
    # a report whose repeats all lack columns, and an empty report
    rep0, al0 = columns_from_rows(rows[3:4], 1)
    assert al0.text.shape == (3, 0)
    assert mtr_amd.format_report(["hand"], [L], rep0, alignments=al0).endswith(b"\n\nmatch gain = 2, mismatch penalty = 1, indel penalty = 4\n\n")
    repe, ale = columns_from_rows([], 1)
    assert mtr_amd.format_report(["hand"], [L], repe, alignments=ale) == b""


def test_alignments_of_another_report_are_refused():
    _, _, rows = parse_a_stdout(open(os.path.join(gu.GOLDEN, "edge.a.stdout"), "rb").read())
    rep, al = columns_from_rows(rows, 10)
    rep1, _ = columns_from_rows(rows[:-1], 10)
    with pytest.raises(mtr_amd.MtrError):
        mtr_amd.format_report([b"x"] * 10, [1] * 10, rep1, alignments=al)
