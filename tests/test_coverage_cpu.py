"""Coverage and count tables (burst_hip --coverage, bh_cov.c) where there is no device: the table writer against the reference's
bcov fixtures (tests/golden/cov, made by make_cov_golden.py), its edge cases, the report's placement sink through the CPU session of
tests/test_samples_cpu.py (the oracle as align back end), the lengths table and the command line's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covlib
import goldenlib as gl
from test_samples_cpu import EDX, Q100, Q292, make_align

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
COV = os.path.join(gl.G, "cov")
LEN = os.path.join(COV, "len.txt")
E_USAGE, E_DEVICE = -1, -5


def write_tables(prefix, headers, lengths, col_names, shared, unique):
    """bh_cov_write_tables: shared / unique [columns][headers][4], col_names the samples' (column 0 is Dataset)"""
    from burst_amd import host
    hs = (C.c_char_p * len(headers))(*[h.encode() for h in headers])
    names = (C.c_char_p * (len(col_names) + 1))(*([None] + [n.encode() for n in col_names]))
    ln = np.ascontiguousarray(lengths, np.uint32)
    sh, un = np.ascontiguousarray(shared, np.uint64), np.ascontiguousarray(unique, np.uint64)
    rc = host.lib().bh_cov_write_tables(prefix.encode(), len(headers), hs, ln.ctypes.data, len(col_names) + 1, names, sh.ctypes.data, un.ctypes.data)
    assert rc == 0, host.lib().bh_last_error()
    return {k: open(prefix + k, "rb").read() for k in covlib.KINDS}


def test_writer_reproduces_bcov(tmp_path):
    """1: integer statistics from dense numpy depth arrays of dna_q100_best.b6 + len.txt -> the host's writer -> bcov's tables, byte for byte"""
    lens = covlib.read_lengths(LEN)
    headers = sorted(lens, key=lambda h: h.encode())
    lengths = [lens[h] for h in headers]
    sh, un = covlib.b6_columns([os.path.join(gl.G, "dna_q100_best.b6")], headers, lengths)
    got = write_tables(str(tmp_path / "w_"), headers, lengths, [], sh[:1], un[:1])
    for kind in ("shared", "shared_binary"):
        want = open(os.path.join(COV, "dna_q100_best_%s.txt" % kind), "rb").read()
        assert got[kind + ".txt"] == want and want.count(b"\n") == 65
    assert got == covlib.tables(headers, lengths, [], sh[:1], un[:1])
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp" in f]


def test_writer_edge_cases(tmp_path):
    """2: mean > sd prints positive; L = 1; unique depth 0 beside shared depth > 0 is a row of 0.0000; rows in strcmp order of the whole
    header, also where headers differ only after a space; a header without shared depth is no row"""
    headers = ["r b", "r", "r a", "one", "tiled", "empty"]
    lengths = [50, 50, 50, 1, 40, 30]
    ref = [0, 1, 2, 3] + [4] * 30 + [4]
    st = [1, 1, 1, 1] + [1] * 30 + [1]
    ed = [11, 21, 31, 2] + [41] * 30 + [21]
    uniq = [False, True, False, True] + [True] * 30 + [False]
    sh, un = covlib.dense_stats(np.array(ref), np.array(st), np.array(ed), np.ones(len(ref), np.int64), np.array(uniq), lengths)
    got = write_tables(str(tmp_path / "e_"), headers, lengths, ["s1"], np.stack([sh, sh]), np.stack([un, un]))
    rows = [ln.split(b"\t") for ln in got["shared.txt"].splitlines()]
    assert rows[0] == [b"#Coverage", b"Dataset", b"s1"] and got["counts.txt"].splitlines()[0] == b"#OTU ID\tDataset\ts1"
    assert [r[0] for r in rows[1:]] == [b"one", b"r", b"r a", b"r b", b"tiled"]          # strcmp: "r" < "r a" < "r b"; "empty" has no row
    cell = {k: {r.split(b"\t")[0]: r.split(b"\t")[1:] for r in got[k].splitlines()[1:]} for k in covlib.KINDS}
    assert cell["shared.txt"][b"tiled"] == [b"30.5000", b"30.5000"]                         # depth 31 on 20 bases, 30 on 20: mean 30.5 > sd 0.5064
    assert cell["unique.txt"][b"tiled"] == [b"30.0000", b"30.0000"] and cell["unique_binary.txt"][b"tiled"] == [b"1.0000", b"1.0000"]
    assert cell["shared.txt"][b"one"] == [b"1.0000", b"1.0000"] and cell["shared_binary.txt"][b"one"] == [b"1.0000", b"1.0000"]      # L = 1
    assert cell["shared.txt"][b"r a"] == [b"0.6000", b"0.6000"] and cell["unique.txt"][b"r a"] == [b"0.0000", b"0.0000"]             # mean 0.6 > sd 0.4949; no unique depth
    assert cell["shared.txt"][b"r b"] == [b"-0.2000", b"-0.2000"]                                                                      # mean 0.2 < sd 0.4041
    assert cell["unique_binary.txt"][b"r b"] == [b"0.0000", b"0.0000"] and cell["shared_binary.txt"][b"r b"] == [b"0.2000", b"0.2000"]
    assert cell["counts.txt"][b"tiled"] == [b"31", b"31"] and cell["counts.txt"][b"r"] == [b"1", b"1"]
    assert got == covlib.tables(headers, lengths, ["s1"], np.stack([sh, sh]), np.stack([un, un]))


def db_headers(db):
    """the unique headers of a database in header-number order (BhDb.headDump: NUL-separated)"""
    out, p = [], db.c.headDump
    for _ in range(db.c.numRefHeads):
        s = C.string_at(p)
        out.append(s.decode())
        p += len(s) + 1
    return out


@pytest.mark.parametrize("mode", ["ALLPATHS", "CAPITALIST"])
def test_sink_delivers_the_lines_of_the_file(mode, tmp_path, monkeypatch):
    """3: -fr through the CPU session with chunks of 7 unique queries rendered by 3 threads: what the sink delivers (expanded by its
    weights) is what the .b6 of the same call holds -- header, columns 9 / 10, and the unique flag recomputed from the file"""
    from burst_amd import host
    monkeypatch.setenv("BURST_HOST_REPORT_THREADS", "3:7")
    db = host.Db.read(EDX)
    heads = db_headers(db)
    seen = {}

    def tap(sample, lines):
        seen[sample] = lines
        return True
    files = [Q100, Q292]
    with host.Session(db, None, mode=mode, thres=0.95, rc=True, accel=False, align=make_align(db), coverage=str(tmp_path / "c_"), coverage_lengths=LEN, coverage_tap=tap) as s:
        outs = []
        for i, q in enumerate(files):
            outs.append(str(tmp_path / ("s%d.b6" % i)))
            assert s.run(q, outs[-1])["rc"] == 0
        assert not s.ended
    assert sorted(seen) == [0, 1]
    for i, o in enumerate(outs):
        want = sorted((r[1], r[2], r[3], r[4]) for r in covlib.parse_b6(o))
        ln = seen[i]
        w = (ln["w"] & 0x7FFFFFFF).astype(np.int64)
        got = sorted((heads[int(r)], int(a), int(b), bool(u >> 31)) for r, a, b, u, k in zip(ln["ref"], ln["st"], ln["ed"], ln["w"], w) for _ in range(int(k)))
        assert got == want and len(want) > 100
        assert any(a > b for _, a, b, _ in want) and (mode != "ALLPATHS" or not all(u for _, _, _, u in want))      # reverse lines, and reads on several lines
    db.close()


def test_no_device_is_a_device_error_and_leaves_no_tables(tmp_path):
    """(9, the error path) the statistics are the device's: a session whose rank 0 has no handle ends on BH_E_DEVICE at its first
    sample's coverage, and closing it writes no table, whole or partial"""
    from burst_amd import host
    db = host.Db.read(EDX)
    prefix = str(tmp_path / "d_")
    with host.Session(db, None, mode="BEST", thres=0.97, accel=False, align=make_align(db), coverage=prefix, coverage_lengths=LEN) as s:
        res = s.run(Q100, str(tmp_path / "a.b6"))
        assert res["rc"] == E_DEVICE and "coverage" in res["err"] and s.ended
        assert s.run(Q100, str(tmp_path / "b.b6"))["rc"] == E_DEVICE
    assert sorted(os.listdir(str(tmp_path))) == ["a.b6"]
    db.close()


def test_lengths_table_must_name_every_header(tmp_path):
    """4a: a header of the database missing from --coverage-lengths is a usage error that names it"""
    from burst_amd import host
    db = host.Db.read(EDX)
    short = tmp_path / "short.txt"
    lines = open(LEN).read().splitlines()
    gone = [ln for ln in lines if ln.startswith("ref07_1 ")]
    assert len(gone) == 1
    short.write_text("\n".join(ln for ln in lines if ln != gone[0]) + "\n")
    cov = C.c_void_p()
    assert host.lib().bh_cov_open(C.byref(db.c), b"p_", str(short).encode(), 0, C.byref(cov)) == E_USAGE and not cov
    assert gone[0].split("\t")[0] in host.lib().bh_last_error().decode()
    assert host.lib().bh_cov_open(C.byref(db.c), b"p_", LEN.encode(), 0, C.byref(cov)) == 0
    nh = C.c_uint32()
    host.lib().bh_cov_dims(cov, None, C.byref(nh))
    got = host._view(host.lib().bh_cov_lengths(cov), nh.value, np.uint32)
    lens = covlib.read_lengths(LEN)
    assert [int(x) for x in got] == [lens[h] for h in db_headers(db)]
    host.lib().bh_cov_close(cov)
    db.close()


def test_default_lengths_from_host_extents():
    """the database's own extent of every header, from the packed references in host memory: max(refStart + lane length) over the
    header's fragments, restated in numpy from the .edx tables"""
    from burst_amd import host
    for name in ("dna.edx", "quick.edx"):
        db = host.Db.read(os.path.join(gl.G, name))
        ext = np.zeros(16 * db.c.numRclumps, np.uint32)
        host.lib().bh_cov_extents_host(C.byref(db.c), ext.ctypes.data)
        assert np.array_equal(ext, lane_lengths(db))
        got = np.zeros(db.c.numRefHeads, np.uint32)
        assert host.lib().bh_cov_lengths_from_extents(C.byref(db.c), ext.ctypes.data, got.ctypes.data) == 0
        assert np.array_equal(got, default_lengths(db, ext)) and got.min() > 0
        db.close()


def lane_lengths(db):
    """index after the last non-pad symbol of every lane, from the clump area as the file packs it (tests/dbutil.py: byte z of a
    16-byte row = lane z, low nibble = even position)"""
    from burst_amd import host
    cl = host._view(db.c.clumpLen, db.c.numRclumps, np.uint32)
    packed = host._view(db.c.packed, db.c.packedWords * 16, np.uint8)
    out, w0 = np.zeros(16 * len(cl), np.uint32), 0
    for c, L in enumerate(cl):
        rows = int(L) // 2 + (int(L) & 1)
        b = packed[16 * w0:16 * (w0 + rows)].reshape(rows, 16)
        sym = np.zeros((2 * rows, 16), np.uint8)
        sym[0::2], sym[1::2] = b & 15, b >> 4
        nz = sym != 0
        out[16 * c:16 * c + 16] = np.where(nz.any(0), 2 * rows - np.argmax(nz[::-1], 0), 0)
        w0 += rows
    return out


def default_lengths(db, ext):
    from burst_amd import host
    n = db.c.origTotR
    ref_map, tmp_rix = host._view(db.c.refMap, n, np.uint32), host._view(db.c.tmpRIX, n, np.uint32)
    start = host._view(db.c.refStart, n, np.uint32) if db.c.refStart else np.zeros(n, np.uint32)
    dd = host._view(db.c.refDedupIx, db.c.totR + 1, np.uint32) if db.c.refDedupIx else np.arange(db.c.totR + 1, dtype=np.uint32)
    out = np.zeros(db.c.numRefHeads, np.uint32)
    for lane in range(db.c.totR):
        for k in range(int(dd[lane]), int(dd[lane + 1])):
            rix = int(tmp_rix[k])
            out[ref_map[rix]] = max(int(out[ref_map[rix]]), int(start[rix]) + int(ext[lane]))
    return out


def _cli(args, cwd):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=cwd, timeout=120)
    return r.returncode, r.stdout


def test_command_line_refusals(tmp_path):
    """4b: --coverage does not go with -d, --make-acx or -x: exit code 1 and one line, before anything is created (on the code before
    the feature, --coverage is an unrecognised option)"""
    d = str(tmp_path)
    refs = os.path.join(gl.G, "refs.fa")
    for args in (["-r", refs, "-d", "QUICK", "-o", os.path.join(d, "x.edx"), "--coverage", "p_"],
                 ["-r", EDX, "--make-acx", os.path.join(d, "x.acx"), "--coverage", "p_"],
                 ["-r", refs, "-q", Q100, "-o", os.path.join(d, "x.b6"), "-x", "--coverage", "p_"],
                 ["-r", EDX, "-q", Q100, "-o", os.path.join(d, "x.b6"), "--coverage-pad", "3"]):
        code, text = _cli(args, d)
        errs = [ln for ln in text.splitlines() if ln.startswith("ERROR")]
        assert code == 1 and len(errs) == 1 and "--coverage" in errs[0] and "Unrecognized" not in text, (args, code, text[-400:])
    assert os.listdir(d) == []
    assert "--coverage" in _cli(["-h"], d)[1]
