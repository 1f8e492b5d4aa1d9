"""--sam without a device: bh_md_host (the MD definition in plain sequential C) against the Python model (tests/samlib.py) on hand-made paths
and on cigarlib's pool, its argument checks, the writer as a stand-alone program under the sanitizers (fake tracer, bh_md_host as the MD
function), the name collision and the lengths table, and the refusals of the command lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarlib as cg
import goldenlib as gl
import pilecases
import samlib

ROOT = gl.ROOT
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
Q100 = os.path.join(gl.G, "q100.fa")
E_USAGE, E_IO = -1, -2
LANE = np.array([1 + i % 4 for i in range(400)], np.uint8)      # A C G T repeated


def both(lane, first, text):
    from burst_amd import host
    ops = samlib.words(text)
    got = host.md_host(lane, first, ops)
    assert got == samlib.md_codes(lane, first, ops), text
    return got[0].decode(), got[1]


@pytest.mark.parametrize("text,md,nm", [("100=", "100", 0), ("1X", "0A0", 1), ("2X", "0A0C0", 2), ("3=2D1X4=", "3^TA0C4", 3), ("5=2I5=", "10", 2), ("1X1D", "0A0^C0", 2)])
def test_the_six_examples(text, md, nm):
    """the issue's examples, on a lane A C G T ...: the letters under 3=2D1X4= are those of columns 4, 5 and 6"""
    assert both(LANE, 1, text) == (md, nm)


def test_insertions_counters_and_letters():
    assert both(LANE, 1, "2I8=") == ("8", 2) and both(LANE, 1, "8=2I") == ("8", 2) and both(LANE, 5, "3I") == ("0", 3)
    for n in (9, 10, 99, 100):      # the counter's decimal widths, before an X, before a D and at the end
        md, nm = both(LANE, 3, "%d=1X%d=2D%d=" % (n, n, n))
        assert md.startswith("%d" % n) and md.endswith("%d" % n) and md.count("%d" % n) >= 3 and nm == 3
    lane = np.arange(16, dtype=np.uint8)      # every code once: the pad code prints N
    assert both(lane, 1, "16X")[0] == "0" + "0".join("NACGTNKMRYSWBVHD") + "0"
    assert both(lane, 1, "1=15D")[0] == "1^ACGTNKMRYSWBVHD0"
    assert both(lane, 16, "1X") == ("0D0", 1)      # the lane's last column


def test_argument_checks():
    from burst_amd import host
    for first, ops in ((0, [1 << 4 | 8]), (400, [2 << 4 | 7]), (1, [3]), (1, [4 << 4 | 3]), (1, [400 << 4 | 7, 1 << 4 | 2])):
        with pytest.raises(host.HostError):
            host.md_host(LANE, first, ops)
    assert host.md_host(LANE, 400, [1 << 4 | 8]) == (b"0T0", 1)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


def test_pool_against_the_model(L):
    """every path of cigarlib's pool (21 lanes in two clumps, reads of 2 .. 1 100 symbols): bh_md_host = the model"""
    from burst_amd import host
    pool = pilecases.PileCases(L, 1)
    n_x = n_d = 0
    for c in pool.cases:
        lane = np.asarray(pool.seqs[c["refIx"]], np.uint8)
        got = host.md_host(lane, c["ref_first"], c["ops"])
        assert got == samlib.md_codes(lane, c["ref_first"], c["ops"])
        n_x += b"^" not in got[0] and got[1] > 0
        n_d += b"^" in got[0]
    assert len(pool.cases) > 100 and n_x > 10 and n_d > 10


def test_apply_md_recovers_the_letters_of_md_host():
    """samlib.apply_md (CIGAR and MD walked together, the independent check of the command-line tests) recovers the letters bh_md_host printed"""
    from burst_amd import host
    md, _ = host.md_host(LANE, 6, samlib.words("4=1X2=3D2I5=2X"))
    got = samlib.apply_md("", 6, "4=1X2=3D2I5=2X", md.decode())
    assert got == {9: "C", 12: "A", 13: "C", 14: "G", 20: "A", 21: "C"}


def test_host_file_under_the_sanitizers(tmp_path):
    """csrc/host/bh_sam.c (with bh_paths.c, whose collector list feeds it) as a stand-alone program with ASan and UBSan linked in: flags, the
    secondary flag per read with a duplicate read, name truncation, unmapped order, the SN collision, a failure that leaves no file"""
    exe = str(tmp_path / "sam_host_main")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "sam_host_main.c"), os.path.join(CSRC, "host", "bh_sam.c"), os.path.join(CSRC, "host", "bh_paths.c"),
                           os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path / "o.b6")], capture_output=True, text=True, timeout=120)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "sam_host_main ok" in r.stdout, r.stdout + r.stderr
    assert "share the name 'chr1'" in r.stdout and r.stdout.count("Sam: 6 records") == 2
    assert sorted(os.listdir(str(tmp_path))) == ["o.b6", "sam_host_main"]


def test_names_and_lengths(tmp_path):
    """two different headers of one SN are a usage error that names both; --sam-lengths has the errors of --coverage-lengths"""
    from burst_amd import host
    lib = host.lib()
    h = C.c_void_p()
    heads = (C.c_char_p * 2)(b"seq1 a", b"seq1 b")
    lens = np.array([5, 6], np.uint32)
    assert lib.bh_sam_open_heads(2, heads, lens.ctypes.data, 0, C.byref(h)) == E_USAGE and not h
    err = lib.bh_last_error().decode()
    assert "'seq1 a'" in err and "'seq1 b'" in err and "--sam" in err
    db = host.Db.read(EDX)
    assert lib.bh_sam_open(C.byref(db.c), str(tmp_path / "missing.txt").encode(), 0, C.byref(h)) == E_IO
    heads = [x for x, _ in samlib.sq_of(samlib.fasta(os.path.join(gl.G, "refs.fa")))]      # the database's headers in the order of their numbers
    t = tmp_path / "len.txt"
    t.write_text("".join("%s\t%d\n" % (x, 1000 + k) for k, x in enumerate(heads[:-1])))
    assert lib.bh_sam_open(C.byref(db.c), str(t).encode(), 0, C.byref(h)) == E_USAGE
    assert "--sam-lengths" in lib.bh_last_error().decode() and heads[-1] in lib.bh_last_error().decode()
    t.write_text("no tab here\n")
    assert lib.bh_sam_open(C.byref(db.c), str(t).encode(), 0, C.byref(h)) == E_USAGE and "name<TAB>length" in lib.bh_last_error().decode()
    t.write_text("".join("%s\t%d\n" % (x, 1000 + k) for k, x in enumerate(heads)))
    assert lib.bh_sam_open(C.byref(db.c), str(t).encode(), 1, C.byref(h)) == 0
    lib.bh_sam_close(h)


REFUSALS = [(["-x"], "-x"), (["-d"], "-d"), (["--make-acx", "x.acx"], "--make-acx"), (["--shard", "db", "--gpus", "2"], "--shard db"), (["--shards", "2"], "--shards"),
            (["--gpus", "2", "--gather", "rccl"], "rccl"), (["--mates", "m.fa", "-m", "ALLPATHS"], "--mates")]


@pytest.mark.parametrize("extra,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_before_a_device_is_touched(tmp_path, extra, word):
    """usage errors, exit code 1, with nothing read, no device opened (this machine may have none) and no file left"""
    r = subprocess.run([BURST_HIP, "-r", EDX, "-q", Q100, "-o", str(tmp_path / "o.b6"), "--sam"] + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --sam" in r.stdout and word in r.stdout, r.stdout
    assert os.listdir(str(tmp_path)) == []


def test_a_mates_field_in_a_samples_line_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\tb.fa\n")
    r = subprocess.run([BURST_HIP, "-r", EDX, "-ad", "--samples", str(lst), "-m", "ALLPATHS", "-fr", "--sam"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "ERROR: --sam" in r.stdout and "mates" in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == ["list.txt"]


@pytest.mark.parametrize("opt", [["--sam-unmapped"], ["--sam-lengths", "len.txt"]])
def test_sub_options_without_sam_are_refused(tmp_path, opt):
    r = subprocess.run([BURST_HIP, "-r", EDX, "-q", Q100, "-o", str(tmp_path / "o.b6")] + opt, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "go with --sam" in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--sam"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--sam is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    for flag in ("--sam", "--sam-unmapped", "--sam-lengths <file>", "MD:Z:"):
        assert flag in r.stdout, flag


def test_session_arguments():
    from burst_amd import capi, host
    db = host.Db.read(EDX)
    with pytest.raises(ValueError, match="go with sam"):
        host.Session(db, None, align=lambda *a: None, sam_unmapped=True)
    with pytest.raises(ValueError, match="sam"):
        host.Session(db, None, align=lambda *a: None, sam=True)
    assert "bhip_md_tags" in capi.EXPORTS and capi.MD_INFO == ("device_us", "requests", "md_bytes", "peak_bytes")
