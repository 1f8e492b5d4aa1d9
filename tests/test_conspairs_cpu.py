"""--consensus-pairs without a device: bh_consensus_pairs_host against the dictionary model of conspairslib, and the collector with the
three files against the model applied to the consensus.fa of the same run -- both through the stand-alone program
tests/csrc/conspairs_host_main.c with ASan and UBSan linked in; every refusal of the command line before a device is touched; the entry
points and the ABI version."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import conspairscases as cc
import conspairslib as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")
QO = ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", "out.b6"]
SUFFIXES = ("consensus_pairs.txt", "consensus_identity.txt", "consensus_compared.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """csrc/host/bh_conspairs.c and bh_consensus.c as a stand-alone program with the sanitizers' runtimes linked in"""
    path = str(tmp_path_factory.mktemp("conspairs_exe") / "conspairs_host_main")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "conspairs_host_main.c")] +
                          [os.path.join(CSRC, "host", f) for f in ("bh_conspairs.c", "bh_consensus.c", "bh_tables.c")] + ["-o", path])
    return path


def solve(exe, tmp_path, n_samples, segs, letters, min_compared=1, pair_cap=None):
    """bh_consensus_pairs_host in the sanitizer program -> (return code, n_pairs, info, pairs, text)"""
    from burst_amd import capi
    segs, letters = capi.pair_arrays(segs, letters)
    if pair_cap is None:
        pair_cap = 1 << 16
    fin, fout = str(tmp_path / "case.in"), str(tmp_path / "case.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<IIQQQ", n_samples, min_compared, len(segs), len(letters), pair_cap) + segs.tobytes() + letters.tobytes())
    r = subprocess.run([exe, "solve", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    rc, n = struct.unpack("<qQ", raw[:16])
    info = struct.unpack("<8Q", raw[16:80])
    if rc == 0:
        return rc, n, info, np.frombuffer(raw[80:80 + 24 * n], capi.PAIR_DTYPE), ""
    return rc, n, info, None, raw[80:].decode()


def same_as_model(exe, tmp_path, case, min_compared=1):
    n, segs, letters = case
    rows = cl.rows_of_segs(segs, letters)
    want = cl.pairs(rows, min_compared)
    rc, n_pairs, info, got, text = solve(exe, tmp_path, n, segs, letters, min_compared)
    assert rc == 0, text
    assert got.tobytes() == cl.pairs_array(want).tobytes()
    assert info[:5] == cl.info(rows, len(segs), len(want)) and info[5:] == (0, 0, 0)
    return want


@pytest.mark.parametrize("seed", range(6))
def test_yardstick_equals_the_model_on_random_inputs(exe, tmp_path, seed):
    want = same_as_model(exe, tmp_path, cc.random_case(seed))
    assert want and any(c != s for _, _, _, c, s in want) and any(s for _, _, _, _, s in want)


@pytest.mark.parametrize("m", [1, 2, 13])
def test_yardstick_on_the_shapes_written_by_hand(exe, tmp_path, m):
    want = same_as_model(exe, tmp_path, cc.shapes(), m)
    if m == 1:
        by = {(h, a, b): (c, s) for h, a, b, c, s in want}
        assert (3, 0, 1) in by and by[(3, 0, 1)] == (9, 7)      # 9000..9008 (N behind them): T against A and A against '-' differ, '-' against '-' is equal
        assert (4, 0, 3) in by and by[(4, 0, 3)] == (4, 3)      # R against R is not compared; T against A differs
        assert (40, 1, 3) not in by and (40, 2, 3) not in by    # Compared == 0 is never a pair
        assert by[(40, 1, 2)][0] > by[(40, 1, 2)][1] > 0
    if m == 13:
        assert all(c >= 13 for _, _, _, c, _ in want) and want


@pytest.mark.parametrize("n_samples,union", [(1, 64), (2, 1), (2, 33), (3, 65), (17, 129), (65, 130), (5, 4160)])
def test_yardstick_on_one_header(exe, tmp_path, n_samples, union):
    same_as_model(exe, tmp_path, cc.one_header(n_samples, union, 7 * n_samples + union))


def test_yardstick_on_the_long_segment_and_the_wide_header(exe, tmp_path):
    assert len(same_as_model(exe, tmp_path, cc.long_segment())) == 4
    want = same_as_model(exe, tmp_path, cc.wide_header())
    assert len(want) == 5 and max(c for _, _, _, c, _ in want) > 20000


def test_yardstick_relabelling_and_capacity(exe, tmp_path):
    case = cc.random_case(3)
    a = same_as_model(exe, tmp_path, case)
    b = same_as_model(exe, tmp_path, cc.relabel(case, 1, 4))
    swap = lambda s: 4 if s == 1 else 1 if s == 4 else s
    assert sorted((h, min(swap(x), swap(y)), max(swap(x), swap(y)), c, s) for h, x, y, c, s in a) == b
    from burst_amd import host
    rc, n, info, got, text = solve(exe, tmp_path, *case, pair_cap=len(a) - 1)
    assert rc == host.E_CAPACITY and n == len(a)
    rc, n, info, got, text = solve(exe, tmp_path, *case, pair_cap=len(a))
    assert rc == 0 and n == len(a)
    for n_samples in (0, 1):      # nothing to pair
        segs = case[1][case[1]["sample"] < n_samples]
        rc, n, info, got, text = solve(exe, tmp_path, n_samples, segs, case[2])
        assert rc == 0 and n == 0 and info == (len(segs), 0, 0, 0, 0, 0, 0, 0)
    rc, n, info, got, text = solve(exe, tmp_path, 5, None, b"")
    assert rc == 0 and n == 0 and info == (0,) * 8


@pytest.mark.parametrize("what,n_samples,rows,letters,m,text", cc.bad_arguments(), ids=[b[0] for b in cc.bad_arguments()])
def test_the_yardstick_refuses_what_the_device_refuses(exe, tmp_path, what, n_samples, rows, letters, m, text):
    from burst_amd import host
    rc, n, info, got, msg = solve(exe, tmp_path, n_samples, cc.seg_rows(rows), letters, m)
    assert rc == host.E_USAGE and text in msg and n == 0, msg


# ---- the collector and the three files -----------------------------------------------------------------------------------------------------

def study(exe, tmp_path, samples, min_breadth=0, m=1):
    """the program's study -> (names, failed names, the bytes of consensus.fa, the three files, standard output)"""
    work = tmp_path / ("study_%s_%d_%d" % (samples, min_breadth, m))
    work.mkdir()
    r = subprocess.run([exe, "study", str(work), samples, str(min_breadth), str(m)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "conspairs_host_main study ok" in r.stdout, r.stdout + r.stderr
    names = ["s%d_%c" % (i, c) for i, c in enumerate(samples)]
    failed = [n for n, c in zip(names, samples) if c == "f"]
    assert sorted(os.listdir(str(work))) == sorted("P_" + s for s in SUFFIXES + ("consensus.fa", "consensus.txt"))      # no temporary file
    fa = open(str(work / "P_consensus.fa"), "rb").read()
    return names, failed, fa, tuple(open(str(work / ("P_" + s)), "rb").read() for s in SUFFIXES), r.stdout


def rows_of(pairs_txt):
    return [ln.split("\t") for ln in pairs_txt.decode().split("\n")[1:] if ln]


def test_three_files_are_the_model_of_the_written_fasta(exe, tmp_path):
    names, failed, fa, got, out = study(exe, tmp_path, "abc")
    want = cl.files(fa, names, failed)
    assert got == want
    rows = rows_of(got[0])
    # rows in strcmp order of the header, then a, then b; the figures the sets were written for
    assert [r[:3] for r in rows] == [["alpha x", "s0_a", "s1_b"], ["alpha x", "s0_a", "s2_c"], ["alpha x", "s1_b", "s2_c"], ["beta", "s0_a", "s1_b"], ["beta", "s0_a", "s2_c"],
                                      ["beta", "s1_b", "s2_c"], ["gamma", "s0_a", "s1_b"]]
    by = {tuple(r[:3]): r[3:] for r in rows}
    assert by[("alpha x", "s0_a", "s1_b")] == ["12", "8", "7", "1", "0.875000"]      # '-' against a base
    assert by[("alpha x", "s0_a", "s2_c")] == ["12", "8", "8", "0", "1.000000"]      # '-' against '-'
    assert by[("beta", "s0_a", "s1_b")] == ["30", "16", "15", "1", "0.937500"]       # 9..16 is N in a: not compared; A against T at 24
    assert by[("beta", "s0_a", "s2_c")] == ["30", "8", "8", "0", "1.000000"]
    ident, comp = (g.decode().split("\n") for g in got[1:])
    assert ident[0] == "#Identity\ts0_a\ts1_b\ts2_c" and comp[0] == "#Compared\ts0_a\ts1_b\ts2_c"
    assert ident[1] == "s0_a\t1.000000\t%.6f\t1.000000" % (30 / 32) and comp[1] == "s0_a\t32\t32\t16"      # both diagonals
    for text in (ident, comp):      # symmetric
        cells = [ln.split("\t")[1:] for ln in text[1:4]]
        assert all(cells[a][b] == cells[b][a] for a in range(3) for b in range(3))
    assert "ConsensusPairs: 3 samples done, 0 failed, 8 records, 3 headers with two or more, 40 union positions, 7 pairs examined, 7 written" in out
    assert "device 0.000 ms" in out


def test_a_failed_sample_reads_na_in_its_row_and_column(exe, tmp_path):
    names, failed, fa, got, out = study(exe, tmp_path, "afb")
    assert failed == ["s1_f"] and got == cl.files(fa, names, failed)
    ident, comp = (g.decode().split("\n") for g in got[1:])
    assert ident[2] == "s1_f\tNA\tNA\tNA" and comp[2] == "s1_f\tNA\tNA\tNA"      # the diagonal included
    assert ident[1].split("\t")[2] == "NA" and comp[3].split("\t")[2] == "NA"
    assert all("s1_f" not in r[:3] for r in rows_of(got[0])) and rows_of(got[0])
    assert "sample 's1_f' failed alone" in out and "2 samples done, 1 failed" in out


def test_a_study_of_one_sample(exe, tmp_path):
    names, failed, fa, got, out = study(exe, tmp_path, "a")
    assert got == cl.files(fa, names, failed)
    assert got[0] == b"#Reference\tSampleA\tSampleB\tLength\tCompared\tSame\tDiffer\tIdentity\n"
    assert got[1] == b"#Identity\ts0_a\ns0_a\t1.000000\n" and got[2] == b"#Compared\ts0_a\ns0_a\t32\n"


def test_a_record_the_breadth_test_suppresses_drops_out_of_the_pairs(exe, tmp_path):
    # 700 permille: alpha x (8 of 12) and a's beta (16 of 30) are not written; b's beta (24 of 30) and both gammas (8 of 8) are
    names, failed, fa, got, out = study(exe, tmp_path, "ab", min_breadth=700)
    assert fa.count(b">") == 3 and got == cl.files(fa, names, failed)
    assert [r[:3] for r in rows_of(got[0])] == [["gamma", "s0_a", "s1_b"]]
    assert got[2].decode().split("\n")[1] == "s0_a\t8\t8"      # the diagonal counts the written records only
    assert ", 3 records, 1 headers with two or more, 8 union positions, 1 pairs examined, 1 written" in out


def test_m_above_every_compared_leaves_the_header_line_and_na(exe, tmp_path):
    names, failed, fa, got, out = study(exe, tmp_path, "abc", m=17)
    assert got == cl.files(fa, names, failed, 17)
    assert rows_of(got[0]) == [] and got[0].count(b"\n") == 1
    ident, comp = (g.decode().split("\n") for g in got[1:])
    assert ident[1] == "s0_a\t1.000000\tNA\tNA" and comp[1] == "s0_a\t32\t0\t0" and ident[3] == "s2_c\tNA\tNA\t1.000000"
    assert "7 pairs examined, 0 written" in out
    # one below: M = 16 keeps exactly the pair with Compared == 16
    names, failed, fa, got, out = study(exe, tmp_path, "abc", m=16)
    assert got == cl.files(fa, names, failed, 16) and [r[:3] for r in rows_of(got[0])] == [["beta", "s0_a", "s1_b"]]


def test_life_cycle_under_the_sanitizers(exe, tmp_path):
    work = tmp_path / "life"
    work.mkdir()
    r = subprocess.run([exe, "life", str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "conspairs_host_main life ok" in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(work)) == []


# ---- the command line, the launcher, the Python layer ----------------------------------------------------------------------------------------

def refused(tmp_path, args, *words):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS"] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and all(w in r.stdout for w in words), r.stdout + r.stderr
    assert "Parsing" not in r.stdout      # (before the database is read, let alone a device touched)
    assert os.listdir(str(tmp_path)) == []


def test_the_flags_go_with_consensus(tmp_path):
    refused(tmp_path, QO + ["--consensus-pairs"], "ERROR: --consensus-pairs and --consensus-pairs-min go with --consensus")
    refused(tmp_path, QO + ["--consensus-pairs-min", "5"], "ERROR: --consensus-pairs and --consensus-pairs-min go with --consensus")
    refused(tmp_path, QO + ["--consensus", "P_", "--consensus-pairs-min", "5"], "ERROR: --consensus-pairs-min goes with --consensus-pairs")


@pytest.mark.parametrize("value", ["0", "2147483648", "-1", "x", "1.5", ""])
def test_n_outside_its_range(tmp_path, value):
    word = "requires an argument" if value == "-1" else "ERROR: --consensus-pairs-min takes 1 .. 2147483647"
    refused(tmp_path, QO + ["--consensus", "P_", "--consensus-pairs", "--consensus-pairs-min", value], word)


@pytest.mark.parametrize("extra,word", [
    (QO + ["-x"], "-x"), (QO + ["-d"], "-d"), (QO + ["--make-acx", "x.acx"], "--make-acx"),
    (QO + ["--gpus", "2", "--shard", "db"], "--shard db"), (QO + ["--shards", "2"], "--shards"), (QO + ["--gpus", "2", "--gather", "rccl"], "rccl"),
    (QO + ["--mates", os.path.join(GOLDEN, "q100.fa")], "--mates"),
    (QO + ["-m", "FORAGE", "--cluster", "C"], "--cluster"), (QO + ["-m", "FORAGE", "--chimeras", "C"], "--chimeras"),
    (QO + ["--consensus-min-depth", "0"], "--consensus-min-depth"), (QO + ["--consensus-min-breadth", "1001"], "--consensus-min-breadth"),
    (QO + ["--consensus-reads", "some"], "--consensus-reads"),
])
def test_everything_that_refuses_consensus_refuses_the_pairs(tmp_path, extra, word):
    refused(tmp_path, ["--consensus", "P_", "--consensus-pairs"] + extra, "ERROR: --consensus", word)


def test_two_outputs_of_one_name_in_a_sample_list(tmp_path):
    work = tmp_path / "w"
    work.mkdir()
    lst = tmp_path / "list.txt"
    q = os.path.join(GOLDEN, "q100.fa")
    lst.write_text("%s\t%s\n%s\t%s\n" % (q, tmp_path / "a" / "x.b6", q, tmp_path / "b" / "x.tsv"))
    refused(work, ["--consensus", str(work / "P_"), "--consensus-pairs", "--samples", str(lst)], "ERROR: --consensus-pairs", "a/x.b6", "b/x.tsv", "'x'")
    # without the flag the consensus takes the list as it did (it stops later, at the database, which is not what this test is about)
    from burst_amd import host
    assert host.lib().bh_conspairs_check_names((host.C.c_char_p * 2)(b"a/x.b6", b"b/x.tsv"), 2) == host.E_USAGE
    assert host.lib().bh_conspairs_check_names((host.C.c_char_p * 2)(b"a/x.b6", b"b/y.b6"), 2) == 0


def test_launcher_refuses_the_flags():
    for extra in (["--consensus-pairs"], ["--consensus-pairs-min", "3"], ["--consensus", "P_", "--consensus-pairs"]):
        r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6"] + extra, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 1 and "--consensus-pairs is not available" in r.stdout and "burst_hip" in r.stdout, r.stdout + r.stderr


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--consensus-pairs [--consensus-pairs-min <int>]" in r.stdout and all(s in r.stdout for s in SUFFIXES)


def test_python_session_wants_a_consensus_with_the_pairs():
    from burst_amd import host
    with pytest.raises(ValueError, match="go with consensus=prefix"):
        host.Session(None, None, consensus_pairs=True)
    with pytest.raises(ValueError, match="go with consensus=prefix"):
        host.Session(None, None, consensus_pairs_min=4)
    with pytest.raises(ValueError, match="consensus_pairs_min goes with consensus_pairs=True"):
        host.Session(None, None, consensus="P_", consensus_pairs_min=4)
    with pytest.raises(ValueError, match="consensus_pairs_min: 1 .. 2\\^31 - 1"):
        host.Session(None, None, consensus="P_", consensus_pairs=True, consensus_pairs_min=1 << 31)


def test_python_yardstick_equals_the_model():
    from burst_amd import host
    n, segs, letters = cc.shapes()
    got, info = host.consensus_pairs_host(n, segs, letters, 2, pair_cap=1)      # (a capacity answer, then the room it asked for)
    rows = cl.rows_of_segs(segs, letters)
    want = cl.pairs(rows, 2)
    assert got.tobytes() == cl.pairs_array(want).tobytes() and tuple(int(x) for x in info[:5]) == cl.info(rows, len(segs), len(want))


def test_the_abi_version_stays_and_the_entry_points_exist():
    from burst_amd import capi, host
    assert capi.lib().bhip_abi_version() == 8
    assert {"bhip_consensus_pairs", "bhip_consensus_pairs_info"} <= set(capi.EXPORTS)
    assert hasattr(capi.lib(), "bhip_consensus_pairs") and hasattr(capi.lib(), "bhip_consensus_pairs_info")
    assert hasattr(capi.Device, "consensus_pairs") and hasattr(capi.Device, "consensus_pairs_info")
    for s in ("bh_conspairs_open", "bh_conspairs_set_solver", "bh_conspairs_check_names", "bh_conspairs_check_min", "bh_conspairs_attach", "bh_conspairs_add", "bh_conspairs_write",
              "bh_conspairs_commit", "bh_conspairs_abort", "bh_conspairs_print_info", "bh_conspairs_last_info", "bh_conspairs_close", "bh_consensus_pairs_host", "bh_consensus_set_pairs",
              "bh_consensus_pairs", "bh_session_consensus_pairs"):
        assert hasattr(host.lib(), s), s
    assert (capi.PAIR_SEG_DTYPE.itemsize, capi.PAIR_DTYPE.itemsize) == (24, 24)
    assert hasattr(host.Session, "consensus_pairs")
