"""burst_hip --consensus end to end on the MI355X: both files against the ones conslib builds by replaying the printed CIGARs over
tests/golden/refs.fa and the query file (nothing of the project is involved in that replay), byte for byte, on q100.fa plus a planted
pile-up with a substitution, a deletion and an insertion; the .b6 with the flag alone is the .b6 without it; the other outputs keep their
bytes beside it; a study of two samples; unique reads; the breadth cut-off; the lengths table and its errors; the Python session."""
import os
import subprocess

import pytest

import goldenlib as gl
import conslib
import pilelib

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
DB = os.path.join(gl.G, "dna.edx")
Q100 = os.path.join(gl.G, "q100.fa")
Q292 = os.path.join(gl.G, "q292.fa")
REFS = {name: seq for name, seq in pilelib.read_fasta(os.path.join(gl.G, "refs.fa"))}
LENGTHS = {name: len(seq) for name, seq in REFS.items()}
PLANT = next(n for n, s in REFS.items() if len(s) >= 700 and set(s[:700].upper()) <= set("ACGT"))      # the first all-ACGT reference
SUB, DEL, INS = 150, 250, 350      # 0-based offsets on PLANT that the planted reads edit
BASE = ["-r", DB, "-ad", "-m", "BEST", "-i", "0.95", "-fr"]


def run(args, want=0):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == want, r.stdout[-3000:]
    return r.stdout


def no_tmp(tmp_path):
    return sorted(f for f in os.listdir(str(tmp_path)) if "tmp" in f) == []


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """q100.fa and 40 reads of 100 bases at stride 10 cut from PLANT; every read that covers SUB / DEL / INS has that base substituted /
    deleted / a base inserted behind it"""
    seq = REFS[PLANT].upper()
    path = str(tmp_path_factory.mktemp("planted") / "q100_planted.fa")
    with open(path, "w") as f:
        f.write(open(Q100).read())
        for k in range(40):
            read = []
            for p in range(10 * k, 10 * k + 100):
                if p == SUB:
                    read.append("ACGT"[("ACGT".index(seq[p]) + 1) % 4])
                elif p != DEL:
                    read.append(seq[p])
                if p == INS:
                    read.append("ACGT"[("ACGT".index(seq[p]) + 2) % 4])
            f.write(">planted_%d\n%s\n" % (k, "".join(read)))
    return path


def model(samples, min_depth=4, min_breadth=0, unique_only=False, lengths=LENGTHS):
    """samples = [(output with the --cigar columns, query file)] in study order -> conslib.files"""
    study = []
    for out, qfile in samples:
        queries = {n: s for n, s in pilelib.read_fasta(qfile)}
        study.append((os.path.splitext(os.path.basename(out))[0], pilelib.lines_of_b6(open(out).read(), REFS, queries, unique_only)))
    return conslib.files(study, lengths, min_depth, min_breadth)


def test_both_files_are_the_replay_of_the_printed_cigars(tmp_path, planted):
    q = ["-q", planted]
    plain, alone, cig, allof = (str(tmp_path / n) for n in ("plain.b6", "alone.b6", "cig.b6", "all.b6"))
    run(BASE + q + ["-o", plain])
    text = run(BASE + q + ["-o", alone, "--consensus", str(tmp_path / "A_")])
    assert "\nConsensus: " in text and "\nPaths: " not in text
    assert open(alone, "rb").read() == open(plain, "rb").read()      # the flag alone leaves the .b6 as it is
    # beside --cigar --variants --sam: the requests of --cigar alone, and the other outputs keep their bytes
    t_cig = run(BASE + q + ["-o", cig, "--cigar", "--variants", str(tmp_path / "C_"), "--sam"])
    t_all = run(BASE + q + ["-o", allof, "--cigar", "--variants", str(tmp_path / "B_"), "--sam", "--consensus", str(tmp_path / "B_")])
    paths = lambda t: [ln.rsplit(",", 1)[0] for ln in t.split("\n") if ln.startswith("Paths: ")]      # requests, ops and lines, without the time
    assert paths(t_all) == paths(t_cig) and paths(t_cig)
    assert open(allof, "rb").read() == open(cig, "rb").read()
    assert open(str(tmp_path / "B_variants.txt"), "rb").read().replace(b"\tall\t", b"\tcig\t") == open(str(tmp_path / "C_variants.txt"), "rb").read()
    assert open(allof + ".sam", "rb").read() == open(cig + ".sam", "rb").read()
    # the model first: the data must show what the test is about
    fa, txt, rows = model([(allof, planted)])
    row = next(r for r in rows if r[0] == PLANT)
    assert row[6] >= 1 and row[7] >= 1 and row[9] >= 1 and row[10] == 1, row      # Subst, Del, InsMajor, a record
    fa_lines = fa.decode().split("\n")
    rec = fa_lines[fa_lines.index(">all|" + PLANT) + 1]
    # (the aligner may place a gap anywhere inside a run of equal bases, and an edit next to one likewise: look around the planted offsets)
    ref = REFS[PLANT].upper()
    assert len(rec) == LENGTHS[PLANT] and "-" in rec[DEL - 8:DEL + 9]
    assert any(rec[p] in "ACGT" and rec[p] != ref[p] for p in range(SUB - 8, SUB + 9))
    assert "N" in rec.strip("N"), "no position under --consensus-min-depth inside a segment"
    assert open(str(tmp_path / "B_consensus.txt"), "rb").read() == txt
    assert open(str(tmp_path / "B_consensus.fa"), "rb").read() == fa
    # the same letters whether or not the lines carry their columns; only the sample's name differs
    assert open(str(tmp_path / "A_consensus.fa"), "rb").read().replace(b">alone|", b">all|") == fa
    assert no_tmp(tmp_path)


def test_samples_study_of_two_blocks_in_study_order(tmp_path):
    lst = tmp_path / "list.txt"
    outs = [str(tmp_path / "zz_first.b6"), str(tmp_path / "aa_second.b6")]
    lst.write_text("%s\t%s\n%s\t%s\n" % (Q100, outs[0], Q292, outs[1]))
    text = run(BASE + ["--samples", str(lst), "--cigar", "--consensus", str(tmp_path / "S_"), "--consensus-min-depth", "1"])
    assert "Samples: 2 done, 0 failed" in text and text.count("\nConsensus: ") == 2
    fa, txt, rows = model([(outs[0], Q100), (outs[1], Q292)], 1)
    assert open(str(tmp_path / "S_consensus.txt"), "rb").read() == txt
    assert open(str(tmp_path / "S_consensus.fa"), "rb").read() == fa
    names = [r[1] for r in rows]
    assert names == sorted(names, key=["zz_first", "aa_second"].index) and set(names) == {"zz_first", "aa_second"}
    assert no_tmp(tmp_path)


def test_unique_reads_and_the_breadth_cut_off(tmp_path):
    out = str(tmp_path / "u.b6")
    args = ["-r", DB, "-ad", "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--cigar", "-o", out, "--consensus-min-depth", "1"]
    run(args + ["--consensus", str(tmp_path / "U_"), "--consensus-reads", "unique"])
    fa_u, txt_u, _ = model([(out, Q100)], 1, unique_only=True)
    fa_all, txt_all, rows = model([(out, Q100)], 1)
    assert open(str(tmp_path / "U_consensus.fa"), "rb").read() == fa_u and open(str(tmp_path / "U_consensus.txt"), "rb").read() == txt_u
    assert txt_u != txt_all, "ALLPATHS prints no read on more than one line: the rule was not exercised"
    run(args + ["--consensus", str(tmp_path / "F_"), "--consensus-min-breadth", "1000"])
    fa_b, txt_b, rows_b = model([(out, Q100)], 1, 1000)
    assert fa_b == b"" and len(rows_b) == len(rows) > 0 and not any(r[10] for r in rows_b)      # no record, all table rows
    assert open(str(tmp_path / "F_consensus.fa"), "rb").read() == b"" and open(str(tmp_path / "F_consensus.txt"), "rb").read() == txt_b
    assert no_tmp(tmp_path)


def test_lengths_table_and_its_errors(tmp_path):
    out = str(tmp_path / "l.b6")
    args = BASE + ["-q", Q100, "--cigar", "-o", out, "--consensus-min-depth", "1", "--consensus", str(tmp_path / "L_")]
    longer = {n: v + 17 for n, v in LENGTHS.items()}
    table = tmp_path / "len.txt"
    table.write_text("".join("%s\t%d\n" % kv for kv in longer.items()))
    run(args + ["--consensus-lengths", str(table)])
    fa, txt, rows = model([(out, Q100)], 1, lengths=longer)
    assert open(str(tmp_path / "L_consensus.fa"), "rb").read() == fa and open(str(tmp_path / "L_consensus.txt"), "rb").read() == txt and rows
    os.remove(str(tmp_path / "L_consensus.fa")); os.remove(str(tmp_path / "L_consensus.txt"))
    # a table that lacks a header: a usage error that names it, before a device is touched
    missing = rows[0][0]
    table.write_text("".join("%s\t%d\n" % kv for kv in longer.items() if kv[0] != missing))
    text = run(args + ["--consensus-lengths", str(table)], want=1)
    assert "--consensus-lengths" in text and missing in text
    # a table shorter than a placement: a usage error that names the header, and no files
    short = dict(longer)
    short[missing] = 3
    table.write_text("".join("%s\t%d\n" % kv for kv in short.items()))
    text = run(args + ["--consensus-lengths", str(table)], want=1)
    assert "--consensus" in text and "'%s'" % missing in text and "beyond its length 3" in text
    assert sorted(os.listdir(str(tmp_path))) in (["l.b6", "len.txt"], ["len.txt"])
    assert no_tmp(tmp_path)


def test_python_session_writes_what_the_command_line_writes(tmp_path):
    """host.Session(consensus=...) on the device and with the plain C yardstick (consensus_host=True): the command line's files both times"""
    from burst_amd import host
    cli_out = str(tmp_path / "s.b6")
    run(["-r", DB, "-ad", "-q", Q100, "-o", cli_out, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--consensus", str(tmp_path / "C_"), "--consensus-min-depth", "1"])
    want_fa, want_txt = open(str(tmp_path / "C_consensus.fa"), "rb").read(), open(str(tmp_path / "C_consensus.txt"), "rb").read()
    assert want_txt.count(b"\n") > 1 and want_fa.count(b">") > 0
    db = host.Db.read(DB)
    dev = db.open_device(0, build_K=12)
    for k, on_host in enumerate((False, True)):
        d = tmp_path / ("ses%d" % k)
        d.mkdir()
        with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, consensus=str(d / "P_"), consensus_min_depth=1, consensus_host=on_host) as s:
            res = s.run(Q100, str(d / "s.b6"))
            assert res["rc"] == 0, res["err"]
            rows = s.consensus()
            assert len(rows) == want_txt.count(b"\n") - 1 and set(rows["sample"].tolist()) == {0}
            info = s.consensus_info()
            assert info["segments"] > 0 and info["lines"] > 0 and info["records"] == want_fa.count(b">") and info["covered"] == int(rows["covered"].sum())
        assert open(str(d / "P_consensus.txt"), "rb").read() == want_txt
        assert open(str(d / "P_consensus.fa"), "rb").read() == want_fa
        assert open(str(d / "s.b6"), "rb").read() == open(cli_out, "rb").read()
