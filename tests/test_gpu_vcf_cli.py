"""burst_hip --vcf end to end on the MI355X: OUT.vcf against the file vcflib renders by replaying the printed CIGARs over
tests/golden/refs.fa and the query file (nothing of the project is involved in that replay), byte for byte; the .b6 with the flag alone
is the .b6 without it; a study of two samples equals two invocations; --vcf-reads unique; the other outputs beside it keep their bytes."""
import os
import subprocess

import numpy as np
import pytest

import cigarlib as cg
import goldenlib as gl
import pilelib
import samlib
import vcflib

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
DB = os.path.join(gl.G, "dna.edx")
Q100 = os.path.join(gl.G, "q100.fa")
REFS_LIST = samlib.fasta(os.path.join(gl.G, "refs.fa"))
REFS = dict(REFS_LIST)
SQ = samlib.sq_of(REFS_LIST)      # the unique headers in the order of their numbers, with the database's own extents
CONTIGS = [(samlib.name_of(h), n) for h, n in SQ]
NUMBER = {h: k for k, (h, _) in enumerate(SQ)}
TIGHT = ["--vcf-min-depth", "2", "--vcf-min-alt", "2"]
COMP = str.maketrans("ACGT", "TGCA")


def run(args):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def with_edited_reads(tmp_path, name="q100_edited.fa"):
    """q100.fa and, for each of a substitution, an insertion and a deletion, four reads over one window of the first reference that carry
    the same edit: three cuts of one edited read, and the reverse complement of one of them"""
    rng = np.random.default_rng(21)
    _, seq = next((n, s) for n, s in REFS_LIST if len(s) >= 900 and set(s[:900]) <= set("ACGT"))
    codes = np.array([pilelib.CODE[c] for c in seq[:900]], np.uint8)
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(open(Q100).read())
        for k, (kind, edits) in enumerate((("sub", (1, 0, 0)), ("ins", (0, 1, 0)), ("del", (0, 0, 1)))):
            start = 100 + 250 * k
            while True:      # the edit well inside the read, so that every cut keeps it interior
                read = cg.edit_read(rng, codes, start, 160, *edits)
                same = int(np.argmax(read[:159] != codes[start:start + 159])) if (read[:159] != codes[start:start + 159]).any() else 0
                if 40 <= same <= 110:
                    break
            text = "".join(pilelib.LETTERS[c] for c in read)
            for j, (a, b) in enumerate(((0, 12), (6, 6), (12, 0))):
                f.write(">%s_cut%d\n%s\n" % (kind, j, text[a:len(text) - b]))
            f.write(">%s_reverse\n%s\n" % (kind, text[3:len(text) - 3].translate(COMP)[::-1]))
    return path


def model_vcf(out_with_cigar, qfile, sample, min_depth, min_alt, unique_only=False):
    queries = {samlib.name_of(n): s for n, s in samlib.fasta(qfile)}
    lines = pilelib.lines_of_b6(open(out_with_cigar).read(), REFS, queries, unique_only)
    return vcflib.render(CONTIGS, sample, lines, min_depth, min_alt, number=lambda h: NUMBER[h])


def no_temporary_files(tmp_path):
    assert sorted(f for f in os.listdir(str(tmp_path)) if "tmp" in f) == []


@pytest.mark.parametrize("mode", ["BEST", "ALLPATHS"])
def test_file_is_the_replay_of_the_printed_cigars(tmp_path, mode):
    qfile = with_edited_reads(tmp_path)
    base = ["-r", DB, "-ad", "-q", qfile, "-m", mode, "-i", "0.95", "-fr"]
    plain, alone, both = (str(tmp_path / n) for n in ("plain.b6", "alone.b6", "both.b6"))
    run(base + ["-o", plain])
    text = run(base + ["-o", alone, "--vcf"] + TIGHT)
    assert "\nVcf: " in text and "VCF records written: %s.vcf" % alone in text
    assert open(alone, "rb").read() == open(plain, "rb").read()      # the flag alone leaves the .b6 as it is
    text = run(base + ["-o", both, "--cigar", "--vcf"] + TIGHT)
    exp, count = model_vcf(both, qfile, "both", 2, 2)
    got = open(both + ".vcf", "rb").read()
    assert got == exp
    assert count["snv"] >= 1 and count["del"] >= 1 and count["ins"] >= 1, count      # records of all three kinds
    line = next(ln for ln in text.split("\n") if ln.startswith("Vcf: "))
    assert "records written %d SNV / %d Del / %d Ins" % (count["snv"], count["del"], count["ins"]) in line
    # the same records whether or not the lines carry their columns; only the sample's name differs
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"#CHROM")]
    assert body(open(alone + ".vcf", "rb").read()) == body(got)
    no_temporary_files(tmp_path)


def test_samples_study_equals_separate_invocations(tmp_path):
    qfile = with_edited_reads(tmp_path)
    q292 = os.path.join(gl.G, "q292.fa")
    d1, d2 = tmp_path / "study", tmp_path / "alone"
    d1.mkdir(), d2.mkdir()
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\n%s\t%s\n" % (qfile, d1 / "zz_first.b6", q292, d1 / "aa_second.b6"))
    common = ["-r", DB, "-ad", "-m", "BEST", "-i", "0.95", "-fr", "--cigar", "--vcf", "--vcf-min-depth", "1", "--vcf-min-alt", "1"]
    text = run(common + ["--samples", str(lst)])
    assert "Samples: 2 done, 0 failed" in text and text.count("\nVcf: ") == 2
    for q, name in ((qfile, "zz_first"), (q292, "aa_second")):
        run(common + ["-q", q, "-o", str(d2 / (name + ".b6"))])
        a, b = open(str(d1 / (name + ".b6.vcf")), "rb").read(), open(str(d2 / (name + ".b6.vcf")), "rb").read()
        assert a == b and a.count(b"\n") > 15
        exp, _ = model_vcf(str(d1 / (name + ".b6")), q, name, 1, 1)
        assert a == exp
    no_temporary_files(d1), no_temporary_files(d2)


def test_unique_reads_only(tmp_path):
    base = ["-r", DB, "-ad", "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--cigar"]
    out = str(tmp_path / "u.b6")
    run(base + ["-o", out, "--vcf", "--vcf-reads", "unique", "--vcf-min-depth", "1", "--vcf-min-alt", "1"])
    exp_u, count_u = model_vcf(out, Q100, "u", 1, 1, unique_only=True)
    exp_all, _ = model_vcf(out, Q100, "u", 1, 1)
    assert open(out + ".vcf", "rb").read() == exp_u
    assert exp_u != exp_all and sum(count_u.values()), "ALLPATHS prints no read on more than one line: the rule was not exercised"


def test_the_other_outputs_beside_it_keep_their_bytes(tmp_path):
    qfile = with_edited_reads(tmp_path)
    base = ["-r", DB, "-ad", "-q", qfile, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--sam", "--variants"]
    d1, d2 = tmp_path / "without", tmp_path / "with"
    d1.mkdir(), d2.mkdir()
    run(base + [str(d1 / "V_"), "-o", str(d1 / "o.b6")])
    run(base + [str(d2 / "V_"), "-o", str(d2 / "o.b6"), "--vcf"] + TIGHT)
    for f in ("o.b6", "o.b6.sam", "V_variants.txt"):
        assert open(str(d1 / f), "rb").read() == open(str(d2 / f), "rb").read(), f
    assert sorted(os.listdir(str(d2))) == ["V_variants.txt", "o.b6", "o.b6.sam", "o.b6.vcf"]
    assert sorted(os.listdir(str(d1))) == ["V_variants.txt", "o.b6", "o.b6.sam"]


def test_lengths_table_reaches_the_contig_lines(tmp_path):
    """--vcf-lengths: the contig lengths come from the table, whatever the database's own extents say"""
    lens = {h: 100000 + 7 * k for k, (h, _) in enumerate(REFS_LIST)}
    table = tmp_path / "len.tsv"
    table.write_text("".join("%s\t%d\n" % kv for kv in lens.items()))
    out = str(tmp_path / "o.b6")
    run(["-r", DB, "-ad", "-q", Q100, "-m", "BEST", "-i", "0.95", "-o", out, "--cigar", "--vcf", "--vcf-min-depth", "1", "--vcf-min-alt", "1", "--vcf-lengths", str(table)])
    queries = {samlib.name_of(n): s for n, s in samlib.fasta(Q100)}
    contigs = [(samlib.name_of(h), n) for h, n in samlib.sq_of(REFS_LIST, lens)]
    exp, _ = vcflib.render(contigs, "o", pilelib.lines_of_b6(open(out).read(), REFS, queries), 1, 1, number=lambda h: NUMBER[h])
    got = open(out + ".vcf", "rb").read()
    assert got == exp and b",length=100000>\n" in got


def test_python_session_writes_what_the_command_line_writes(tmp_path):
    """host.Session(vcf=True) on the device and with the plain C solvers (vcf_host=True): the command line's file both times"""
    from burst_amd import host
    cli_out = str(tmp_path / "s.b6")
    run(["-r", DB, "-ad", "-q", Q100, "-o", cli_out, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--vcf", "--vcf-min-depth", "1", "--vcf-min-alt", "1"])
    want = open(cli_out + ".vcf", "rb").read()
    db = host.Db.read(DB)
    dev = db.open_device(0, build_K=12)
    for k, on_host in enumerate((False, True)):
        d = tmp_path / ("ses%d" % k)
        d.mkdir()
        with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, vcf=True, vcf_min_depth=1, vcf_min_alt=1, vcf_host=on_host) as s:
            res = s.run(Q100, str(d / "s.b6"))
            assert res["rc"] == 0, res["err"]
            info = s.vcf_info()
            assert info["lines"] > 0 and info["snv"] + info["del"] + info["ins"] == sum(1 for ln in want.split(b"\n") if ln and not ln.startswith(b"#"))
        assert open(str(d / "s.b6.vcf"), "rb").read() == want
        assert open(str(d / "s.b6"), "rb").read() == open(cli_out, "rb").read()
