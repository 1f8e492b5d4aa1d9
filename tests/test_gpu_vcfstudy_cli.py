"""burst_hip --vcf --vcf-study end to end on the MI355X, on the golden dna.edx: a study of three samples -- reads with a planted
substitution, insertion and deletion; the same windows unedited; q292.fa, which lies elsewhere -- whose study file equals the file
vcfstudylib renders from the three .b6 files' own CIGAR columns (nothing of the project is involved in that replay), byte for byte; every
OUT.vcf and .b6 is what a run without the flag writes; a -q / -o run is a study of one sample; the Python session writes the command
line's file."""
import os
import subprocess

import numpy as np
import pytest

import cigarlib as cg
import goldenlib as gl
import pilelib
import samlib
import vcflib
import vcfstudylib

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
DB = os.path.join(gl.G, "dna.edx")
Q292 = os.path.join(gl.G, "q292.fa")
REFS_LIST = samlib.fasta(os.path.join(gl.G, "refs.fa"))
REFS = dict(REFS_LIST)
SQ = samlib.sq_of(REFS_LIST)      # the unique headers in the order of their numbers, with the database's own extents
CONTIGS = [(samlib.name_of(h), n) for h, n in SQ]
NUMBER = {h: k for k, (h, _) in enumerate(SQ)}
COMP = str.maketrans("ACGT", "TGCA")
COMMON = ["-r", DB, "-ad", "-m", "BEST", "-i", "0.95", "-fr", "--cigar", "--vcf", "--vcf-min-depth", "2", "--vcf-min-alt", "2"]
READ = 160


def run(args):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def free_windows():
    """(header, sequence, three window starts, 0-based) on a reference where no read of q292.fa is placed anywhere under the identity of these
    runs: the recorded FORAGE output at 0.95 holds every such placement"""
    taken = {}
    for ln in open(os.path.join(gl.G, "dna_q292_forage_fr.b6")):
        f = ln.split("\t")
        taken.setdefault(f[1], []).append((min(int(f[8]), int(f[9])), max(int(f[8]), int(f[9]))))
    for name, seq in REFS_LIST:
        starts, at = [], 20
        while at + READ + 20 <= len(seq) and len(starts) < 3:
            lo, hi = at - 19, at + READ + 20      # 1-based, with a margin
            if set(seq[at:at + READ]) <= set("ACGT") and not any(a <= hi and b >= lo for a, b in taken.get(name, [])):
                starts.append(at)
                at += READ + 40
            else:
                at += 10
        if len(starts) == 3:
            return name, seq, starts
    raise AssertionError("no reference has three windows without a read of q292.fa")


def two_query_files(tmp_path):
    """edited.fa: per window four reads that carry one edit (a substitution, an insertion, a deletion): three cuts of one edited read and the
    reverse complement of one of them.  plain.fa: the same cuts of the unedited windows"""
    rng = np.random.default_rng(21)
    name, seq, starts = free_windows()
    codes = np.array([pilelib.CODE[c] for c in seq], np.uint8)
    edited, plain = str(tmp_path / "edited.fa"), str(tmp_path / "plain.fa")
    with open(edited, "w") as fe, open(plain, "w") as fp:
        for k, (kind, edits) in enumerate((("sub", (1, 0, 0)), ("ins", (0, 1, 0)), ("del", (0, 0, 1)))):
            start = starts[k]
            while True:      # the edit well inside the read, so that every cut keeps it interior
                read = cg.edit_read(rng, codes, start, READ, *edits)
                n = min(len(read), READ) - 1
                differs = read[:n] != codes[start:start + n]
                if differs.any() and 40 <= int(np.argmax(differs)) <= 110:
                    break
            for f, text in ((fe, "".join(pilelib.LETTERS[c] for c in read)), (fp, seq[start:start + READ])):
                for j, (a, b) in enumerate(((0, 12), (6, 6), (12, 0))):
                    f.write(">%s_cut%d\n%s\n" % (kind, j, text[a:len(text) - b]))
                f.write(">%s_reverse\n%s\n" % (kind, text[3:len(text) - 3].translate(COMP)[::-1]))
    return edited, plain, samlib.name_of(name), [(s + 30, s + 125) for s in starts]


def lines_of(b6, qfile):
    queries = {samlib.name_of(n): s for n, s in samlib.fasta(qfile)}
    return pilelib.lines_of_b6(open(b6).read(), REFS, queries)


def body(b):
    return [ln.split("\t") for ln in b.decode().split("\n") if ln and not ln.startswith("#")]


def no_temporary_files(d):
    assert sorted(f for f in os.listdir(str(d)) if "tmp" in f) == []


def test_study_of_three_samples(tmp_path):
    edited, plain, contig, windows = two_query_files(tmp_path)
    d1, d2 = tmp_path / "study", tmp_path / "without"
    d1.mkdir(), d2.mkdir()
    samples = [("edited", edited), ("plain", plain), ("q292", Q292)]
    for d in (d1, d2):
        (d / "list.txt").write_text("".join("%s\t%s\n" % (q, d / (name + ".b6")) for name, q in samples))
    text = run(COMMON + ["--samples", str(d1 / "list.txt"), "--vcf-study", str(d1 / "P_")])
    assert "Samples: 3 done, 0 failed" in text and text.count("\nVcf: ") == 3 and "Study VCF written: %sstudy.vcf" % (d1 / "P_") in text
    got = open(str(d1 / "P_study.vcf"), "rb").read()
    exp, count = vcfstudylib.render(CONTIGS, [n for n, _ in samples], [lines_of(str(d1 / (n + ".b6")), q) for n, q in samples], 2, 2, number=lambda h: NUMBER[h])
    assert got == exp
    assert count["snv"] >= 1 and count["del"] >= 1 and count["ins"] >= 1, count
    line = next(ln for ln in text.split("\n") if ln.startswith("VcfStudy: "))
    assert "3 samples done, 0 failed, records %d SNV / %d Del / %d Ins, %d cells" % (count["snv"], count["del"], count["ins"], 3 * sum(count.values())) in line
    # every sample's own files are those of a run without the flag, and the projections of the study file
    run(COMMON + ["--samples", str(d2 / "list.txt")])
    for k, (name, _) in enumerate(samples):
        for ext in (".b6", ".b6.vcf"):
            assert open(str(d1 / (name + ext)), "rb").read() == open(str(d2 / (name + ext)), "rb").read(), name + ext
        own = open(str(d1 / (name + ".b6.vcf")), "rb").read()
        assert vcfstudylib.project(got, k, 2, 2) == ["\t".join(r) for r in body(own)], name
    # at the planted edits the unedited sample has its reads on the reference, and q292 has no read
    planted = [r for r in body(got) if r[0] == contig and any(a <= int(r[1]) <= b for a, b in windows)]
    kinds = set("snv" if len(r[3]) == len(r[4].split(",")[0]) else "del" if len(r[3]) > len(r[4]) else "ins" for r in planted)
    assert kinds == {"snv", "del", "ins"}, planted
    for r in planted:
        e, p, z = (r[9 + k].split(":") for k in range(3))
        assert int(e[0]) >= 2 and max(int(x) for x in e[1].split(",")[1:]) >= 2
        assert int(p[0]) > 0 and p[1].split(",")[0] == p[0] and set(p[1].split(",")[1:]) == {"0"}, r
        assert z[0] == "0" and set(z[1].split(",")) == {"0"}, r
        assert r[7] == "DP=%d;NS=2" % (int(e[0]) + int(p[0]))
    assert sorted(os.listdir(str(d1))) == sorted(os.listdir(str(d2)) + ["P_study.vcf"])
    no_temporary_files(d1)


def test_a_single_run_is_a_study_of_one_sample(tmp_path):
    edited, _, _, _ = two_query_files(tmp_path)
    out = str(tmp_path / "one.b6")
    text = run(COMMON + ["-q", edited, "-o", out, "--vcf-study", str(tmp_path / "Q_")])
    assert "\nVcfStudy: 1 samples done, 0 failed" in text
    got, own = open(str(tmp_path / "Q_study.vcf"), "rb").read(), open(out + ".vcf", "rb").read()
    exp, count = vcfstudylib.render(CONTIGS, ["one"], [lines_of(out, edited)], 2, 2, number=lambda h: NUMBER[h])
    assert got == exp and sum(count.values()) >= 3
    assert own == vcflib.render(CONTIGS, "one", lines_of(out, edited), 2, 2, number=lambda h: NUMBER[h])[0]
    assert [r[:7] + r[8:] for r in body(got)] == [r[:7] + r[8:] for r in body(own)]      # the records of OUT.vcf, one column; INFO gains NS
    assert all(r[7] == o[7] + ";NS=1" for r, o in zip(body(got), body(own)))
    no_temporary_files(tmp_path)


def test_python_session_writes_what_the_command_line_writes(tmp_path):
    """host.Session(vcf=True, vcf_study=prefix) on the device and with the plain C solvers: the command line's study file both times"""
    from burst_amd import host
    edited, plain, _, _ = two_query_files(tmp_path)
    cli = tmp_path / "cli"
    cli.mkdir()
    (cli / "list.txt").write_text("%s\t%s\n%s\t%s\n" % (edited, cli / "edited.b6", plain, cli / "plain.b6"))
    run(COMMON + ["--samples", str(cli / "list.txt"), "--vcf-study", str(cli / "P_")])
    want = open(str(cli / "P_study.vcf"), "rb").read()
    assert len(body(want)) >= 3
    db = host.Db.read(DB)
    dev = db.open_device(0, build_K=12)
    with pytest.raises(ValueError, match="vcf_study goes with vcf"):
        host.Session(db, dev, vcf_study="P_")
    for k, on_host in enumerate((False, True)):
        d = tmp_path / ("ses%d" % k)
        d.mkdir()
        with host.Session(db, dev, mode="BEST", thres=0.95, rc=True, accel=True, K=12, cigar=True, vcf=True, vcf_min_depth=2, vcf_min_alt=2, vcf_host=on_host,
                          vcf_study=str(d / "P_"), vcf_study_host=on_host) as s:
            for name, q in (("edited", edited), ("plain", plain)):
                res = s.run(q, str(d / (name + ".b6")))
                assert res["rc"] == 0, res["err"]
            info = s.vcf_study()
            assert (info["samples"], info["failed"]) == (2, 0) and info["snv"] + info["del"] + info["ins"] == len(body(want)) and info["host_bytes"] > 0
            assert (info["device_us"] > 0) == (not on_host)
        assert open(str(d / "P_study.vcf"), "rb").read() == want
        for f in ("edited.b6", "edited.b6.vcf", "plain.b6.vcf"):
            assert open(str(d / f), "rb").read() == open(str(cli / f), "rb").read(), f
        no_temporary_files(d)
