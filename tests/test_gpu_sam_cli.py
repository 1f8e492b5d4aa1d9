"""burst_hip --sam end to end on the MI355X, on the golden database: the .sam is the model's file (tests/samlib.py) byte for byte, the .b6
is the bytes of the run without the flag, every record passes checks that involve neither the model nor the project's code (SEQ length, NM,
the reference letters its CIGAR and MD claim against tests/golden/refs.fa), and the flag goes with --sam-unmapped, --samples, two ranks,
--variants, --chimeras and FASTA references."""
import os
import subprocess

import pytest

import goldenlib as gl
import samlib

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
REFS_FA = os.path.join(gl.G, "refs.fa")
Q100 = os.path.join(gl.G, "q100.fa")
REFS = samlib.fasta(REFS_FA)


def run(args):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


SQ = samlib.sq_of(REFS)      # the database's own extents are the lengths of the references


def check_properties(sam_text, b6_text, refs=REFS):
    """independent of the model: SEQ length = '=' + X + I, NM = column 11, and the letters CIGAR + MD claim are those of refs.fa"""
    import re
    rseq = {samlib.name_of(h): s for h, s in refs}
    recs = [r for r in samlib.records(sam_text) if not int(r[1]) & 4]
    lines = [ln.split("\t") for ln in b6_text.split("\n") if ln]
    assert len(recs) == len(lines) > 50
    n_claims = 0
    for r, f in zip(recs, lines):
        n = {c: 0 for c in "=XID"}
        for k, c in re.findall(r"(\d+)([=XID])", r[5]):
            n[c] += int(k)
        assert len(r[9]) == n["="] + n["X"] + n["I"]
        assert r[11] == "NM:i:" + f[10] and int(f[10]) == n["X"] + n["I"] + n["D"]
        assert r[12].startswith("MD:Z:") and r[4] == "255" and r[10] == "*"
        ref = rseq[r[2]]
        claims = samlib.apply_md(r[9], int(r[3]), r[5], r[12][5:])
        for x, letter in claims.items():
            assert (ref[x] if ref[x] in samlib.MD_LETTERS[1:] else "N") == letter, (r[0], x)
        n_claims += len(claims)
    assert n_claims > 20
    return recs


CASES = [("ALLPATHS", "0.95", ["-fr", "-ad"]), ("BEST", "0.95", ["-ad"]), ("FORAGE", "0.95", ["-fr", "-ad"])]


@pytest.mark.parametrize("mode,ident,extra", CASES, ids=[c[0] for c in CASES])
def test_sam_is_the_models_file(mode, ident, extra, tmp_path):
    base = ["-r", EDX, "-q", Q100, "-m", mode, "-i", ident] + extra
    plain, cig, both, sam_only = (str(tmp_path / x) for x in ("plain.b6", "cigar.b6", "both.b6", "sam.b6"))
    run(base + ["-o", plain])
    run(base + ["-o", cig, "--cigar"])
    text = run(base + ["-o", both, "--cigar", "--sam"])
    assert "\nSam: " in text and "SAM records written" in text
    run(base + ["-o", sam_only, "--sam"])
    assert open(both, "rb").read() == open(cig, "rb").read()
    assert open(sam_only, "rb").read() == open(plain, "rb").read()      # without --cigar the .b6 keeps its columns
    b6 = open(cig).read()
    got = open(both + ".sam").read()
    assert got == samlib.expected_sam(b6, samlib.fasta(Q100), REFS, SQ)
    assert open(sam_only + ".sam").read() == got
    recs = check_properties(got, b6)
    if mode != "BEST":
        assert any(int(r[1]) & 0x100 for r in recs) and any(int(r[1]) & 0x10 for r in recs)
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp" in f]


@pytest.fixture(scope="module")
def mixed_queries(tmp_path_factory):
    """q100's first 40 reads with reads the database cannot place between them"""
    import numpy as np
    rng = np.random.default_rng(5)
    q = samlib.fasta(Q100)[:40]
    path = str(tmp_path_factory.mktemp("samq") / "mixed.fa")
    with open(path, "w") as f:
        for k, (h, s) in enumerate(q):
            f.write(">%s\n%s\n" % (h, s))
            if k % 4 == 0:
                f.write(">junk%d with a comment\n%s\n" % (k, "".join("ACGT"[i] for i in rng.integers(0, 4, size=90))))
    return path


def test_unmapped_records(mixed_queries, tmp_path):
    out = str(tmp_path / "o.b6")
    text = run(["-r", EDX, "-ad", "-q", mixed_queries, "-m", "BEST", "-i", "0.95", "-fr", "-o", out, "--cigar", "--sam", "--sam-unmapped"])
    b6 = open(out).read()
    q = samlib.fasta(mixed_queries)
    got = open(out + ".sam").read()
    assert got == samlib.expected_sam(b6, q, REFS, SQ, unmapped=True)
    recs = samlib.records(got)
    with_line = {ln.split("\t")[0] for ln in b6.split("\n") if ln}
    unm = [r for r in recs if int(r[1]) & 4]
    assert len(unm) == len(q) - len(with_line) >= 10 and [r[0] for r in unm] == [samlib.name_of(h) for h, _ in q if h not in with_line]
    assert "Sam: %d records, %d unmapped records" % (len(recs) - len(unm), len(unm)) in text


def test_samples_equal_separate_invocations(mixed_queries, tmp_path):
    lst = tmp_path / "list.txt"
    outs = [str(tmp_path / "a.b6"), str(tmp_path / "b.b6")]
    lst.write_text("%s\t%s\n%s\t%s\n" % (Q100, outs[0], mixed_queries, outs[1]))
    args = ["-m", "ALLPATHS", "-i", "0.95", "-fr", "--sam", "--sam-unmapped"]
    text = run(["-r", EDX, "-ad", "--samples", str(lst)] + args)
    assert "Samples: 2 done, 0 failed" in text and text.count("\nSam: ") == 2
    for k, q in enumerate((Q100, mixed_queries)):
        single = str(tmp_path / ("single%d.b6" % k))
        run(["-r", EDX, "-ad", "-q", q, "-o", single] + args)
        assert open(outs[k] + ".sam", "rb").read() == open(single + ".sam", "rb").read()
        assert open(outs[k], "rb").read() == open(single, "rb").read()


def test_two_ranks_variants_and_fasta(tmp_path):
    base = ["-r", EDX, "-ad", "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr"]
    one, two, var, vs = (str(tmp_path / x) for x in ("one.b6", "two.b6", "var.b6", "vs.b6"))
    run(base + ["-o", one, "--sam"])
    text = run(base + ["-o", two, "--sam", "--gpus", "2", "--devices", "0,0", "--gather", "host"])
    assert "host gather: 2 rank(s)" in text
    assert open(two + ".sam", "rb").read() == open(one + ".sam", "rb").read() and open(two, "rb").read() == open(one, "rb").read()
    # --sam beside --variants: both collectors get the traced groups, the table is unchanged
    run(base + ["-o", var, "--variants", str(tmp_path / "V_"), "--variants-min-depth", "1", "--variants-min-alt", "1"])
    run(base + ["-o", vs, "--variants", str(tmp_path / "W_"), "--variants-min-depth", "1", "--variants-min-alt", "1", "--sam"])
    assert open(str(tmp_path / "V_variants.txt")).read().replace("\tvar\t", "\tvs\t") == open(str(tmp_path / "W_variants.txt")).read()
    assert open(vs + ".sam", "rb").read() == open(one + ".sam", "rb").read()
    # FASTA references
    fa, fac = str(tmp_path / "fa.b6"), str(tmp_path / "fac.b6")
    fbase = ["-r", REFS_FA, "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr", "-s"]
    run(fbase + ["-o", fac, "--cigar"])
    run(fbase + ["-o", fa, "--cigar", "--sam"])
    assert open(fa, "rb").read() == open(fac, "rb").read()
    check_properties(open(fa + ".sam").read(), open(fa).read())
    assert open(fa + ".sam").read() == samlib.expected_sam(open(fa).read(), samlib.fasta(Q100), REFS, SQ)      # header and LN of a FASTA reference too


def test_chimeras_table_is_unchanged(tmp_path):
    """a self-alignment: --sam beside --chimeras"""
    base = ["-r", Q100, "-q", Q100, "-m", "FORAGE", "-i", "0.93"]
    a, b = str(tmp_path / "a.b6"), str(tmp_path / "b.b6")
    run(base + ["-o", a, "--chimeras", str(tmp_path / "A_")])
    run(base + ["-o", b, "--chimeras", str(tmp_path / "B_"), "--sam"])
    assert open(str(tmp_path / "A_chimeras.txt"), "rb").read() == open(str(tmp_path / "B_chimeras.txt"), "rb").read()
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(b + ".sam") > 1000


def test_lengths_table_reaches_the_sq_lines(tmp_path):
    """--sam-lengths: LN comes from the table, whatever the database's own extents say"""
    lens = {h: 100000 + 7 * k for k, (h, _) in enumerate(REFS)}
    table = tmp_path / "len.tsv"
    table.write_text("".join("%s\t%d\n" % kv for kv in lens.items()))
    out = str(tmp_path / "o.b6")
    run(["-r", EDX, "-ad", "-q", Q100, "-m", "BEST", "-i", "0.95", "-o", out, "--cigar", "--sam", "--sam-lengths", str(table)])
    got = open(out + ".sam").read()
    assert got == samlib.expected_sam(open(out).read(), samlib.fasta(Q100), REFS, samlib.sq_of(REFS, lens))
    assert "\tLN:100000\n" in got


def test_python_session(tmp_path):
    """host.Session(sam=True) writes what the command line writes; sam_info() has the sample's figures"""
    from burst_amd import host
    cli_out, ses_out = str(tmp_path / "cli.b6"), str(tmp_path / "ses.b6")
    run(["-r", EDX, "-ad", "-q", Q100, "-o", cli_out, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--sam", "--sam-unmapped"])
    db = host.Db.read(EDX)
    dev = db.open_device(0, build_K=12)
    with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, sam=True, sam_unmapped=True) as s:
        res = s.run(Q100, ses_out)
        assert res["rc"] == 0, res["err"]
        info = s.sam_info()
    assert open(ses_out + ".sam", "rb").read() == open(cli_out + ".sam", "rb").read() and open(ses_out, "rb").read() == open(cli_out, "rb").read()
    recs = samlib.records(open(ses_out + ".sam").read())
    n_unm = sum(1 for r in recs if int(r[1]) & 4)
    assert info["records"] == len(recs) - n_unm > 50 and info["unmapped"] == n_unm and info["device_us"] > 0
    assert info["md_bytes"] >= info["records"]      # (every string ends in a number)
