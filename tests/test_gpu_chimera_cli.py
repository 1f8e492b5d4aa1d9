"""burst_hip --chimeras end to end on the MI355X: a generated FASTA of sibling amplicon families with planted two-parent chimeras aligned
against itself in FORAGE; the .b6 is the bytes of the run without the flag, and the table is what the Python model (tests/chimeralib.py)
writes from the TEXT of the same command with --cigar; FASTA and .edx references, --cigar and --cluster beside it, two ranks with the host
gather, duplicate names, host.Session(chimeras=).

The identity cutoff is 0.93, not the 0.95 of the clustering tests: the chimera A[:40] + B[40:] differs from A in the 9 sibling positions
from 40 on, and 150 bases at 0.95 allow 7 edits -- its line towards A, which the two-parent model needs, would not be printed.  0.93 allows
10: every planted read aligns end to end against both parents (6 + 6 and 9 + 3 edits), and the siblings (12 apart) still do not see each
other.  The definition is untouched."""
import os
import re
import subprocess

import numpy as np
import pytest

import chimeralib as ml
import goldenlib as gl

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
CUTOFF = "0.93"


def run(args, expect=0):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == expect, r.stdout[-3000:]
    return r.stdout


def revcomp(s):
    return [3 - b for b in reversed(s)]


def write_reads(path, duplicate_name=False):
    """three pairs of sibling families of 150-base reads: the siblings' bases differ in 12 evenly spread positions; per family the base
    (`;size=9`) and four reads 1 .. 3 substitutions away (no size); per pair the chimeras A[:75] + B[75:] and A[:40] + B[40:] (`;size=1`),
    the second written as its reverse complement; an exact copy of the first pair's first chimera; a read alone.  Returns the names in
    file order and those of the planted reads"""
    rng = np.random.default_rng(23)
    seqs, kind = [], []
    for pair in range(3):
        a = rng.integers(0, 4, size=150)
        b = a.copy()
        for p in range(6, 150, 12)[:12]:
            b[p] = (b[p] + 1 + rng.integers(0, 3)) % 4
        assert int((a != b).sum()) == 12
        for base in (a, b):
            seqs.append(base.tolist()); kind.append("parent")
            for k in range(4):
                s = base.copy()
                for p in rng.choice(150, size=1 + k % 3, replace=False):
                    s[p] = (s[p] + 1 + rng.integers(0, 3)) % 4
                seqs.append(s.tolist()); kind.append("family")
        seqs.append(a[:75].tolist() + b[75:].tolist()); kind.append("chimera")
        seqs.append(revcomp(a[:40].tolist() + b[40:].tolist())); kind.append("chimera")
        if pair == 0:
            seqs.append(a[:75].tolist() + b[75:].tolist()); kind.append("chimera")
    seqs.append(rng.integers(0, 4, size=150).tolist()); kind.append("alone")
    order = rng.permutation(len(seqs))
    names, planted = [], []
    with open(path, "w") as f:
        for n, k in enumerate(order):
            name = "read%02d" % n + {"parent": ";size=9", "chimera": ";size=1;" if n % 2 else ";size=1"}.get(kind[k], "")
            if duplicate_name and n == 30:
                name = names[3]
            names.append(name)
            if kind[k] == "chimera":
                planted.append(name)
            f.write(">%s\n%s\n" % (name, "".join("ACGT"[b] for b in seqs[k])))
    return names, planted


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    fa = str(d / "reads.fa")
    names, planted = write_reads(fa)
    assert len(names) == 38 and len(planted) == 7 and ml.read_fasta_names(fa) == names
    return fa, names, planted


@pytest.fixture(scope="module")
def edx(reads, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("edx") / "reads.edx")
    run(["-r", reads[0], "-d", "QUICK", "160", "-o", path, "-i", CUTOFF])
    return path


def chimeras_line(text):
    m = re.findall(r"^Chimeras: (\d+) reads, (\d+) lines, (\d+) foreign lines, (\d+) pairs kept, (\d+) reads evaluated, (\d+) chimeric, device ([0-9.]+) ms$", text, re.M)
    assert len(m) == 1, text[-2000:]
    return [int(x) for x in m[0][:6]]


def check_table(prefix, names, planted, cigar_text):
    """the table is the model's from the --cigar text; every planted chimera is Y with Model 0, no other read is Y"""
    want = ml.table_from_b6(names, cigar_text, True)
    got = open(prefix + "chimeras.txt").read()
    assert got == want
    rows = {r[0]: r for r in (ln.split("\t") for ln in got.splitlines()[1:])}
    assert list(rows) == names
    for nm in planted:
        assert rows[nm][1] == "Y" and rows[nm][3] == "0" and rows[nm][5] != rows[nm][7], rows[nm]
    assert sorted(nm for nm in names if rows[nm][1] == "Y") == sorted(planted)
    return rows


@pytest.mark.parametrize("ref", ["fasta", "edx"])
def test_table_is_the_models(reads, edx, ref, tmp_path):
    fa, names, planted = reads
    base = (["-r", fa] if ref == "fasta" else ["-r", edx, "-ad"]) + ["-q", fa, "-m", "FORAGE", "-i", CUTOFF, "-fr"]
    plain, out, cg, cgc, P, C = (str(tmp_path / n) for n in ("plain.b6", "self.b6", "cigar.b6", "cigar_chim.b6", "P.", "C."))
    assert "Chimeras" not in run(base + ["-o", plain])
    text = run(base + ["-o", out, "--chimeras", P, "--chimera-sizes"])
    assert open(out, "rb").read() == open(plain, "rb").read() and os.path.getsize(out) > 0      # 12 columns, nothing traced into the file
    assert "Paths:" not in text
    run(base + ["-o", cg, "--cigar"])
    cigar_text = open(cg).read()
    assert all(len(ln.split("\t")) == 14 for ln in cigar_text.splitlines())
    rows = check_table(P, names, planted, cigar_text)
    w, lens, lines, ops, printed, foreign = ml.from_b6(names, cigar_text, True)
    want, kept = ml.chimera(w, lens, lines, ops)
    got = chimeras_line(text)
    assert got == [len(names), printed, foreign, kept, sum(1 for r in want if r[0]), len(planted)] and foreign == 0 and printed == len(open(plain).read().splitlines())
    assert any(int(c[8]) > int(c[9]) for c in (ln.split("\t") for ln in cigar_text.splitlines()) if c[0] in planted)      # reverse lines took part
    # A[:75] + B[75:]: its line towards B has its last X on symbol 66, the one towards A its first on symbol 78 -- Model 0 from cut 67 on
    copies = [nm for nm in planted if rows[nm][4] == "67"]
    assert len(copies) == 4      # three pairs and the exact copy, which carries its unique query's path
    # --cigar beside it: the file is the --cigar run's, the table the same
    text = run(base + ["-o", cgc, "--cigar", "--chimeras", C, "--chimera-sizes"])
    assert open(cgc, "rb").read() == open(cg, "rb").read() and "Paths:" in text
    assert open(C + "chimeras.txt").read() == open(P + "chimeras.txt").read()
    # the policy options reach the definition
    text = run(base + ["-o", out, "--chimeras", C, "--chimera-sizes", "--chimera-skew", "9", "--chimera-min-seg", "50", "--chimera-min-gain", "7"])
    assert open(C + "chimeras.txt").read() == ml.table_from_b6(names, cigar_text, True, skew=9, min_seg=50, min_gain=7) != open(P + "chimeras.txt").read()
    assert sorted(os.listdir(str(tmp_path))) == ["C.chimeras.txt", "P.chimeras.txt", "cigar.b6", "cigar_chim.b6", "plain.b6", "self.b6"]


def test_unit_weights_evaluate_nobody(reads, tmp_path):
    """without --chimera-sizes every read weighs 1 and S = 2 leaves no candidate parent; with --chimera-skew 1 every other read is one"""
    fa, names, _ = reads
    base = ["-r", fa, "-q", fa, "-m", "FORAGE", "-i", CUTOFF, "-fr"]
    run(base + ["-o", str(tmp_path / "cg.b6"), "--cigar"])
    cigar_text = open(str(tmp_path / "cg.b6")).read()
    text = run(base + ["-o", str(tmp_path / "o.b6"), "--chimeras", str(tmp_path / "U.")])
    assert chimeras_line(text)[3:] == [0, 0, 0]
    assert open(str(tmp_path / "U.chimeras.txt")).read() == ml.table_from_b6(names, cigar_text, False)
    text = run(base + ["-o", str(tmp_path / "o.b6"), "--chimeras", str(tmp_path / "V."), "--chimera-skew", "1"])
    assert chimeras_line(text)[4] > 7
    assert open(str(tmp_path / "V.chimeras.txt")).read() == ml.table_from_b6(names, cigar_text, False, skew=1)


def test_two_ranks_and_cluster(reads, tmp_path):
    fa, names, planted = reads
    base = ["-r", fa, "-q", fa, "-m", "FORAGE", "-i", CUTOFF, "-fr"]
    one, two, clu, both = (tmp_path / n for n in ("one", "two", "clu", "both"))
    for d in (one, two, clu, both):
        d.mkdir()
    run(base + ["-o", str(one / "o.b6"), "--chimeras", str(one / "P."), "--chimera-sizes"])
    text = run(base + ["-o", str(two / "o.b6"), "--chimeras", str(two / "P."), "--chimera-sizes", "--gpus", "2", "--devices", "0,0"])
    assert "host gather: 2 rank(s)" in text
    assert chimeras_line(text)[5] == len(planted)
    assert open(str(one / "o.b6"), "rb").read() == open(str(two / "o.b6"), "rb").read()
    assert open(str(one / "P.chimeras.txt"), "rb").read() == open(str(two / "P.chimeras.txt"), "rb").read()
    # --cluster beside it: its two tables are those of the run without --chimeras
    run(base + ["-o", str(clu / "o.b6"), "--cluster", str(clu / "P."), "--cluster-sizes"])
    text = run(base + ["-o", str(both / "o.b6"), "--cluster", str(both / "P."), "--cluster-sizes", "--chimeras", str(both / "P."), "--chimera-sizes"])
    assert "Clusters:" in text and chimeras_line(text)[5] == len(planted)
    for t in ("P.clusters.txt", "P.cluster_sizes.txt"):
        assert open(str(clu / t), "rb").read() == open(str(both / t), "rb").read()
    assert open(str(both / "P.chimeras.txt"), "rb").read() == open(str(one / "P.chimeras.txt"), "rb").read()
    assert open(str(both / "o.b6"), "rb").read() == open(str(one / "o.b6"), "rb").read()


def test_duplicate_names_exit_1_and_leave_no_table(tmp_path):
    fa = str(tmp_path / "dup.fa")
    names, _ = write_reads(fa, duplicate_name=True)
    text = run(["-r", fa, "-q", fa, "-m", "FORAGE", "-i", CUTOFF, "-o", str(tmp_path / "o.b6"), "--chimeras", str(tmp_path / "P.")], expect=1)
    assert "ERROR: --chimeras needs every read named once" in text and "reads 4 and 31" in text and "'%s'" % names[3] in text
    assert sorted(os.listdir(str(tmp_path))) == ["dup.fa", "o.b6"]


def test_python_session(reads, edx, tmp_path):
    """host.Session(chimeras=): chimeras() returns a row per read in file order, the table is written with the sample"""
    from burst_amd import host
    fa, names, planted = reads
    run(["-r", edx, "-ad", "-q", fa, "-m", "FORAGE", "-i", CUTOFF, "-fr", "-o", str(tmp_path / "cg.b6"), "--cigar"])
    cigar_text = open(str(tmp_path / "cg.b6")).read()
    db = host.Db.read(edx)
    dev = db.open_device(0, build_K=12)
    out, P = str(tmp_path / "s.b6"), str(tmp_path / "py.")
    with host.Session(db, dev, mode="FORAGE", thres=float(CUTOFF), rc=True, accel=True, K=12, chimeras=P, chimera_sizes=True) as s:
        res = s.run(fa, out)
        assert res["rc"] == 0, res["err"]
        rows = s.chimeras()
        info = s.chimeras_info()
    assert all(len(ln.split("\t")) == 12 for ln in open(out).read().splitlines())
    w, lens, lines, ops, printed, foreign = ml.from_b6(names, cigar_text, True)
    want, kept = ml.chimera(w, lens, lines, ops)
    assert ml.rows_of(rows) == want
    assert (info["nodes"], info["lines"], info["foreign"], info["pairs_kept"], info["chimeric"]) == (len(names), printed, foreign, kept, len(planted))
    check_table(P, names, planted, cigar_text)
