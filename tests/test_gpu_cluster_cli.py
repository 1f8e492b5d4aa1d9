"""burst_hip --cluster end to end on the MI355X: a generated FASTA of amplicon-like families aligned against itself in FORAGE; the .b6 is
the bytes of the run without the flag, and both tables are what the Python model (tests/clusterlib.py) writes from that .b6 TEXT; FASTA
and .edx references, --cluster-sizes, two ranks with the host gather, --cigar beside it, duplicate names, host.Session(cluster=)."""
import os
import re
import subprocess

import numpy as np
import pytest

import clusterlib as cl
import goldenlib as gl

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")


def run(args, expect=0):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == expect, r.stdout[-3000:]
    return r.stdout


def write_reads(path, duplicate_name=False):
    """four families of 13 reads of 120 bases, 0-3 substitutions from the family's base (random bases differ in about 90 positions);
    two exact copies of other reads; a read of 100 bases contained in a longer one; a read alone.  Every third read carries a size."""
    rng = np.random.default_rng(11)
    seqs = []
    for _ in range(4):
        base = rng.integers(0, 4, size=120)
        for k in range(13):
            s = base.copy()
            for p in rng.choice(120, size=k % 4, replace=False):
                s[p] = (s[p] + 1 + rng.integers(0, 3)) % 4
            seqs.append(s)
    seqs += [seqs[5].copy(), seqs[30].copy(), seqs[17][10:110].copy(), rng.integers(0, 4, size=120)]
    order = rng.permutation(len(seqs))
    names = []
    with open(path, "w") as f:
        for n, k in enumerate(order):
            name = "read%02d" % n + (";size=%d" % (2 + n % 5) if n % 3 == 0 else ";size=7;" if n % 3 == 1 and n % 2 else "")
            if duplicate_name and n == 40:
                name = names[3]
            names.append(name)
            f.write(">%s\n%s\n" % (name, "".join("ACGT"[b] for b in seqs[k])))
    return names


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    fa = str(d / "reads.fa")
    names = write_reads(fa)
    assert len(names) == 56 and cl.read_fasta_names(fa) == names
    return fa, names


@pytest.fixture(scope="module")
def edx(reads, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("edx") / "reads.edx")
    run(["-r", reads[0], "-d", "QUICK", "130", "-o", path, "-i", "0.95"])
    return path


def clusters_line(text):
    m = re.findall(r"^Clusters: (\d+) reads, (\d+) lines, (\d+) foreign lines, (\d+) edges kept, (\d+) centroids, (\d+) rounds, device ([0-9.]+) ms$", text, re.M)
    assert len(m) == 1, text[-2000:]
    return [int(x) for x in m[0][:6]]


def check_tables(prefix, names, b6_text, sizes):
    a, b = cl.tables_from_b6(names, b6_text, sizes)
    assert open(prefix + "clusters.txt").read() == a and open(prefix + "cluster_sizes.txt").read() == b
    rows = [r.split("\t") for r in b.splitlines()[1:]]
    assert len(rows) not in (1, len(names))
    w = [cl.weight_of(nm, sizes) for nm in names]
    assert sum(int(r[2]) for r in rows) == sum(w) and sum(int(r[1]) for r in rows) == len(names)
    return len(rows)


@pytest.mark.parametrize("ref", ["fasta", "edx"])
def test_tables_are_the_models(reads, edx, ref, tmp_path):
    fa, names = reads
    base = (["-r", fa] if ref == "fasta" else ["-r", edx, "-ad"]) + ["-q", fa, "-m", "FORAGE", "-i", "0.95", "-fr"]
    plain, out, outs, P, S = (str(tmp_path / n) for n in ("plain.b6", "self.b6", "sized.b6", "P.", "S."))
    assert "Clusters" not in run(base + ["-o", plain])
    text = run(base + ["-o", out, "--cluster", P])
    b6 = open(out).read()
    assert open(out, "rb").read() == open(plain, "rb").read() and len(b6) > 0
    n_centroids = check_tables(P, names, b6, False)
    _, edges, lines, foreign = cl.from_b6(names, b6, False)
    got = clusters_line(text)
    assert got[:3] == [len(names), lines, foreign] == [56, len(b6.splitlines()), 0] and got[4] == n_centroids and got[5] >= 1
    assert got[3] <= len(set((q, r) for q, r, _ in edges))
    assert n_centroids >= 5      # four families more than the budget apart and the read alone: no line joins two of them
    text = run(base + ["-o", outs, "--cluster", S, "--cluster-sizes"])
    assert open(outs, "rb").read() == open(plain, "rb").read()
    check_tables(S, names, b6, True)
    assert open(S + "clusters.txt").read() != open(P + "clusters.txt").read().replace("P.", "S.")      # the sizes change the priorities
    assert sorted(os.listdir(str(tmp_path))) == ["P.cluster_sizes.txt", "P.clusters.txt", "S.cluster_sizes.txt", "S.clusters.txt", "plain.b6", "self.b6", "sized.b6"]


def test_contained_read_and_exact_copies(reads, tmp_path):
    """the edges are directed: the read of 100 bases has a line against the read that contains it, never the other way round; exact copies
    name each other with 0 edits"""
    fa, names = reads
    out, P = str(tmp_path / "o.b6"), str(tmp_path / "P.")
    run(["-r", fa, "-q", fa, "-m", "FORAGE", "-i", "0.95", "-fr", "-o", out, "--cluster", P])
    lens = {}
    for ln in open(fa):
        if ln.startswith(">"):
            cur = ln[1:].strip()
        else:
            lens[cur] = len(ln.strip())
    short = [nm for nm in names if lens[nm] == 100]
    assert len(short) == 1
    pairs = {(c[0], c[1]): int(c[10]) for c in (ln.split("\t") for ln in open(out).read().splitlines())}
    assert any(q == short[0] and r != q for q, r in pairs) and not any(r == short[0] and q != r for q, r in pairs)
    zero = [(q, r) for (q, r), e in pairs.items() if q != r and e == 0 and lens[q] == lens[r] == 120]
    assert len(zero) >= 4 and all((r, q) in zero for q, r in zero)


def test_two_ranks_and_cigar(reads, edx, tmp_path):
    fa, names = reads
    base = ["-r", fa, "-q", fa, "-m", "FORAGE", "-i", "0.95", "-fr"]
    one, two, cg = (tmp_path / n for n in ("one", "two", "cigar"))
    for d in (one, two, cg):
        d.mkdir()
    run(base + ["-o", str(one / "o.b6"), "--cluster", str(one / "P.")])
    text = run(base + ["-o", str(two / "o.b6"), "--cluster", str(two / "P."), "--gpus", "2", "--devices", "0,0"])
    assert "host gather: 2 rank(s)" in text
    clusters_line(text)
    assert open(str(one / "o.b6"), "rb").read() == open(str(two / "o.b6"), "rb").read()
    for t in ("P.clusters.txt", "P.cluster_sizes.txt"):
        assert open(str(one / t), "rb").read() == open(str(two / t), "rb").read()
    # --cigar beside it: two more columns per line, the tables still the model's from columns 1, 2 and 11
    run(["-r", edx, "-ad", "-q", fa, "-m", "FORAGE", "-i", "0.95", "-fr", "-o", str(cg / "o.b6"), "--cluster", str(cg / "P."), "--cigar"])
    b6 = open(str(cg / "o.b6")).read()
    assert b6 and all(len(ln.split("\t")) == 14 for ln in b6.splitlines())
    check_tables(str(cg / "P."), names, b6, False)


def test_duplicate_names_exit_1_and_leave_no_table(tmp_path):
    fa = str(tmp_path / "dup.fa")
    names = write_reads(fa, duplicate_name=True)
    text = run(["-r", fa, "-q", fa, "-m", "FORAGE", "-i", "0.95", "-o", str(tmp_path / "o.b6"), "--cluster", str(tmp_path / "P.")], expect=1)
    assert "ERROR: --cluster needs every read named once" in text and "reads 4 and 41" in text and "'%s'" % names[3] in text
    assert sorted(os.listdir(str(tmp_path))) == ["dup.fa", "o.b6"]


def test_python_session(reads, edx, tmp_path):
    """host.Session(cluster=): clusters() returns (centroid, edits) per read in file order, the tables are written with the sample"""
    from burst_amd import host
    fa, names = reads
    db = host.Db.read(edx)
    dev = db.open_device(0, build_K=12)
    out, P = str(tmp_path / "s.b6"), str(tmp_path / "py.")
    with host.Session(db, dev, mode="FORAGE", thres=0.95, rc=True, accel=True, K=12, cluster=P, cluster_sizes=True) as s:
        res = s.run(fa, out)
        assert res["rc"] == 0, res["err"]
        centroid, edits = s.clusters()
        info = s.clusters_info()
    b6 = open(out).read()
    w, e, lines, foreign = cl.from_b6(names, b6, True)
    assert (centroid.tolist(), edits.tolist()) == cl.cluster(w, e)
    assert (info["nodes"], info["lines"], info["foreign"]) == (len(names), lines, foreign)
    check_tables(P, names, b6, True)
