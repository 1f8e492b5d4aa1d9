"""burst_hip --cigar end to end on the MI355X.  Per case: without its last two columns the output is the bytes of the run without the
flag (which the golden tests hold to the reference); every line's CIGAR adds up to the line's own columns; and every CIGAR is replayed
over tests/golden/refs.fa from the printed position with the query -- a check that involves none of the project's code."""
import os
import subprocess

import numpy as np
import pytest

import cigarlib as cg
import goldenlib as gl

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
TAX = os.path.join(gl.G, "tax.txt")
EXEMPT_CAP = 0.10      # share of lines whose path's I count may differ from the record's gapR (more than one best end column)

# IUPAC base sets in the code order . A C G T N K M R Y S W B V H D; two symbols cost 0 iff one set contains the other; with N penalised
# (the default, -n) every pair with an N costs 1
CHARS = ".ACGTNKMRYSWBVHD"
SETS = [0, 1, 2, 4, 8, 15, 12, 3, 5, 10, 6, 9, 14, 7, 11, 13]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "K": "M", "M": "K", "R": "Y", "Y": "R", "S": "S", "W": "W", "B": "V", "V": "B", "H": "D", "D": "H"}


def cost(a, b, n_penalised):
    ia, ib = CHARS.index(a) if a in CHARS else 5, CHARS.index(b) if b in CHARS else 5
    if n_penalised and (ia == 5 or ib == 5):
        return 1
    sa, sb = SETS[ia], SETS[ib]
    return 0 if (sa & sb) in (sa, sb) else 1


def fasta(path):
    out, name = {}, None
    for ln in open(path):
        ln = ln.rstrip("\r\n")
        if ln.startswith(">"):
            name = ln[1:]
            out[name] = []
        elif name is not None:
            out[name].append(ln.upper().replace("U", "T"))
    return {k: "".join(v) for k, v in out.items()}


REFS = fasta(os.path.join(gl.G, "refs.fa"))
QUERIES = {f: fasta(os.path.join(gl.G, f)) for f in ("q100.fa", "q292.fa")}


def run(args, expect_paths):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert ("\nPaths: " in r.stdout) == expect_paths, r.stdout[-3000:]
    return r.stdout


def check_lines(with_flag, without, qfile, tax, n_penalised, L, replay=True):
    """with_flag / without: the two outputs' bytes"""
    a, b = with_flag.decode().split("\n"), without.decode().split("\n")
    assert a[-1] == "" and b[-1] == "" and len(a) == len(b) and len(a) > 100
    n_exempt = 0
    for la, lb in zip(a[:-1], b[:-1]):
        body, pos, cigar = la.rsplit("\t", 2)
        assert body == lb
        f = la.split("\t")
        assert len(f) == (15 if tax else 14)
        qlen, st, en, ed, n_mis, n_gap = int(f[7]), int(f[8]), int(f[9]), int(f[10]), int(f[4]), int(f[5])
        pos = int(pos)
        n = {c: 0 for c in "=XID"}
        items = cg.parse_cigar(cigar)
        for k, c in items:
            assert k > 0
            n[c] += k
        assert all(x[1] != y[1] for x, y in zip(items[:-1], items[1:])), "runs are merged"
        assert n["="] + n["X"] + n["I"] == qlen
        assert n["X"] + n["I"] + n["D"] == ed
        assert pos >= 1 and pos + n["="] + n["X"] + n["D"] - 1 == max(st, en)      # the path ends where the line says the placement ends
        query = QUERIES[qfile][f[0]]
        if st > en:
            query = "".join(COMP.get(c, "N") for c in reversed(query))
        ref = REFS[f[1]]
        assert len(query) == qlen
        if replay:
            x, y = pos - 1, 0
            for k, c in items:
                for _ in range(k):
                    if c in "=X":
                        assert cost(query[y], ref[x], n_penalised) == (0 if c == "=" else 1), (la, x, y)
                        x += 1; y += 1
                    elif c == "I":
                        y += 1
                    else:
                        x += 1
            assert y == qlen
        if n["D"] + n["I"] != n_gap or n["X"] != n_mis:
            # allowed only where the last row attains its best (score, H) in more than one end column (the record's gapR is the first
            # such column's, the path ends in the last): the restatement over the placement's surroundings must say so
            n_exempt += 1
            pad = 2 * ed + 4
            lo = max(0, pos - 1 - pad)
            win = ref[lo:max(st, en) + pad]
            code = lambda s: np.array([CHARS.index(c) if c in CHARS else 5 for c in s], np.uint8)
            lut = np.array([255 if not (i and j) else cost(CHARS[i], CHARS[j], n_penalised) for i in range(16) for j in range(16)], np.uint8)
            ok, _, o = cg.trace(L, code(query), code(win), ed, lut, final_pos=max(st, en) - lo)
            assert ok and o.n_same_cols > 1, la
    share = n_exempt / (len(a) - 1)
    print("%d lines, %d (%.1f %%) with more than one best end column" % (len(a) - 1, n_exempt, 100 * share))
    assert share <= EXEMPT_CAP
    return share


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


CASES = [
    ("quick", "q292.fa", "BEST", "0.96", ["-fr", "-ad"]),
    ("quick", "q100.fa", "ALLPATHS", "0.97", ["-fr", "-ad"]),
    ("quick", "q100.fa", "CAPITALIST", "0.97", ["-fr", "-ad"]),
    ("quick", "q100.fa", "FORAGE", "0.96", ["-ad"]),
    ("dna", "q100.fa", "BEST", "0.95", ["-fr", "-ad"]),
    ("dna", "q100.fa", "ALLPATHS", "0.95", ["-fr", "-ad"]),
    ("dna", "q292.fa", "CAPITALIST", "0.95", ["-fr"]),                      # no accelerator: the merged hit list
    ("dna", "q292.fa", "FORAGE", "0.95", ["-fr", "-ad"]),
    ("dna", "q100.fa", "ALLPATHS", "0.95", ["-fr", "-y", "-ad"]),           # N free
    ("fasta", "q100.fa", "ALLPATHS", "0.95", ["-fr", "-s"]),                # FASTA references, sheared
    ("dna", "q100.fa", "BEST", "0.95", ["-fr", "-ad", "-b", TAX]),          # the two columns come behind the taxonomy
    ("dna", "q100.fa", "ALLPATHS", "0.95", ["-fr", "-ad", "--gpus", "2", "--devices", "0,0", "--gather", "host"]),
]


@pytest.mark.parametrize("db,qfile,mode,ident,extra", CASES, ids=["%s_%s_%s_%s" % (c[0], c[1][:-3], c[2], "_".join(x.strip("-") for x in c[4] if x.startswith("-"))) for c in CASES])
def test_cigar_columns(db, qfile, mode, ident, extra, tmp_path, L):
    ref = os.path.join(gl.G, "refs.fa") if db == "fasta" else os.path.join(gl.G, db + ".edx")
    base = ["-r", ref, "-q", os.path.join(gl.G, qfile), "-m", mode, "-i", ident] + extra
    plain, with_flag = str(tmp_path / "plain.b6"), str(tmp_path / "cigar.b6")
    run(base + ["-o", plain], False)
    text = run(base + ["-o", with_flag, "--cigar"], True)
    if "--gpus" in extra:
        assert "host gather: 2 rank(s)" in text
    check_lines(open(with_flag, "rb").read(), open(plain, "rb").read(), qfile, "-b" in extra, "-y" not in extra, L)


def test_samples_study_of_two_files(tmp_path, L):
    lst = tmp_path / "list.txt"
    outs = {}
    for flag in ("plain", "cigar"):
        d = tmp_path / flag
        d.mkdir()
        outs[flag] = [str(d / "a.b6"), str(d / "b.b6")]
        lst.write_text("%s\t%s\n%s\t%s\n" % (os.path.join(gl.G, "q100.fa"), outs[flag][0], os.path.join(gl.G, "q292.fa"), outs[flag][1]))
        text = run(["-r", os.path.join(gl.G, "dna.edx"), "-ad", "--samples", str(lst), "-m", "BEST", "-i", "0.95", "-fr"] + (["--cigar"] if flag == "cigar" else []), flag == "cigar")
        assert "Samples: 2 done, 0 failed" in text
        if flag == "cigar":
            assert text.count("\nPaths: ") == 2
    for k, qfile in enumerate(("q100.fa", "q292.fa")):
        check_lines(open(outs["cigar"][k], "rb").read(), open(outs["plain"][k], "rb").read(), qfile, False, True, L)


def test_python_session_and_report(tmp_path, L):
    """host.Session(cigar=True) writes what the command line writes"""
    from burst_amd import host
    ref = os.path.join(gl.G, "dna.edx")
    cli_out, ses_out = str(tmp_path / "cli.b6"), str(tmp_path / "ses.b6")
    run(["-r", ref, "-ad", "-q", os.path.join(gl.G, "q100.fa"), "-o", cli_out, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--cigar"], True)
    db = host.Db.read(ref)
    dev = db.open_device(0, build_K=12)
    with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, cigar=True) as s:
        res = s.run(os.path.join(gl.G, "q100.fa"), ses_out)
        assert res["rc"] == 0, res["err"]
    assert open(ses_out, "rb").read() == open(cli_out, "rb").read()
