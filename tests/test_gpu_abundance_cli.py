"""burst_hip --abundance end to end on the MI355X: the .b6 is the bytes of the run without the flag, and the table is what the Python model
(tests/emlib.py) writes from that .b6 TEXT (read = column 1, header = column 2) -- which is what proves the grouping under -fr and for
duplicate reads; together with --coverage, --cigar and --samples; host.Session(abundance=)."""
import os
import re
import subprocess

import numpy as np
import pytest

import emlib as em
import goldenlib as gl

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
Q100, Q292 = os.path.join(gl.G, "q100.fa"), os.path.join(gl.G, "q292.fa")


def run(args, expect=0):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == expect, r.stdout[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def acx(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("acx") / "dna.acx")
    subprocess.check_call([CLI, "-r", EDX, "--make-acx", path], stdout=subprocess.DEVNULL)
    return path


def model_table(b6_text, name, max_iters=1000, tol=1024):
    headers, gw, ln, _ = em.b6_groups(b6_text)
    counts, info = em.em(len(headers), gw, ln, max_iters, tol)
    return em.table_text(headers, [name], [counts]), info


def abundance_line(text):
    m = re.findall(r"^Abundance: (\d+) reads, (\d+) pairs, (\d+) classes, (\d+) iterations, (converged|not converged) \(last delta (\d+)\), device ([0-9.]+) ms$", text, re.M)
    assert m, text[-2000:]
    return m


def read_table(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    return rows[0], {r[0]: r[1:] for r in rows[1:]}


@pytest.mark.parametrize("accel", ["acx", "ad"])
def test_allpaths_table_is_the_models(acx, accel, tmp_path):
    base = ["-r", EDX, "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr"] + (["-a", acx] if accel == "acx" else ["-ad"])
    plain, out, P = str(tmp_path / "plain.b6"), str(tmp_path / "sample_one.b6"), str(tmp_path / "P_")
    assert "Abundance" not in run(base + ["-o", plain])
    text = run(base + ["-o", out, "--abundance", P])
    assert open(out, "rb").read() == open(plain, "rb").read()
    assert sorted(open(out, "rb").read().splitlines()) == gl.golden_lines([c for c in gl.cases() if c["name"] == "dna_q100_allpaths_fr"][0])
    want, info = model_table(open(out).read(), "sample_one")
    assert open(P + "abundance.txt").read() == want
    (reads, pairs, classes, iters, conv, delta, _), = abundance_line(text)
    assert (int(reads), int(classes), int(iters), conv, int(delta)) == (497, 94, 10, "converged", 299)
    assert info == [10, 578, 94, 299, 1]
    assert 94 <= int(pairs) <= 578      # (the groups are the unique queries: reads of equal sequence are one group of their number as weight)
    assert sorted(os.listdir(str(tmp_path))) == ["P_abundance.txt", "plain.b6", "sample_one.b6"]


def test_iterations_and_tolerance_flags(tmp_path):
    base = ["-r", EDX, "-ad", "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr"]
    out, P = str(tmp_path / "o.b6"), str(tmp_path / "P")
    text = run(base + ["-o", out, "--abundance", P, "--abundance-iters", "3", "--abundance-tol", "0"])
    want, info = model_table(open(out).read(), "o", 3, 0)
    assert open(P + "abundance.txt").read() == want and info[0] == 3 and info[4] == 0
    (_, _, _, iters, conv, delta, _), = abundance_line(text)
    assert (int(iters), conv, int(delta)) == (3, "not converged", info[3])


@pytest.mark.parametrize("mode", ["BEST", "CAPITALIST", "ANY"])
def test_one_line_per_read_equals_the_counts(mode, tmp_path):
    """with one line per read the loop stops at once and the table is PREFIXcounts.txt cell for cell (BEST with --coverage beside it)"""
    out, P = str(tmp_path / "o.b6"), str(tmp_path / "P")
    text = run(["-r", EDX, "-ad", "-q", Q100, "-m", mode, "-i", "0.95", "-fr", "-o", out, "--coverage", P, "--abundance", P])
    (_, pairs, classes, iters, conv, delta, _), = abundance_line(text)
    assert conv == "converged" and int(delta) == 0 and int(iters) <= 2
    head_a, rows_a = read_table(P + "abundance.txt")
    head_c, rows_c = read_table(P + "counts.txt")
    assert head_a == head_c == ["#OTU ID", "Dataset", "o"]
    assert sorted(rows_a) == sorted(rows_c) and len(rows_a) > 20
    for name, cells in rows_a.items():
        assert all(re.fullmatch(r"\d+\.0000", c) for c in cells)
        assert [int(float(c)) for c in cells] == [int(c) for c in rows_c[name]]
    want, _ = model_table(open(out).read(), "o")
    assert open(P + "abundance.txt").read() == want


def test_forage_and_two_ranks(tmp_path):
    """FORAGE: every placement of a read is a candidate; two ranks on one device with the host gather: the table is rank 0's"""
    for k, extra in enumerate((["-m", "FORAGE"], ["-m", "ALLPATHS", "--gpus", "2", "--devices", "0,0", "--gather", "host"])):
        out, P = str(tmp_path / ("o%d.b6" % k)), str(tmp_path / ("P%d_" % k))
        text = run(["-r", EDX, "-ad", "-q", Q100, "-i", "0.95", "-fr", "-o", out, "--abundance", P] + extra)
        want, info = model_table(open(out).read(), "o%d" % k)
        assert open(P + "abundance.txt").read() == want
        (_, pairs, classes, iters, _, _, _), = abundance_line(text)
        assert [int(iters), int(classes)] == [info[0], info[2]] and info[2] <= int(pairs) <= info[1]


def test_samples_with_a_failed_one(tmp_path):
    lst = tmp_path / "list.txt"
    outs = [str(tmp_path / n) for n in ("a.b6", "gone.b6", "c.b6")]
    lst.write_text("%s\t%s\n%s\t%s\n%s\t%s\n" % (Q100, outs[0], str(tmp_path / "missing.fa"), outs[1], Q292, outs[2]))
    P = str(tmp_path / "S_")
    text = run(["-r", EDX, "-ad", "--samples", str(lst), "-m", "ALLPATHS", "-i", "0.95", "-fr", "--abundance", P], expect=2)      # (cannot open: the failed sample's code)
    assert "Samples: 2 done, 1 failed" in text and "abundance: sample 'gone' failed alone" in text
    assert len(abundance_line(text)) == 2
    assert not os.path.exists(outs[1])
    cols = []
    for o in (outs[0], outs[2]):
        headers, gw, ln, _ = em.b6_groups(open(o).read())
        counts, _ = em.em(len(headers), gw, ln, 1000, 1024)
        cols.append(dict(zip(headers, counts)))
    allh = sorted(set(cols[0]) | set(cols[1]), key=lambda s: s.encode())
    want = em.table_text(allh, ["a", "gone", "c"], [[cols[0].get(h, 0) for h in allh], [0] * len(allh), [cols[1].get(h, 0) for h in allh]])
    got = open(P + "abundance.txt").read()
    assert got == want
    head, rows = read_table(P + "abundance.txt")
    assert head == ["#OTU ID", "Dataset", "a", "gone", "c"] and all(r[2] == "0.0000" for r in rows.values())


def test_cigar_beside_it_changes_nothing(tmp_path):
    base = ["-r", EDX, "-ad", "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr"]
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir(); d2.mkdir()
    run(base + ["-o", str(d1 / "o.b6"), "--abundance", str(d1 / "P")])
    text = run(base + ["-o", str(d2 / "o.b6"), "--abundance", str(d2 / "P"), "--cigar", "--coverage", str(d2 / "P")])
    assert "\nPaths: " in text and "\nCoverage: " in text and len(abundance_line(text)) == 1
    assert open(str(d1 / "Pabundance.txt"), "rb").read() == open(str(d2 / "Pabundance.txt"), "rb").read()
    a, b = open(str(d1 / "o.b6")).read().splitlines(), open(str(d2 / "o.b6")).read().splitlines()
    assert len(a) == len(b) == 588
    for x, y in zip(a, b):
        assert len(y.split("\t")) == 14 and y.split("\t")[:12] == x.split("\t")


def test_python_session(tmp_path):
    """host.Session(abundance=): abundance() returns the integer columns, close() writes the table"""
    from burst_amd import host
    db = host.Db.read(EDX)
    dev = db.open_device(0, build_K=12)
    outs, P = [str(tmp_path / "x.b6"), str(tmp_path / "y.b6")], str(tmp_path / "py_")
    with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, abundance=P, abundance_iters=50, abundance_tol=16) as s:
        for q, o in zip((Q100, Q292), outs):
            res = s.run(q, o)
            assert res["rc"] == 0, res["err"]
        cols = s.abundance()
        last = s.abundance_info()
    import ctypes as C
    ref_head = C.cast(db.c.refHead, C.POINTER(C.c_char_p))
    heads = {int(db.c.refMap[i]): ref_head[i].decode() for i in range(db.c.origTotR)}
    assert cols.shape == (3, db.c.numRefHeads) and (cols[0] == cols[1] + cols[2]).all()
    for k, o in enumerate(outs):
        headers, gw, ln, _ = em.b6_groups(open(o).read())
        counts, info = em.em(len(headers), gw, ln, 50, 16)
        got = {heads[h]: int(v) for h, v in enumerate(cols[k + 1]) if v}
        assert got == {h: c for h, c in zip(headers, counts) if c}
    assert [last[k] for k in ("iterations", "classes", "delta", "converged")] == [info[0]] + info[2:] and info[2] <= last["pairs"] <= info[1]
    assert open(P + "abundance.txt").read().startswith("#OTU ID\tDataset\tx\ty\n")
    # a pair of mate files is refused by a session with an abundance, before anything runs
    s = host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, abundance=str(tmp_path / "m_"))
    res = s.run(Q100, str(tmp_path / "m.b6"), mates=Q292)
    s.close()
    assert res["rc"] == host.E_USAGE and "abundance" in res["err"] and not os.path.exists(str(tmp_path / "m.b6"))
