"""burst_hip --taxa end to end on the MI355X: BEST output gives the reference's embalmulate table; ALLPATHS samples give the tables the
Python model (tests/taxalib.py, tests/emlib.py) writes from the .b6 TEXT the run left (read = column 1, header = column 2, taxonomy from the
map's text); every .b6 and the abundance table are the bytes of the run without the flag; two ranks; host.Session(taxa=)."""
import os
import re
import subprocess

import pytest

import emlib as em
import goldenlib as gl
import taxalib as tl

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
TAX = os.path.join(gl.G, "tax.txt")
Q100, Q292 = os.path.join(gl.G, "q100.fa"), os.path.join(gl.G, "q292.fa")


def run(args, expect=0):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == expect, r.stdout[-3000:]
    return r.stdout


def taxa_lines(text):
    m = re.findall(r"^Taxa: (\d+) reads, (\d+) groups, (\d+) pairs, (\d+) reads at the root, deepest level (\d+), device ([0-9.]+) ms$", text, re.M)
    assert m, text[-2000:]
    return [tuple(int(x) for x in t[:5]) for t in m]


def study(b6_texts, names, agree=1000, abundance=False):
    """the model's files (suffix -> text) for the .b6 texts of a study, and per sample info[0..4] with weight-1 groups"""
    tax_map = tl.read_map(open(TAX).read())
    per = [tl.b6_groups(t, tax_map) for t in b6_texts]
    heads = sorted({h for p in per for h in p[0]}, key=lambda s: s.encode())
    hix = {h: i for i, h in enumerate(heads)}
    tnames, parent, depth, hn = tl.tree_of([tax_map.get(h, "") for h in heads])
    own, clade, clade_em, infos = [], [], [], []
    for text, (h, _, gw, lines, _) in zip(b6_texts, per):
        _, o, c, info = tl.taxa(parent, hn, gw, [(g, hix[h[r]]) for g, r in lines], agree)
        own.append(o); clade.append(c); infos.append(info)
        if abundance:
            eh, egw, eln, _ = em.b6_groups(text)
            counts = em.em(len(eh), egw, eln, 1000, 1024)[0]
            full = [0] * len(heads)
            for name, cnt in zip(eh, counts):
                full[hix[name]] = cnt
            clade_em.append(tl.rollup(parent, hn, full)[1])
    return tl.tables(tnames, depth, names, own, clade, clade_em if abundance else None), infos


def files_of(d, prefix):
    return {f[len(prefix):]: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.startswith(prefix) and f.endswith(".txt") and "taxa" in f}


def test_best_equals_the_reference_table(tmp_path):
    out, P = str(tmp_path / "s1.b6"), str(tmp_path / "P_")
    text = run(["-r", EDX, "-ad", "-q", Q100, "-m", "BEST", "-i", "0.95", "-fr", "-b", TAX, "-o", out, "--taxa", P])
    assert sorted(open(out, "rb").read().splitlines()) == gl.golden_lines([c for c in gl.cases() if c["name"] == "dna_q100_best_tax_fr"][0])
    ref = {}
    for ln in open(os.path.join(gl.G, "taxa", "dna_q100_best_tax_fr_taxa.txt")).read().split("\n")[1:]:
        if "\t" in ln:
            name, n = ln.split("\t")
            ref[name or "Unassigned"] = int(n)
    rows = [ln.split("\t") for ln in open(P + "taxa.txt").read().splitlines()]
    assert rows[0] == ["#OTU ID", "Dataset", "s1"] and {(r[0], int(r[2])) for r in rows[1:]} == set(ref.items()) and len(rows) == 42
    (reads, groups, pairs, root, deepest), = taxa_lines(text)
    assert (reads, root, deepest) == (497, 33, 7) and groups == pairs <= 497
    want, _ = study([open(out).read()], ["s1"])
    assert files_of(str(tmp_path), "P_") == want and sorted(want) == ["taxa.txt"] + ["taxa_L%d.txt" % k for k in range(1, 8)]


@pytest.mark.parametrize("agree", [1000, 600])
def test_samples_with_abundance_equal_the_model(tmp_path, agree):
    d0, d1 = tmp_path / "plain", tmp_path / "taxa"
    d0.mkdir(); d1.mkdir()
    texts = []
    for d, extra in ((d0, []), (d1, ["--taxa", str(d1 / "S_")] + (["--taxa-agree", str(agree)] if agree != 1000 else []))):
        lst = d / "list.txt"
        lst.write_text("%s\t%s\n%s\t%s\n" % (Q100, str(d / "a.b6"), Q292, str(d / "c.b6")))
        texts.append(run(["-r", EDX, "-ad", "--samples", str(lst), "-m", "ALLPATHS", "-i", "0.95", "-fr", "-b", TAX, "--abundance", str(d / "S_")] + extra))
    assert "Taxa:" not in texts[0] and "Samples: 2 done, 0 failed" in texts[1]
    for f in ("a.b6", "c.b6", "S_abundance.txt"):      # the flag changes no other output
        assert open(str(d0 / f), "rb").read() == open(str(d1 / f), "rb").read(), f
    assert sorted(open(str(d1 / "a.b6"), "rb").read().splitlines()) == gl.golden_lines([c for c in gl.cases() if c["name"] == "dna_q100_allpaths_tax_fr"][0])
    want, infos = study([open(str(d1 / f)).read() for f in ("a.b6", "c.b6")], ["a", "c"], agree, abundance=True)
    got = files_of(str(d1), "S_")
    assert sorted(got) == sorted(want) and got == want
    assert "taxa_L7.txt" in got and "taxa_abundance_L7.txt" in got
    lines = taxa_lines(texts[1])
    assert len(lines) == 2
    for (reads, groups, pairs, root, deepest), info in zip(lines, infos):      # (the groups are the unique queries: no more of them than reads)
        assert (reads, root, deepest) == (info[2], info[3], info[4]) and groups <= info[1] and pairs <= info[0]
    assert sorted(os.listdir(str(d0))) == ["S_abundance.txt", "a.b6", "c.b6", "list.txt"]


def test_failed_sample_is_a_zero_column(tmp_path):
    lst = tmp_path / "list.txt"
    outs = [str(tmp_path / n) for n in ("a.b6", "gone.b6", "c.b6")]
    lst.write_text("%s\t%s\n%s\t%s\n%s\t%s\n" % (Q100, outs[0], str(tmp_path / "missing.fa"), outs[1], Q292, outs[2]))
    P = str(tmp_path / "S_")
    text = run(["-r", EDX, "-ad", "--samples", str(lst), "-m", "ALLPATHS", "-i", "0.95", "-fr", "-b", TAX, "--taxa", P], expect=2)
    assert "Samples: 2 done, 1 failed" in text and "taxa: sample 'gone' failed alone" in text and len(taxa_lines(text)) == 2
    rows = [ln.split("\t") for ln in open(P + "taxa.txt").read().splitlines()]
    assert rows[0] == ["#OTU ID", "Dataset", "a", "gone", "c"] and all(r[3] == "0" and int(r[1]) == int(r[2]) + int(r[4]) for r in rows[1:])
    want, _ = study([open(outs[0]).read(), "", open(outs[2]).read()], ["a", "gone", "c"])
    assert files_of(str(tmp_path), "S_") == want


def test_two_ranks_and_other_modes(tmp_path):
    """two ranks on one device with the host gather: the tables are rank 0's; FORAGE and CAPITALIST lines through the same groups"""
    for k, extra in enumerate((["-m", "ALLPATHS", "--gpus", "2", "--devices", "0,0", "--gather", "host"], ["-m", "FORAGE"], ["-m", "CAPITALIST"])):
        out, P = str(tmp_path / ("o%d.b6" % k)), str(tmp_path / ("P%d_" % k))
        text = run(["-r", EDX, "-ad", "-q", Q100, "-i", "0.95", "-fr", "-b", TAX, "-o", out, "--taxa", P, "--taxa-agree", "750"] + extra)
        want, (info,) = study([open(out).read()], ["o%d" % k], 750)
        assert files_of(str(tmp_path), "P%d_" % k) == want
        (reads, groups, pairs, root, deepest), = taxa_lines(text)
        assert (reads, root, deepest) == (info[2], info[3], info[4])


def test_python_session(tmp_path):
    """host.Session(taxa=): taxa() returns the integer columns, close() writes the tables"""
    from burst_amd import host
    db = host.Db.read(EDX)
    dev = db.open_device(0, build_K=12)
    outs, P = [str(tmp_path / "x.b6"), str(tmp_path / "y.b6")], str(tmp_path / "py_")
    with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, taxonomy=TAX, taxa=P, taxa_agree=600, abundance=P) as s:
        for q, o in zip((Q100, Q292), outs):
            res = s.run(q, o)
            assert res["rc"] == 0, res["err"]
        t = s.taxa()
        last = s.taxa_info()
    assert t["own"].shape == (3, len(t["names"])) and (t["own"][0] == t["own"][1] + t["own"][2]).all() and t["names"][0] == b"Unassigned"
    assert tl.is_preorder(t["parent"].tolist()) and t["depth"].tolist() == tl.depths(t["parent"].tolist())
    assert t["clade"][:, 0].tolist() == [int(t["own"][c].sum()) for c in range(3)] and t["clade_em"][1, 0] == int(t["clade"][1, 0]) << 30
    want, infos = study([open(o).read() for o in outs], ["x", "y"], 600, abundance=True)
    assert files_of(str(tmp_path), "py_") == want
    assert (last["reads"], last["root_reads"], last["deepest"]) == (infos[1][2], infos[1][3], infos[1][4]) and last["device_us"] > 0
    # a pair of mate files is refused by a session with taxon tables, before anything runs
    s = host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, taxonomy=TAX, taxa=str(tmp_path / "m_"))
    res = s.run(Q100, str(tmp_path / "m.b6"), mates=Q292)
    s.close()
    assert res["rc"] == host.E_USAGE and "taxon tables" in res["err"] and not os.path.exists(str(tmp_path / "m.b6"))
