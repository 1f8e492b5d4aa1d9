"""burst_hip --variants end to end on the MI355X: the table against the one pilelib builds by replaying the printed CIGARs over
tests/golden/refs.fa and the query file (nothing of the project is involved in that replay), byte for byte; the .b6 with the flag alone
is the .b6 without it; a study of two samples; --variants-reads unique; the default thresholds."""
import os
import subprocess

import numpy as np
import pytest

import cigarlib as cg
import goldenlib as gl
import pilelib

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
DB = os.path.join(gl.G, "dna.edx")
Q100 = os.path.join(gl.G, "q100.fa")
REFS = {name: seq for name, seq in pilelib.read_fasta(os.path.join(gl.G, "refs.fa"))}
LOOSE = ["--variants-min-depth", "1", "--variants-min-alt", "1"]


def run(args):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def with_edited_reads(tmp_path):
    """q100.fa and three reads with one interior insertion each, cut from the first reference"""
    rng = np.random.default_rng(21)
    name, seq = next((n, s) for n, s in REFS.items() if len(s) >= 700 and set(s[:700].upper()) <= set("ACGT"))
    codes = np.array([pilelib.CODE[c] for c in seq[:700]], np.uint8)
    path = str(tmp_path / "q100_edited.fa")
    with open(path, "w") as f:
        f.write(open(Q100).read())
        for k in range(3):
            read = cg.edit_read(rng, codes, 100 + 150 * k, 100, 0, 1, 0)
            f.write(">edited_%d\n%s\n" % (k, "".join(pilelib.LETTERS[c] for c in read)))
    return path


def model_table(samples, min_depth, min_alt, unique_only=False):
    """samples = [(output with the --cigar columns, query file)] in study order"""
    blocks = []
    for out, qfile in samples:
        queries = {n: s for n, s in pilelib.read_fasta(qfile)}
        lines = pilelib.lines_of_b6(open(out).read(), REFS, queries, unique_only)
        rows = pilelib.reported(pilelib.pile(lines), min_depth, min_alt)
        assert rows, "the model finds no site to report"
        blocks.append((os.path.splitext(os.path.basename(out))[0], rows))
    return pilelib.table(blocks), blocks


@pytest.mark.parametrize("mode", ["BEST", "ALLPATHS"])
def test_table_is_the_replay_of_the_printed_cigars(tmp_path, mode):
    qfile = with_edited_reads(tmp_path)
    base = ["-r", DB, "-ad", "-q", qfile, "-m", mode, "-i", "0.95", "-fr"]
    plain, alone, both = (str(tmp_path / n) for n in ("plain.b6", "alone.b6", "both.b6"))
    run(base + ["-o", plain])
    text = run(base + ["-o", alone, "--variants", str(tmp_path / "A_")] + LOOSE)
    assert "\nVariants: " in text and "\nPaths: " not in text
    assert open(alone, "rb").read() == open(plain, "rb").read()      # the flag alone leaves the .b6 as it is
    text = run(base + ["-o", both, "--cigar", "--variants", str(tmp_path / "B_")] + LOOSE)
    assert "\nVariants: " in text and "\nPaths: " in text
    exp, blocks = model_table([(both, qfile)], 1, 1)
    got = open(str(tmp_path / "B_variants.txt"), "rb").read()
    assert got == exp
    assert len(blocks[0][1]) > 20 and any(r[10] for r in blocks[0][1]), "no interior insertion among the rows"
    # the same rows whether or not the lines carry their columns; only the sample's name differs
    strip = lambda b: [ln.split(b"\t")[:3] + ln.split(b"\t")[4:] for ln in b.split(b"\n")]
    assert strip(open(str(tmp_path / "A_variants.txt"), "rb").read()) == strip(got)
    assert sorted(f for f in os.listdir(str(tmp_path)) if "tmp" in f) == []


def test_samples_study_of_two_blocks_in_study_order(tmp_path):
    lst = tmp_path / "list.txt"
    outs = [str(tmp_path / "zz_first.b6"), str(tmp_path / "aa_second.b6")]
    q292 = os.path.join(gl.G, "q292.fa")
    lst.write_text("%s\t%s\n%s\t%s\n" % (Q100, outs[0], q292, outs[1]))
    text = run(["-r", DB, "-ad", "--samples", str(lst), "-m", "BEST", "-i", "0.95", "-fr", "--cigar", "--variants", str(tmp_path / "S_")] + LOOSE)
    assert "Samples: 2 done, 0 failed" in text and text.count("\nVariants: ") == 2
    exp, blocks = model_table([(outs[0], Q100), (outs[1], q292)], 1, 1)
    got = open(str(tmp_path / "S_variants.txt"), "rb").read()
    assert got == exp and [n for n, _ in blocks] == ["zz_first", "aa_second"]
    names = [ln.split("\t")[3] for ln in got.decode().split("\n")[1:] if ln]
    assert names == ["zz_first"] * len(blocks[0][1]) + ["aa_second"] * len(blocks[1][1])


def test_unique_reads_only(tmp_path):
    base = ["-r", DB, "-ad", "-q", Q100, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--cigar"]
    out = str(tmp_path / "u.b6")
    run(base + ["-o", out, "--variants", str(tmp_path / "U_"), "--variants-reads", "unique"] + LOOSE)
    exp_u, blocks_u = model_table([(out, Q100)], 1, 1, unique_only=True)
    exp_all, blocks_all = model_table([(out, Q100)], 1, 1)
    assert open(str(tmp_path / "U_variants.txt"), "rb").read() == exp_u
    assert exp_u != exp_all and blocks_u[0][1], "ALLPATHS prints no read on more than one line: the rule was not exercised"


def test_default_thresholds_on_the_reads_five_times_over(tmp_path):
    qfile = str(tmp_path / "five.fa")
    with open(qfile, "w") as f:
        for k in range(5):
            for name, seq in pilelib.read_fasta(Q100):
                f.write(">%s_copy%d\n%s\n" % (name, k, seq))
    out = str(tmp_path / "five.b6")
    run(["-r", DB, "-ad", "-q", qfile, "-o", out, "-m", "BEST", "-i", "0.95", "-fr", "--cigar", "--variants", str(tmp_path / "D_")])
    exp, blocks = model_table([(out, qfile)], 4, 2)
    assert open(str(tmp_path / "D_variants.txt"), "rb").read() == exp
    assert all(r[3] >= 4 for r in blocks[0][1]) and all(r[3] % 5 == 0 for r in blocks[0][1])


def test_python_session_writes_what_the_command_line_writes(tmp_path):
    """host.Session(variants=...) on the device and with the plain C count (variants_host=True): the command line's table both times"""
    from burst_amd import host
    cli_out = str(tmp_path / "s.b6")
    run(["-r", DB, "-ad", "-q", Q100, "-o", cli_out, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--variants", str(tmp_path / "C_")] + LOOSE)
    want = open(str(tmp_path / "C_variants.txt"), "rb").read()
    assert want.count(b"\n") > 1
    db = host.Db.read(DB)
    dev = db.open_device(0, build_K=12)
    for k, on_host in enumerate((False, True)):
        d = tmp_path / ("ses%d" % k)
        d.mkdir()
        with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, variants=str(d / "P_"), variants_min_depth=1, variants_min_alt=1,
                          variants_host=on_host) as s:
            res = s.run(Q100, str(d / "s.b6"))
            assert res["rc"] == 0, res["err"]
            rows, samples = s.variants()
            assert len(rows) == want.count(b"\n") - 1 and set(samples.tolist()) == {0}
            assert s.variants_info()["sites"] == len(rows) and s.variants_info()["lines"] > 0
        assert open(str(d / "P_variants.txt"), "rb").read() == want
        assert open(str(d / "s.b6"), "rb").read() == open(cli_out, "rb").read()
