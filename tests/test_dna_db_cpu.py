"""The compressive database build (-d DNA / RNA with -s) on the host restatement of the duplicate marks (BURST_HOST_DNA_MARKS=1):
byte-identical to the reference's databases (tests/golden/dna.edx and the cases of tests/golden/make_golden_dna.py)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
D = os.path.join(G, "dna_cases")
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")
REF = os.path.join(ROOT, "oracle", "_ref", "burst12")
ENV = dict(os.environ, BURST_HOST_DNA_MARKS="1")
CASES = json.load(open(os.path.join(G, "dna_cases.json")))


def run(args, env=ENV):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def acx_sha(name):
    return json.load(open(os.path.join(G, "acx.sha256")))[name]


@pytest.mark.parametrize("mode", ["DNA", "RNA"])
def test_golden_dna_database(tmp_path, mode):
    edx, acx = str(tmp_path / "x.edx"), str(tmp_path / "x.acx")
    r = run(["-r", os.path.join(G, "refs.fa"), "-d", mode, "320", "-o", edx, "-a", acx, "-s", "500", "-i", "0.95"])
    assert r.returncode == 0, r.stdout
    assert "duplicate marks computed on the host" in r.stdout
    assert open(edx, "rb").read() == open(os.path.join(G, "dna.edx"), "rb").read()
    assert sha(acx) == acx_sha("dna.acx")


def test_golden_dna_database_y(tmp_path):
    edx, acx = str(tmp_path / "x.edx"), str(tmp_path / "x.acx")
    r = run(["-r", os.path.join(G, "refs.fa"), "-d", "DNA", "320", "-o", edx, "-a", acx, "-s", "500", "-i", "0.95", "-y"])
    assert r.returncode == 0, r.stdout
    assert open(edx, "rb").read() == open(os.path.join(G, "dna.edx"), "rb").read()
    assert sha(acx) == acx_sha("dna_y.acx")


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_dna_cases(tmp_path, name):
    c = CASES[name]
    edx, acx = str(tmp_path / "x.edx"), str(tmp_path / "x.acx")
    r = run(["-r", os.path.join(D, c["input"]), "-o", edx, "-a", acx] + c["args"])
    assert r.returncode == 0, r.stdout
    got = open(edx, "rb").read()
    if "edx" in c:
        assert got == open(os.path.join(D, c["edx"]), "rb").read()
    else:
        assert hashlib.sha256(got).hexdigest() == c["edx_sha256"]
    assert sha(acx) == c["acx_sha256"]


def test_python_host_entry(tmp_path):
    sys.path.insert(0, ROOT)
    from burst_amd import host
    d = host.Db.from_fasta(os.path.join(G, "refs.fa"), 320, 0.95, 500, layout="DNA", partitions=1)
    assert d.dna_stats.device == -1 and d.dna_stats.W == 836
    out = str(tmp_path / "p.edx")
    d.write(out, db_qlen=320, thres=0.95)
    assert open(out, "rb").read() == open(os.path.join(G, "dna.edx"), "rb").read()


def test_without_shear_is_quick(tmp_path):
    a, b = str(tmp_path / "a.edx"), str(tmp_path / "b.edx")
    assert run(["-r", os.path.join(G, "refs.fa"), "-d", "DNA", "320", "-o", a, "-i", "0.95"]).returncode == 0
    assert run(["-r", os.path.join(G, "refs.fa"), "-d", "QUICK", "320", "-o", b, "-i", "0.95"]).returncode == 0
    assert open(a, "rb").read() == open(b, "rb").read()


def test_dp_is_inert_under_quick(tmp_path):
    a, b = str(tmp_path / "a.edx"), str(tmp_path / "b.edx")
    assert run(["-r", os.path.join(G, "refs.fa"), "-d", "QUICK", "320", "-o", a, "-s", "500", "-i", "0.95", "-dp", "3"]).returncode == 0
    assert run(["-r", os.path.join(G, "refs.fa"), "-d", "QUICK", "320", "-o", b, "-s", "500", "-i", "0.95"]).returncode == 0
    assert open(a, "rb").read() == open(b, "rb").read()


def test_refusals(tmp_path):
    out = str(tmp_path / "x.edx")
    r = run(["-r", os.path.join(G, "refs.fa"), "-d", "DNA", "320", "-o", out, "-s", "500", "-dp", "-1"])
    assert r.returncode == 1 and "dbpartition" in r.stdout
    r = run(["-r", os.path.join(G, "refs.fa"), "-d", "DNA", "5", "-o", out, "-s", "1", "-i", "0.97"])
    assert r.returncode == 1 and "shear + overlap >= 24" in r.stdout
    r = run(["-r", os.path.join(G, "refs.fa"), "-d", "DNA", "320", "-o", out, "-s", "500", "-cr", "3"])
    assert r.returncode == 1 and "fingerprints" in r.stdout


@pytest.mark.skipif(not os.path.exists(REF), reason="no compiled reference (oracle/_ref/burst12)")
@pytest.mark.parametrize("args", [["--seed", "3", "--", "-d", "DNA", "120", "-s", "200", "-i", "0.97"],
                                  ["--seed", "4", "--rate", "0.002", "--", "-d", "DNA", "150", "-s", "100", "-i", "0.97", "-dp", "2"]])
def test_differential(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dna_db_diff.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=ENV)
    assert r.returncode == 0, r.stdout
