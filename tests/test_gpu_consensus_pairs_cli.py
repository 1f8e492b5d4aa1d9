"""burst_hip --consensus PREFIX --consensus-pairs end to end on the MI355X, on the tiny database of the consensus test: three samples of a
few hundred reads, one of them with planted substitutions; the three files against the model of conspairslib applied to the written
consensus.fa; Differ on the planted reference; the outputs without the flag keep their bytes; --gpus 1; a sample list with an unreadable
sample; a study of one sample; the Python session."""
import os
import subprocess

import pytest

import conspairslib as cl
import goldenlib as gl
import pilelib

pytestmark = pytest.mark.gpu

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
DB = os.path.join(gl.G, "dna.edx")
Q100 = os.path.join(gl.G, "q100.fa")
REFS = {name: seq for name, seq in pilelib.read_fasta(os.path.join(gl.G, "refs.fa"))}
PLANT = next(n for n, s in REFS.items() if len(s) >= 700 and set(s[:700].upper()) <= set("ACGT"))      # the first all-ACGT reference
PLANTED = (150, 300, 450)      # 0-based offsets on PLANT that the reads of the modified sample substitute
BASE = ["-r", DB, "-ad", "-m", "BEST", "-i", "0.95", "-fr"]
SUFFIXES = ("consensus_pairs.txt", "consensus_identity.txt", "consensus_compared.txt")
FIVE = ("consensus.fa", "consensus.txt") + SUFFIXES


def run(args, want=0):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == want, r.stdout[-3000:]
    return r.stdout


def read(path):
    return open(str(path), "rb").read()


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    """three query files: q100.fa and 61 reads of 100 bases at stride 10 cut from PLANT; the second has every cut read twice; in the third
    every cut read that covers a planted offset shows the next base there.  One run with the flag, shared by the tests, never changed"""
    d = tmp_path_factory.mktemp("pairs_study")
    seq = REFS[PLANT].upper()
    files = []
    for name, copies, plant in (("plain", 1, False), ("twice", 2, False), ("planted", 1, True)):
        path = str(d / (name + ".fa"))
        with open(path, "w") as f:
            f.write(open(Q100).read())
            for k in range(61):
                read_ = "".join("ACGT"[("ACGT".index(seq[p]) + 1) % 4] if plant and p in PLANTED else seq[p] for p in range(10 * k, 10 * k + 100))
                for c in range(copies):
                    f.write(">cut_%d_%d\n%s\n" % (k, c, read_))
        files.append(path)
    lst = d / "list.txt"
    outs = [str(d / n) for n in ("plain.b6", "twice.b6", "planted.b6")]
    lst.write_text("".join("%s\t%s\n" % qo for qo in zip(files, outs)))
    args = BASE + ["--samples", str(lst), "--consensus", str(d / "P_"), "--consensus-min-depth", "1"]
    text = run(args + ["--consensus-pairs"])
    return d, files, outs, args, text


def test_three_files_are_the_model_of_the_written_fasta(study):
    d, files, outs, args, text = study
    names = ["plain", "twice", "planted"]
    fa = read(d / "P_consensus.fa")
    want = cl.files(fa, names)
    got = tuple(read(d / ("P_" + s)) for s in SUFFIXES)
    assert got == want
    rows = {tuple(r[:3]): r[3:] for r in (ln.split("\t") for ln in got[0].decode().split("\n")[1:] if ln)}
    # the planted positions are covered in every sample (the data must show what the test is about) ...
    recs = dict(zip(fa.decode().split("\n")[0::2], fa.decode().split("\n")[1::2]))
    ref = REFS[PLANT].upper()
    for p in PLANTED:
        assert recs[">plain|" + PLANT][p] == recs[">twice|" + PLANT][p] == ref[p] and recs[">planted|" + PLANT][p] == "ACGT"[("ACGT".index(ref[p]) + 1) % 4]
    # ... the unmodified samples agree everywhere on the planted reference, the modified one differs from both exactly there
    assert rows[(PLANT, "plain", "twice")][3] == "0" and int(rows[(PLANT, "plain", "twice")][1]) >= 700
    assert rows[(PLANT, "plain", "planted")][3] == "3" and rows[(PLANT, "twice", "planted")][3] == "3"
    assert len(rows) > 3 and list(rows) == sorted(rows, key=lambda k: (k[0].encode(), names.index(k[1]), names.index(k[2])))
    line = next(ln for ln in text.split("\n") if ln.startswith("ConsensusPairs: "))
    assert "3 samples done, 0 failed, %d records" % fa.count(b">") in line and "%d written" % len(rows) in line and "host bytes kept, device " in line
    assert "Samples: 3 done, 0 failed" in text and "Consensus pairs written: %sconsensus_pairs.txt" % (d / "P_") in text
    assert sorted(f for f in os.listdir(str(d)) if "tmp" in f) == []


def test_without_the_flag_the_outputs_keep_their_bytes_and_no_new_file(study, tmp_path):
    d, files, outs, args, text = study
    lst = tmp_path / "list.txt"
    mine = [str(tmp_path / os.path.basename(o)) for o in outs]
    lst.write_text("".join("%s\t%s\n" % qo for qo in zip(files, mine)))
    plain = run(BASE + ["--samples", str(lst), "--consensus", str(tmp_path / "P_"), "--consensus-min-depth", "1"])
    assert "ConsensusPairs" not in plain and "Consensus pairs written" not in plain
    for a, b in zip(outs, mine):
        assert read(a) == read(b)
    assert read(tmp_path / "P_consensus.fa") == read(d / "P_consensus.fa") and read(tmp_path / "P_consensus.txt") == read(d / "P_consensus.txt")
    assert sorted(os.listdir(str(tmp_path))) == sorted(["list.txt", "P_consensus.fa", "P_consensus.txt"] + [os.path.basename(o) for o in outs])


def test_gpus_1_and_m(study, tmp_path):
    d, files, outs, args, text = study
    lst = tmp_path / "list.txt"
    lst.write_text("".join("%s\t%s\n" % (q, tmp_path / os.path.basename(o)) for q, o in zip(files, outs)))
    run(BASE + ["--gpus", "1", "--samples", str(lst), "--consensus", str(tmp_path / "P_"), "--consensus-min-depth", "1", "--consensus-pairs"])
    for s in FIVE:
        assert read(tmp_path / ("P_" + s)) == read(d / ("P_" + s)), s
    m = 1 + max(int(ln.split("\t")[4]) for ln in read(d / "P_consensus_pairs.txt").decode().split("\n")[1:] if ln)      # above every Compared
    run(BASE + ["--gpus", "1", "--samples", str(lst), "--consensus", str(tmp_path / "M_"), "--consensus-min-depth", "1", "--consensus-pairs", "--consensus-pairs-min", str(m)])
    assert (read(tmp_path / "M_consensus_pairs.txt"),) + tuple(read(tmp_path / ("M_" + s)) for s in SUFFIXES[1:]) == cl.files(read(d / "P_consensus.fa"), ["plain", "twice", "planted"], (), m)
    assert read(tmp_path / "M_consensus_pairs.txt").count(b"\n") == 1


def test_a_sample_list_with_an_unreadable_sample(study, tmp_path):
    d, files, outs, args, text = study
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\n%s\t%s\n%s\t%s\n" % (files[0], tmp_path / "plain.b6", tmp_path / "missing.fa", tmp_path / "gone.b6", files[2], tmp_path / "planted.b6"))
    out = run(BASE + ["--samples", str(lst), "--consensus", str(tmp_path / "P_"), "--consensus-min-depth", "1", "--consensus-pairs"], want=2)
    assert "Samples: 2 done, 1 failed" in out and "consensus: sample 'gone' failed alone" in out and "ConsensusPairs: 2 samples done, 1 failed" in out
    names = ["plain", "gone", "planted"]
    got = tuple(read(tmp_path / ("P_" + s)) for s in SUFFIXES)
    assert got == cl.files(read(tmp_path / "P_consensus.fa"), names, ["gone"])
    assert got[1].decode().split("\n")[2] == "gone\tNA\tNA\tNA" and got[2].decode().split("\n")[2] == "gone\tNA\tNA\tNA"
    assert ("\t".join((PLANT, "plain", "planted")) + "\t").encode() in got[0] and b"\tgone\t" not in got[0]


def test_a_study_of_one_sample_and_the_python_session(study, tmp_path):
    d, files, outs, args, text = study
    out = run(BASE + ["-q", files[2], "-o", str(tmp_path / "one.b6"), "--consensus", str(tmp_path / "O_"), "--consensus-min-depth", "1", "--consensus-pairs"])
    assert "\nConsensusPairs: 1 samples done, 0 failed" in out
    got = tuple(read(tmp_path / ("O_" + s)) for s in SUFFIXES)
    assert got == cl.files(read(tmp_path / "O_consensus.fa"), ["one"]) and got[0].count(b"\n") == 1 and got[1] == b"#Identity\tone\none\t1.000000\n"
    # host.Session on the device and with the plain C yardstick: the command line's five files both times
    from burst_amd import host
    db = host.Db.read(DB)
    dev = db.open_device(0, build_K=12)
    for k, on_host in enumerate((False, True)):
        w = tmp_path / ("ses%d" % k)
        w.mkdir()
        with host.Session(db, dev, mode="BEST", thres=0.95, rc=True, accel=True, K=12, consensus=str(w / "P_"), consensus_min_depth=1, consensus_pairs=True,
                          consensus_pairs_host=on_host) as s:
            for q, o in zip(files, outs):
                res = s.run(q, str(w / os.path.basename(o)))
                assert res["rc"] == 0, res["err"]
            info = s.consensus_pairs()
            assert (info["samples"], info["failed"]) == (3, 0) and info["pairs"] > 3 and info["host_bytes"] > 0 and (info["device_us"] > 0) == (not on_host)
        for sfx in FIVE:
            assert read(w / ("P_" + sfx)) == read(d / ("P_" + sfx)), sfx
