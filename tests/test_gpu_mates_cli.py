"""burst_hip --mates on the MI355X: the pair files of the CPU test (tests/matesdata.py) through the command line, with an accelerator file
and with one built on the device, in ALLPATHS and FORAGE.  The paired output must be, byte for byte, the definition (tests/mateslib.py)
applied to the outputs of two single-end runs of the same binary with the same flags, made in the same test; the `Mates:` line must
carry the definition's counts."""
import os
import re
import subprocess

import pytest

import goldenlib as gl
import matesdata as md
import mateslib as ml

pytestmark = pytest.mark.gpu
CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
_state = {}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mates_cli"))
    p1, p2, _ = md.write_files(d)
    acx = os.path.join(d, "dna.acx")
    subprocess.check_call([CLI, "-r", EDX, "--make-acx", acx], stdout=subprocess.DEVNULL, timeout=600)
    return d, p1, p2, acx


def run(args):
    r = subprocess.run([CLI, "-r", EDX] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def accel(kind, files):
    return ["-a", files[3]] if kind == "a" else ["-ad", "-k", "12"]


def singles(files, kind, mode):
    """the two single-end outputs (-q FILE -m MODE -fr), once per accelerator kind and mode"""
    if (kind, mode) not in _state:
        out = []
        for k, p in enumerate(files[1:3]):
            o = os.path.join(files[0], "single_%s_%s_%d.b6" % (kind, mode, k))
            run(accel(kind, files) + ["-q", p, "-o", o, "-m", mode, "-i", "0.95", "-fr"])
            out.append(open(o, "rb").read())
        _state[(kind, mode)] = tuple(out)
    return _state[(kind, mode)]


def mates_line(stdout):
    m = re.findall(r"^Mates: (\d+) \+ (\d+) reads, (\d+) pairs named in both files, (\d+) placed on both sides; (\d+) \+ (\d+) lines, (\d+) combinations examined, (\d+) written; ([0-9.]+) ms on the device$",
                   stdout, re.M)
    assert len(m) >= 1, stdout[-2000:]
    return [tuple(int(x) for x in g[:8]) + (float(g[8]),) for g in m]


def check_counts(line, b1, b2, files, *opts):
    c = ml.counts(b1, b2, md.names_of(files[1]), md.names_of(files[2]), *opts)
    assert line[:8] == (c["reads1"], c["reads2"], c["named"], c["placed"], len(b1.splitlines()), len(b2.splitlines()), c["examined"], c["written"])
    assert line[8] > 0


@pytest.mark.parametrize("mode", ["ALLPATHS", "FORAGE"])
@pytest.mark.parametrize("kind", ["ad", "a"])
def test_mates_is_the_definition(files, kind, mode):
    b1, b2 = singles(files, kind, mode)
    assert len(b1) and len(b2)
    out = os.path.join(files[0], "paired_%s_%s.b6" % (kind, mode))
    so = run(accel(kind, files) + ["-q", files[1], "--mates", files[2], "-o", out, "-m", mode, "-i", "0.95", "--insert-max", str(md.INSERT_MAX)])      # (-fr is implied)
    exp = ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all")
    assert open(out, "rb").read() == exp and len(exp.splitlines()) > 400
    check_counts(mates_line(so)[0], b1, b2, files, "fr", 0, md.INSERT_MAX, "all")
    assert not [f for f in os.listdir(files[0]) if f.endswith(".tmp")]


def test_options_reach_the_join(files):
    b1, b2 = singles(files, "ad", "FORAGE")
    out = os.path.join(files[0], "paired_opts.b6")
    for opts, args in ((("fr", 300, 500, "best"), ["--insert-min", "300", "--insert-max", "500", "--mates-report", "best"]),
                       (("ff", 0, 1000, "all"), ["--mates-orientation", "ff"])):
        so = run(accel("ad", files) + ["-q", files[1], "--mates", files[2], "-o", out, "-m", "FORAGE", "-i", "0.95"] + args)
        exp = ml.paired_text(b1, b2, *opts)
        assert open(out, "rb").read() == exp and len(exp) > 0
        check_counts(mates_line(so)[0], b1, b2, files, *opts)


def test_three_field_lines_in_a_sample_list(files):
    """a list that mixes plain samples and pairs: the plain outputs are the single-end runs', the pairs' the definition"""
    b1, b2 = singles(files, "ad", "ALLPATHS")
    d = files[0]
    outs = [os.path.join(d, "list_o%d.b6" % i) for i in range(4)]
    lst = os.path.join(d, "list.tsv")
    open(lst, "w").write("%s\t%s\n%s\t%s\t%s\n%s\t%s\n%s\t%s\t%s\n" % (files[1], outs[0], files[1], outs[1], files[2], files[2], outs[2], files[1], outs[3], files[2]))
    so = run(accel("ad", files) + ["--samples", lst, "-m", "ALLPATHS", "-i", "0.95", "-fr", "--insert-max", str(md.INSERT_MAX)])
    exp = ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all")
    assert open(outs[0], "rb").read() == b1 and open(outs[2], "rb").read() == b2
    assert open(outs[1], "rb").read() == exp and open(outs[3], "rb").read() == exp
    lines = mates_line(so)
    assert len(lines) == 2 and "Samples: 4 done, 0 failed" in so
    for ln in lines:
        check_counts(ln, b1, b2, files, "fr", 0, md.INSERT_MAX, "all")


def test_two_ranks_on_one_device(files):
    b1, b2 = singles(files, "ad", "FORAGE")
    out = os.path.join(files[0], "paired_2ranks.b6")
    so = run(accel("ad", files) + ["-q", files[1], "--mates", files[2], "-o", out, "-m", "FORAGE", "-i", "0.95", "--insert-max", str(md.INSERT_MAX), "--gpus", "2", "--devices", "0,0"])
    # (the ranks' records meet in (entry, reference) order whatever the number of ranks: the single-end lines are the same lines)
    assert open(out, "rb").read() == ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all")
    check_counts(mates_line(so)[0], b1, b2, files, "fr", 0, md.INSERT_MAX, "all")


def test_database_sharded_over_two_ranks(files):
    """--shards 2: the rank that reports holds a slice of the database; the join needs only some resident handle"""
    b1, b2 = singles(files, "ad", "ALLPATHS")
    out = os.path.join(files[0], "paired_shards.b6")
    run(accel("ad", files) + ["-q", files[1], "--mates", files[2], "-o", out, "-m", "ALLPATHS", "-i", "0.95", "--insert-max", str(md.INSERT_MAX), "--gpus", "2", "--devices", "0,0", "--shards", "2"])
    assert open(out, "rb").read() == ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all")
