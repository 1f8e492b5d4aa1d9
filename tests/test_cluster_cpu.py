"""--cluster without a device: bh_cluster_host (the definition in plain sequential C) against the Python model (tests/clusterlib.py) on
the graphs the device tests use, the name table, the lines and the two tables behind the solver hook, and the refusals of the command
lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

import clustercases as cc
import clusterlib as cl
from burst_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")


def check(weights, edges):
    centroid, edits, info = host.cluster_host(weights, edges)
    want_c, want_e = cl.cluster(weights, edges)
    assert centroid.tolist() == want_c and edits.tolist() == want_e
    assert int(info[2]) == sum(1 for i, c in enumerate(want_c) if c == i) and int(info[5]) == len(edges) and int(info[6]) == len(weights)
    return want_c, want_e


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_equals_model(name):
    check(*cc.CASES[name])


def test_hand_values():
    """what the cases are there for, spelled out"""
    c, e = check(*cc.CASES["chain300"])
    assert c[:6] == [0, 0, 2, 2, 4, 4] and e[:4] == [0, 1, 0, 0]
    c, _ = check(*cc.CASES["chain300_reversed"])
    assert c[-4:] == [297, 297, 299, 299]
    assert check(*cc.CASES["five_times"]) == ([0, 0], [0, 2])
    assert check(*cc.CASES["equal_edits_earlier_wins"]) == ([0, 1, 0], [0, 0, 3])
    assert check(*cc.CASES["nearer_later_wins"]) == ([0, 1, 1], [0, 0, 1])
    assert check(*cc.CASES["lower_priority_only"])[0] == [0, 1, 2, 3]
    assert check(*cc.CASES["directed"]) == ([0, 1, 1], [0, 0, 0])
    assert check(*cc.CASES["weights_1_and_max"]) == ([1, 1, 2, 1], [1, 0, 0, 2])
    for deg in (63, 64, 65, 1000):
        assert check(*cc.CASES["star%d_last" % deg])[0][0] == deg + 1
        assert check(*cc.CASES["star%d_first" % deg])[0][0] == 2
        assert check(*cc.CASES["star%d_absent" % deg])[0][0] == 0


@pytest.mark.parametrize("seed", cc.RANDOM_SEEDS)
def test_random_graphs(seed):
    w, e = cc.random_graph(seed)
    assert len(w) == 2000 and len(e) == 20000
    c, _ = check(w, e)
    assert 1 < sum(1 for i, x in enumerate(c) if x == i) < 2000


def test_node_out_of_range():
    with pytest.raises(host.HostError, match="names node"):
        host.cluster_host([1, 1], [(0, 2, 0)])


def b6(q, r, edits):
    return "%s\t%s\t97.5\t120\t%d\t0\t1\t120\t1\t120\t%d\t7\n" % (q, r, edits, edits)


NAMES = ["a;size=3", "b;size=10;", "c", "d;size=3", "lonely", "e;size=x", "f;size=2;extra"]
B6 = (b6("a;size=3", "b;size=10;", 2) + b6("a;size=3", "a;size=3", 0) + b6("a;size=3", "elsewhere", 0)      # an edge, a self line, a foreign line
      + b6("c", "a;size=3", 4) + b6("c", "a;size=3", 1)                                                       # two strands, different edits
      + b6("c", "d;size=3", 1) + b6("d;size=3", "c", 1)                                                       # equal edits: the earlier centroid
      + b6("b;size=10;", "a;size=3", 2) + b6("e;size=x", "f;size=2;extra", 0) + b6("f;size=2;extra", "e;size=x", 0)
      + b6("f;size=2;extra", "not a read", 3))


@pytest.mark.parametrize("sizes", [False, True], ids=["unit", "sizes"])
@pytest.mark.parametrize("solver", ["host", "python"])
def test_tables_from_a_hand_made_b6(tmp_path, sizes, solver):
    """foreign lines, self lines, a read without lines, `;size=` with and without the closing `;` (and two names where it is no suffix),
    two lines for one (q, r): the tables are the model's text byte for byte, whichever solver sits behind the hook"""
    (tmp_path / "self.b6").write_text(B6)
    prefix = str(tmp_path / "P.")
    seen = []

    def py_solver(w, e):
        seen.append((w.tolist(), len(e)))
        return cl.cluster(w.tolist(), [(int(x["q"]), int(x["r"]), int(x["edits"])) for x in e])

    with host.Clusterer(prefix, NAMES, sizes=sizes, solver=py_solver if solver == "python" else None) as c:
        c.add_b6(str(tmp_path / "self.b6"))
        centroid, edits = c.solve()
        info = c.info()
        c.write()
    w, e, lines, foreign = cl.from_b6(NAMES, B6, sizes)
    assert w == ([3, 10, 1, 3, 1, 1, 1] if sizes else [1] * 7)
    assert (info["lines"], info["foreign"]) == (lines, foreign) == (11, 2)
    assert (centroid.tolist(), edits.tolist()) == cl.cluster(w, e)
    if solver == "python":
        assert seen == [(w, len(e))]
    a, b = cl.tables_from_b6(NAMES, B6, sizes)
    assert open(prefix + "clusters.txt").read() == a and open(prefix + "cluster_sizes.txt").read() == b
    assert sorted(os.listdir(str(tmp_path))) == ["P.cluster_sizes.txt", "P.clusters.txt", "self.b6"]
    if sizes:      # b (10) first; a joins it; d (3) is a centroid; c's edge to a leads to a member, so c joins d
        assert a.splitlines()[1:5] == ["a;size=3\tb;size=10;\tM\t2\t3", "b;size=10;\tb;size=10;\tC\t0\t10", "c\td;size=3\tM\t1\t1", "d;size=3\td;size=3\tC\t0\t3"]
        assert b.splitlines()[1] == "b;size=10;\t2\t13"
    else:          # file order: a first; b and c join a, c with its smaller edits; d's only edge leads to a member
        assert a.splitlines()[1:5] == ["a;size=3\ta;size=3\tC\t0\t1", "b;size=10;\ta;size=3\tM\t2\t1", "c\ta;size=3\tM\t1\t1", "d;size=3\td;size=3\tC\t0\t1"]
    assert sum(int(r.split("\t")[2]) for r in b.splitlines()[1:]) == sum(w)


def test_duplicate_names_are_a_usage_error_and_leave_nothing(tmp_path):
    prefix = str(tmp_path / "P.")
    with pytest.raises(host.HostError) as ei:
        host.Clusterer(prefix, ["x", "y", "z", "y"])
    assert "error %d" % host.E_USAGE in str(ei.value) and "reads 2 and 4" in str(ei.value) and "'y'" in str(ei.value)      # (BH_E_USAGE is exit code 1 of burst_hip)
    assert os.listdir(str(tmp_path)) == []


def test_an_error_is_final(tmp_path):
    (tmp_path / "bad.b6").write_text(b6("x", "y", 0) + b6("nobody", "y", 0))
    with host.Clusterer(str(tmp_path / "P."), ["x", "y"]) as c:
        with pytest.raises(host.HostError, match="column 1 names no read"):
            c.add_b6(str(tmp_path / "bad.b6"))
        with pytest.raises(host.HostError):
            c.solve()
        with pytest.raises(host.HostError):
            c.write()
    assert os.listdir(str(tmp_path)) == ["bad.b6"]


def test_size_out_of_range(tmp_path):
    for bad in ("r;size=0", "r;size=4294967296"):
        with pytest.raises(host.HostError, match="cluster-sizes"):
            host.Clusterer(str(tmp_path / "P."), [bad], sizes=True)
    with host.Clusterer(str(tmp_path / "P."), ["r;size=4294967295", "s;size=0"], sizes=False) as c:
        assert c.solve()[0].tolist() == [0, 1]


SELF = ["-r", os.path.join(GOLDEN, "q100.fa"), "-q", os.path.join(GOLDEN, "q100.fa")]


@pytest.mark.parametrize("args,word", [
    (["-m", "ALLPATHS"], "FORAGE"), (["-m", "BEST"], "FORAGE"), (["-m", "CAPITALIST"], "FORAGE"), (["-m", "ANY"], "FORAGE"), ([], "FORAGE"),
    (["-m", "FORAGE", "--samples", "LIST"], "--samples"),
    (["-m", "FORAGE", "--mates", "m.fa"], "--mates"),
    (["-m", "FORAGE", "-x"], "-x"),
    (["-m", "FORAGE", "-d"], "-d"),
    (["-m", "FORAGE", "--make-acx", "x.acx"], "--make-acx"),
    (["-m", "FORAGE", "--gpus", "2", "--shard", "db"], "--shard db"),
    (["-m", "FORAGE", "--shards", "2"], "--shards"),
    (["-m", "FORAGE", "--gpus", "2", "--gather", "rccl"], "rccl"),
    (["-m", "FORAGE", "--coverage", "C."], "--coverage"),
    (["-m", "FORAGE", "--abundance", "A."], "--abundance"),
    (["-m", "FORAGE", "--variants", "V."], "--variants"),
])
def test_refusals_before_a_device_is_touched(tmp_path, args, word):
    """usage errors, exit code 1, with nothing read, no device opened (this machine may have none) and no file left"""
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\n")
    args = [str(lst) if a == "LIST" else a for a in args]
    io = [] if "--samples" in args else ["-o", str(tmp_path / "o.b6")]
    r = subprocess.run([BURST_HIP] + (SELF if io else SELF[:2]) + io + ["--cluster", str(tmp_path / "P.")] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --cluster" in r.stdout and word in r.stdout, r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["list.txt"]


def test_sizes_without_cluster_is_refused(tmp_path):
    r = subprocess.run([BURST_HIP] + SELF + ["-o", str(tmp_path / "o.b6"), "-m", "FORAGE", "--cluster-sizes"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "ERROR: --cluster-sizes goes with --cluster" in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--cluster", "P"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--cluster is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--cluster <prefix>" in r.stdout and "--cluster-sizes" in r.stdout


def test_session_refuses_other_modes():
    with pytest.raises(ValueError, match="FORAGE"):
        host.Session(host.Db(), devs=[None], mode="BEST", cluster="P.", align=lambda *a: 0)


def test_exports_follow_the_header():
    text = open(os.path.join(ROOT, "include", "burst_hip.h")).read()
    for name in ("bhip_cluster_run", "bhip_cluster_info"):
        assert name in capi.EXPORTS and "BHIP_API int %s(" % name in text
    assert capi.CLUSTER_EDGE_DTYPE.itemsize == 12
    assert np.dtype(capi.CLUSTER_EDGE_DTYPE).names == ("q", "r", "edits")


def test_host_file_under_the_sanitizers(tmp_path):
    """csrc/host/bh_cluster.c as a stand-alone program with ASan and UBSan linked in: names, lines, solve, tables, errors, a random graph"""
    exe, prefix, b6_path = str(tmp_path / "cluster_host_main"), str(tmp_path / "SAN_"), str(tmp_path / "t.b6")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "cluster_host_main.c"), os.path.join(CSRC, "host", "bh_cluster.c"), os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    names = ["a;size=3", "b;size=10;", "c", "d;size=3", "lonely", "e;size=x", "f;size=2;extra", ""]
    text = b6("a;size=3", "b;size=10;", 2) + b6("c", "a;size=3", 4) + b6("c", "nobody", 4) + b6("", "c", 1)
    open(b6_path, "w").write(text)
    r = subprocess.run([exe, prefix, b6_path], capture_output=True, text=True)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "cluster_host_main ok" in r.stdout, r.stdout + r.stderr
    assert "reads 1 and 3 of the query file are both named 'x'" in r.stdout
    a, b = cl.tables_from_b6(names, text, True)      # (the program's second pass, with the sizes, wrote last)
    assert open(prefix + "clusters.txt").read() == a and open(prefix + "cluster_sizes.txt").read() == b
