"""--chimeras without a device: bh_chimera_host (the definition in plain sequential C) against the Python model (tests/chimeralib.py) on
the inputs the device tests use, its argument checks, the lines and the table behind the solver hook, and the refusals of the command
lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chimeracases as cc
import chimeralib as ml
from burst_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")


def check(w, lens, lines, ops, par):
    got, info = host.chimera_host(w, lens, lines, ops, **par)
    want, kept = ml.chimera(w, lens, lines, ops, **par)
    assert ml.rows_of(got) == want
    assert [int(x) for x in info] == [kept, sum(1 for r in want if r[0]), sum(1 for r in want if r[0] == 2), 0, 0, len(lines), len(w), 0]
    return want


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_equals_model(name):
    check(*cc.CASES[name])


def test_hand_values():
    """what the cases are there for, spelled out: (role, single, model, cut, a, ea, b, eb) of read 0"""
    base = (2, 3, 0, 16, 1, 0, 2, 0)      # X at 29, 31, 33 towards 1, at 6, 8, 10 towards 2: every cut 16 .. 24 has model 0, the smallest wins
    for name in ("baseline", "baseline_reverse", "baseline_mixed_strands", "gain_exactly_d"):
        assert check(*cc.CASES[name])[0] == base, name
    assert check(*cc.CASES["gain_d_minus_1"])[0] == (1,) + base[1:]
    assert check(*cc.CASES["min_seg_1"])[0] == (2, 3, 0, 11, 1, 0, 2, 0)      # the first cut behind B's last X (symbol 10: position 21 <= 22)
    for name in ("d_at_the_cut", "d_at_the_cut_reverse"):      # the D is left of the cut in both orientations: parent 1 is clean on the right only
        assert check(*cc.CASES[name])[0] == (2, 1, 0, 16, 2, 0, 1, 0), name
    for name in ("i_runs", "i_runs_reverse"):
        assert check(*cc.CASES[name])[0] == (2, 3, 0, 16, 2, 0, 1, 0), name
    assert check(*cc.CASES["len_2g_one_cut"])[0][:4] == (2, 3, 0, 16)
    assert check(*cc.CASES["len_2g_minus_1"]) == [(0,) * 8] * 3
    assert check(*cc.CASES["len_1"]) == [(0,) * 8] * 3
    assert check(*cc.CASES["edits254"])[0] == (2, 254, 0, 254, 2, 0, 1, 0)
    assert check(*cc.CASES["equal_left_goes_to_priority"])[0] == (1, 0, 0, 16, 2, 0, 2, 0)
    assert check(*cc.CASES["five_times"])[0] == (2, 3, 0, 16, 1, 0, 2, 0)      # (q, 1): 3 edits twice, the first given has them on the right
    rows = check(*cc.CASES["skew_edge"])
    assert rows[0] == (2, 3, 0, 16, 1, 0, 2, 0) and rows[4] == (1, 0, 0, 16, 1, 0, 2, 0)      # read 0 does not see the clean parent 3; read 4 does (Single 0), and equal L and R go to the higher priority
    rows = check(*cc.CASES["wide_product"])
    assert rows[0][0] == 2 and rows[1] == (0,) * 8
    for name in ("self_lines_only", "one_candidate_only", "no_lines", "lines_1"):
        assert all(r == (0,) * 8 for r in check(*cc.CASES[name])), name
    for n in (63, 64, 65, 129, 4095):
        assert check(*cc.CASES["len_%d" % n])[0][:3] == (2, 3, 0), n
    for k in (2, 64, 65, 1500):
        assert check(*cc.CASES["lines_%d" % k])[0][0] != 0, k


@pytest.mark.parametrize("seed", cc.RANDOM_SEEDS)
def test_random_cases(seed):
    w, lens, lines, ops, par = cc.random_case(seed)
    assert len(w) == 2000 and len(lines) == 20000
    rows = check(w, lens, lines, ops, par)
    assert sum(1 for r in rows if r[0] == 2) > 0 and sum(1 for r in rows if r[0] == 1) > 0 and sum(1 for r in rows if r[0] == 0) > 0


W3, L3 = [1, 2, 2], [8, 8, 8]


@pytest.mark.parametrize("lines,ops,par,word", [
    ([(0, 3, 0, 1, 0)], [8 << 4 | 7], {}, "names node"),
    ([(3, 0, 0, 1, 0)], [8 << 4 | 7], {}, "names node"),
    ([(0, 1, 0, 2, 0)], [8 << 4 | 7], {}, "leave"),
    ([(0, 1, 0, 1, 1)], [8 << 4 | 7], {}, "leave"),
    ([(0, 1, 0, 1, 2 ** 62)], [8 << 4 | 7], {}, "leave"),
    ([(0, 1, 0, 1, 0)], [8 << 4 | 3], {}, "no run of"),
    ([(0, 1, 0, 2, 0)], [8 << 4 | 7, 0 << 4 | 8], {}, "no run of"),
    ([(0, 1, 0, 1, 0)], [7 << 4 | 7], {}, "consume"),
    ([(0, 1, 0, 2, 0)], [8 << 4 | 7, 1 << 4 | 1], {}, "consume"),
    ([(0, 1, 0, 2, 0)], [8 << 4 | 7, 255 << 4 | 2], {}, "edits"),
    ([(0, 1, 0, 1, 0)], [8 << 4 | 7], {"skew": 0}, "at least 1"),
    ([(0, 1, 0, 1, 0)], [8 << 4 | 7], {"min_seg": 0}, "at least 1"),
    ([(0, 1, 0, 1, 0)], [8 << 4 | 7], {"min_gain": 0}, "at least 1"),
])
def test_argument_checks(lines, ops, par, word):
    """every condition bhip_chimera_run answers with BHIP_E_ARG, through the yardstick's copy of the checks"""
    with pytest.raises(host.HostError, match=word) as ei:
        host.chimera_host(W3, L3, lines, ops, **par)
    assert "error %d" % host.E_USAGE in str(ei.value)


@pytest.mark.parametrize("length", [0, 4096])
def test_read_length_checks(length):
    ops = [length << 4 | 7] if length else [1 << 4 | 2]
    with pytest.raises(host.HostError, match="symbols"):
        host.chimera_host(W3, [length, 8, 8], [(0, 1, 0, 1, 0)], ops)


def test_a_d_of_254_is_accepted():
    rows, _ = host.chimera_host(W3, L3, [(0, 1, 0, 2, 0)], [8 << 4 | 7, 254 << 4 | 2])
    assert ml.rows_of(rows) == [(0,) * 8] * 3


def b6(q, r, cigar, rev=False, qlen=40):
    words = ml.ops_of(cigar)
    edits = sum(w >> 4 for w in words if w & 15 != 7)
    st, ed = (qlen, 1) if rev else (1, qlen)
    return "%s\t%s\t97.5\t%d\t%d\t0\t1\t%d\t%d\t%d\t%d\t7\t1\t%s\n" % (q, r, qlen, edits, qlen, st, ed, edits, cigar)


NAMES = ["q;size=1", "a;size=9", "b;size=9;", "lonely", "n;size=4", "c"]
B6 = (b6("q;size=1", "a;size=9", cc.xs(40, [30, 32, 34])) + b6("q;size=1", "b;size=9;", cc.mirror(cc.xs(40, [3, 5, 7])), rev=True)      # a chimera, one line reverse
      + b6("q;size=1", "q;size=1", "40=") + b6("q;size=1", "elsewhere", "40=")                                                           # a self line, a foreign line
      + b6("q;size=1", "a;size=9", cc.xs(40, [1, 2, 3, 4])) + b6("q;size=1", "a;size=9", cc.xs(40, [2, 3, 4]))                           # (q, a) again: more edits, equal edits later
      + b6("n;size=4", "a;size=9", cc.xs(40, [20])) + b6("n;size=4", "b;size=9;", cc.xs(40, [21]))                                       # two parents, no gain
      + b6("c", "lonely", "40=") + b6("c", "n;size=4", cc.xs(40, [], dels=[20]))                                                          # unit weights: c has no candidate parent but n with the sizes
      + b6("a;size=9", "b;size=9;", cc.xs(40, [9])) + b6("c", "not a read", "40="))


@pytest.mark.parametrize("sizes", [False, True], ids=["unit", "sizes"])
def test_table_from_a_hand_made_b6(tmp_path, sizes):
    """foreign lines, self lines, a reverse line, a read without lines, `;size=` with and without the closing `;`, three lines for one
    (q, r): the table is the model's text byte for byte with bh_chimera_host behind the solver hook"""
    (tmp_path / "self.b6").write_text(B6)
    prefix = str(tmp_path / "P.")
    with host.ChimeraChecker(prefix, NAMES, [40] * len(NAMES), sizes=sizes) as c:
        c.add_b6(str(tmp_path / "self.b6"))
        rows = c.solve()
        info = c.info()
        c.write()
    w, lens, lines, ops, printed, foreign = ml.from_b6(NAMES, B6, sizes)
    assert w == ([1, 9, 9, 1, 4, 1] if sizes else [1] * 6)
    assert (info["lines"], info["foreign"]) == (printed, foreign) == (12, 2)
    want, kept = ml.chimera(w, lens, lines, ops)
    assert ml.rows_of(rows) == want and info["pairs_kept"] == kept
    text = ml.table_from_b6(NAMES, B6, sizes)
    assert open(prefix + "chimeras.txt").read() == text
    assert sorted(os.listdir(str(tmp_path))) == ["P.chimeras.txt", "self.b6"]
    if sizes:
        assert text.splitlines()[:2] == ["#Read\tRole\tSingle\tModel\tCut\tParentA\tEditsA\tParentB\tEditsB\tWeight", "q;size=1\tY\t3\t0\t16\ta;size=9\t0\tb;size=9;\t0\t1"]
        assert text.splitlines()[4:6] == ["lonely\t-\t0\t0\t0\t*\t0\t*\t0\t1", "n;size=4\tN\t1\t0\t21\tb;size=9;\t0\ta;size=9\t0\t4"]
    else:          # unit weights with S = 2: nobody has a candidate parent
        assert all(r.split("\t")[1] == "-" for r in text.splitlines()[1:])


def test_duplicate_names_are_a_usage_error_and_leave_nothing(tmp_path):
    with pytest.raises(host.HostError) as ei:
        host.ChimeraChecker(str(tmp_path / "P."), ["x", "y", "z", "y"], [40] * 4)
    assert "error %d" % host.E_USAGE in str(ei.value) and "--chimeras needs every read named once: reads 2 and 4" in str(ei.value) and "'y'" in str(ei.value)
    assert os.listdir(str(tmp_path)) == []


def test_size_out_of_range_and_an_error_is_final(tmp_path):
    for bad in ("r;size=0", "r;size=4294967296"):
        with pytest.raises(host.HostError, match="--chimera-sizes"):
            host.ChimeraChecker(str(tmp_path / "P."), [bad], [40], sizes=True)
    (tmp_path / "bad.b6").write_text(b6("x", "y", "40=") + b6("nobody", "y", "40="))
    with host.ChimeraChecker(str(tmp_path / "P."), ["x", "y"], [40, 40]) as c:
        with pytest.raises(host.HostError, match="column 1 names no read"):
            c.add_b6(str(tmp_path / "bad.b6"))
        with pytest.raises(host.HostError):
            c.solve()
        with pytest.raises(host.HostError):
            c.write()
    (tmp_path / "plain.b6").write_text("x\ty\t97.5\t40\t0\t0\t1\t40\t1\t40\t0\t7\n")
    with host.ChimeraChecker(str(tmp_path / "P."), ["x", "y"], [40, 40]) as c:
        with pytest.raises(host.HostError, match="--cigar"):
            c.add_b6(str(tmp_path / "plain.b6"))
    assert sorted(os.listdir(str(tmp_path))) == ["bad.b6", "plain.b6"]


@pytest.mark.parametrize("par", [{"skew": 0}, {"min_seg": 0}, {"min_gain": 0}, {"skew": 2 ** 31}, {"min_seg": 2 ** 31}, {"min_gain": 2 ** 31}])
def test_policy_out_of_range(tmp_path, par):
    with pytest.raises(host.HostError, match="2147483647"):
        host.ChimeraChecker(str(tmp_path / "P."), ["x"], [40], **par)


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
    r = subprocess.run([BURST_HIP] + (SELF if io else SELF[:2]) + io + ["--chimeras", str(tmp_path / "P.")] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --chimeras" in r.stdout and word in r.stdout, r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["list.txt"]


@pytest.mark.parametrize("opt", [["--chimera-sizes"], ["--chimera-skew", "3"], ["--chimera-min-seg", "8"], ["--chimera-min-gain", "2"]])
def test_sub_options_without_chimeras_are_refused(tmp_path, opt):
    r = subprocess.run([BURST_HIP] + SELF + ["-o", str(tmp_path / "o.b6"), "-m", "FORAGE"] + opt, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "go with --chimeras" in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("opt", ["--chimera-skew", "--chimera-min-seg", "--chimera-min-gain"])
@pytest.mark.parametrize("value", ["0", "2147483648", "-1", "x"])
def test_policy_values_out_of_range_are_refused(tmp_path, opt, value):
    r = subprocess.run([BURST_HIP] + SELF + ["-o", str(tmp_path / "o.b6"), "-m", "FORAGE", "--chimeras", str(tmp_path / "P."), opt, value], capture_output=True, text=True,
                       cwd=str(tmp_path))
    # (a value that begins with '-' reads as the next flag: the option then lacks its argument, which is refused as well)
    assert r.returncode == 1 and "ERROR: %s %s" % (opt, "requires an argument" if value == "-1" else "takes a number 1 .. 2147483647") in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--chimeras", "P"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--chimeras is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    for flag in ("--chimeras <prefix>", "--chimera-sizes", "--chimera-skew", "--chimera-min-seg", "--chimera-min-gain"):
        assert flag in r.stdout, flag


def test_session_refuses_other_modes():
    with pytest.raises(ValueError, match="FORAGE"):
        host.Session(host.Db(), devs=[None], mode="BEST", chimeras="P.", align=lambda *a: 0)


def test_exports_follow_the_header():
    text = open(os.path.join(ROOT, "include", "burst_hip.h")).read()
    for name in ("bhip_chimera_run", "bhip_chimera_info"):
        assert name in capi.EXPORTS and "BHIP_API int %s(" % name in text
    assert "typedef struct BhipChimLine { uint32_t q, r, flags /* bit 0: reverse */, n_ops; uint64_t op_off; } BhipChimLine;" in text
    assert "typedef struct BhipChimera  { uint32_t role /* 0 '-', 1 'N', 2 'Y' */, single, model, cut, a, ea, b, eb; } BhipChimera;" in text
    assert np.dtype(capi.CHIM_LINE_DTYPE).names == ("q", "r", "flags", "n_ops", "op_off") and capi.CHIM_LINE_DTYPE.itemsize == 24
    assert np.dtype(capi.CHIMERA_DTYPE).names == ("role", "single", "model", "cut", "a", "ea", "b", "eb") and capi.CHIMERA_DTYPE.itemsize == 32


def test_host_file_under_the_sanitizers(tmp_path):
    """csrc/host/bh_chimera.c (with bh_cluster.c, whose name table it uses) as a stand-alone program with ASan and UBSan linked in: names,
    a .b6 with the path columns, solve by bh_chimera_host, the table, the usage errors"""
    exe, prefix, b6_path = str(tmp_path / "chimera_host_main"), str(tmp_path / "SAN_"), str(tmp_path / "t.b6")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "chimera_host_main.c"), os.path.join(CSRC, "host", "bh_chimera.c"), os.path.join(CSRC, "host", "bh_cluster.c"),
                           os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    open(b6_path, "w").write(B6)
    r = subprocess.run([exe, prefix, b6_path], capture_output=True, text=True)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "chimera_host_main ok" in r.stdout, r.stdout + r.stderr
    assert "reads 1 and 3 of the query file are both named 'x'" in r.stdout
    assert open(prefix + "chimeras.txt").read() == ml.table_from_b6(NAMES, B6, True)
