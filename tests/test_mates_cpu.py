"""Paired-end reads (bh_mates.c, bh_session_run_mates: host.Session.run(q1, out, mates=q2), burst_hip --mates) where there is no device: the
session runs with the ORACLE as align back end (as tests/test_samples_cpu.py does) and the definition's brute force (tests/mateslib.py)
as the joiner, so everything around the kernels is the product's -- the two mates through the per-sample path, the collector, the
numbering of pairs and headers, the writer, the error rule.  The paired output must be, byte for byte, mateslib applied to the outputs
of two plain runs with the same session options."""
import os
import subprocess

import numpy as np
import pytest

import goldenlib as gl
import matesdata as md
import mateslib as ml
import test_samples_cpu as ts

TAX = os.path.join(gl.G, "tax.txt")
THRES = 0.95


def brute(a, b, orientation, ins_min, ins_max, report, cap):
    r = ml.join(a.tolist(), b.tolist(), ml.ORIENTATIONS[orientation], ins_min, ins_max, ml.REPORTS[report])
    return np.array([i for i, _ in r], np.uint32), np.array([j for _, j in r], np.uint32)


class Data:
    """the pair files, the database and an oracle back end that remembers what it has searched (a search per file and mode, not per test)"""
    def __init__(self, d):
        from burst_amd import host
        self.dir = d
        self.p1, self.p2, self.pairs = md.write_files(d)
        self.db = host.Db.read(ts.EDX)
        inner, self.seen, self.single_out = ts.make_align(self.db), {}, {}

        def align(qs, ranges, mode_no):
            key = (mode_no, tuple(ranges), qs.batch(*ranges[0]).codes.tobytes() if ranges else b"")
            if key not in self.seen:
                self.seen[key] = inner(qs, ranges, mode_no)
            return self.seen[key]
        self.align = align

    def session(self, mode, tax=False, **kw):
        from burst_amd import host
        if tax:
            kw["taxonomy"] = TAX
        return host.Session(self.db, None, accel=False, align=self.align, mode=mode, thres=THRES, rc=True, **kw)

    def single(self, mode, tax=False):
        """the two single-end outputs of the mode"""
        if (mode, tax) not in self.single_out:
            with self.session(mode, tax) as s:
                out = []
                for k, p in enumerate((self.p1, self.p2)):
                    o = os.path.join(self.dir, "single_%s_%d_%d.b6" % (mode, tax, k))
                    assert s.run(p, o)["rc"] == 0
                    out.append(open(o, "rb").read())
            self.single_out[(mode, tax)] = tuple(out)
        return self.single_out[(mode, tax)]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = Data(str(tmp_path_factory.mktemp("mates")))
    yield d
    d.db.close()


def pair_sets(b1, b2, orientation, ins_max):
    """per pair name: its reported combinations"""
    p1, p2 = ml.parse_b6(b1), ml.parse_b6(b2)
    a, b = ml.number_lines(p1, p2)
    out = {}
    for i, j in ml.join(a, b, orientation, 0, ins_max, "all"):
        out.setdefault(ml.pair_name(p1[i][0]), []).append((i, j))
    return out, a, b, p1, p2


def test_the_expected_set_is_not_vacuous(data):
    """asserted on the EXPECTED output alone (two single-end FORAGE runs + mateslib): the generator's cases are there"""
    b1, b2 = data.single("FORAGE")
    fr, a, b, p1, p2 = pair_sets(b1, b2, "fr", md.INSERT_MAX)
    wide = pair_sets(b1, b2, "fr", 1000)[0]
    ff = pair_sets(b1, b2, "ff", md.INSERT_MAX)[0]
    kind = {name.encode(): k for k, name, _, _ in data.pairs}
    assert sum(1 for v in fr.values() if len(v) > 1) >= 50
    assert sum(1 for n in wide if n not in fr and kind[n] == "long") >= 10                                              # the insert bound alone
    assert sum(1 for n in ff if n not in fr and n not in wide) >= 10                                                  # the orientation alone
    placed = {ml.pair_name(x[0]) for x in p1} & {ml.pair_name(x[0]) for x in p2}
    shared = {(la.pair, la.ref) for la in a} & {(lb.pair, lb.ref) for lb in b}
    named = {ml.pair_name(x[0]): la.pair for x, la in zip(p1, a)}
    assert sum(1 for n in placed if not any(p == named[n] for p, _ in shared)) >= 10                                   # the reference
    best = ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "best")
    assert best != ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all") and len(best) > 0
    # ALLPATHS: each mate's minimum-edit ties only
    a1, a2 = data.single("ALLPATHS")
    assert 200 <= len(pair_sets(a1, a2, "fr", md.INSERT_MAX)[0]) <= len(fr)
    assert {"/1" in x[0].decode() for x in p1} == {True, False}


@pytest.mark.parametrize("tax", [False, True])
@pytest.mark.parametrize("orientation", ["fr", "ff"])
@pytest.mark.parametrize("report", ["all", "best"])
@pytest.mark.parametrize("mode", ["ALLPATHS", "FORAGE"])
def test_paired_output_is_the_definition(data, mode, report, orientation, tax):
    b1, b2 = data.single(mode, tax)
    assert (b1.count(b"\t") == 12 * len(b1.splitlines())) == tax and len(b1) and len(b2)
    out = os.path.join(data.dir, "paired_%s_%s_%s_%d.b6" % (mode, report, orientation, tax))
    with data.session(mode, tax, mates_orientation=orientation, mates_report=report, insert_max=md.INSERT_MAX, mates_join=brute) as s:
        res = s.run(data.p1, out, mates=data.p2)
        assert res["rc"] == 0 and not s.ended, res
    exp = ml.paired_text(b1, b2, orientation, 0, md.INSERT_MAX, report)
    got = open(out, "rb").read()
    assert got == exp and len(exp) > 0
    assert sorted(os.listdir(data.dir)) == sorted(set(os.listdir(data.dir)) - {os.path.basename(out) + x for x in (".tmp", ".mate1.tmp", ".mate2.tmp")})
    c = ml.counts(b1, b2, md.names_of(data.p1), md.names_of(data.p2), orientation, 0, md.INSERT_MAX, report)
    m = res["mates"]
    assert (m["reads1"], m["reads2"], m["pairsNamed"], m["pairsPlaced"], m["examined"], m["written"]) == (c["reads1"], c["reads2"], c["named"], c["placed"], c["examined"], c["written"])
    assert (m["lines1"], m["lines2"], res["nLines"]) == (len(b1.splitlines()), len(b2.splitlines()), len(exp.splitlines()))


def test_pairs_between_plain_samples(data, tmp_path):
    """one session: q100, the pair, q292, the pair again -- the plain samples' outputs are the golden files, the pair's is the same both times"""
    o = [str(tmp_path / ("o%d.b6" % i)) for i in range(4)]
    with data.session("FORAGE", insert_max=md.INSERT_MAX, mates_join=brute) as s:
        s.prefetch(ts.Q100)
        assert s.run(ts.Q100, o[0])["rc"] == 0
        assert s.run(data.p1, o[1], mates=data.p2)["rc"] == 0
        s.prefetch(ts.Q292)
        assert s.run(ts.Q292, o[2])["rc"] == 0
        assert s.run(data.p1, o[3], mates=data.p2)["rc"] == 0
    # (-i 0.95 here: the golden FORAGE files of both query sets are -i 0.95 runs)
    assert sorted(open(o[0], "rb").read().splitlines()) == ts.golden("dna_q100_forage_noacx_t1_fr")
    assert sorted(open(o[2], "rb").read().splitlines()) == ts.golden("dna_q292_forage_noacx_t1_fr")
    b1, b2 = data.single("FORAGE")
    assert open(o[1], "rb").read() == open(o[3], "rb").read() == ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all")


def test_unreadable_mates_file_fails_alone(data, tmp_path):
    out = str(tmp_path / "pair.b6")
    with data.session("ALLPATHS", insert_max=md.INSERT_MAX, mates_join=brute) as s:
        for q1, q2 in ((data.p1, str(tmp_path / "absent.fa")), (str(tmp_path / "absent.fa"), data.p2)):
            res = s.run(q1, out, mates=q2)
            assert res["rc"] == ts.E_IO and "absent.fa" in res["err"] and not s.ended
            assert os.listdir(str(tmp_path)) == []
        assert s.run(data.p1, out, mates=data.p2)["rc"] == 0
    b1, b2 = data.single("ALLPATHS")
    assert open(out, "rb").read() == ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "all")
    assert os.listdir(str(tmp_path)) == ["pair.b6"]


def test_session_refuses_what_the_join_cannot_use(data, tmp_path):
    from burst_amd import host
    out = str(tmp_path / "pair.b6")
    for kw in (dict(mode="BEST", rc=True), dict(mode="CAPITALIST", rc=True), dict(mode="ANY", rc=True), dict(mode="ALLPATHS", rc=False)):
        with host.Session(data.db, None, accel=False, align=data.align, thres=THRES, mates_join=brute, **kw) as s:
            res = s.run(data.p1, out, mates=data.p2)
            assert res["rc"] == ts.E_USAGE and not s.ended and not os.path.exists(out), kw
    for kw in (dict(mates_orientation="fx"), dict(mates_report="some"), dict(insert_min=5, insert_max=4)):
        with pytest.raises(ValueError):
            host.Session(data.db, None, accel=False, align=data.align, mode="ALLPATHS", rc=True, **kw)


def test_capacity_answer_is_retried_once(data, tmp_path):
    calls = []

    def shy(a, b, orientation, ins_min, ins_max, report, cap):
        ia, ib = brute(a, b, orientation, ins_min, ins_max, report, cap)
        calls.append((cap, len(ia)))
        return cap + 7 if len(calls) == 1 else (ia, ib)      # (the first answer: room wanted, more than was offered)

    def greedy(a, b, orientation, ins_min, ins_max, report, cap):
        calls.append(cap)
        return cap + 1

    b1, b2 = data.single("FORAGE")
    exp = ml.paired_text(b1, b2, "fr", 0, 100000, "all")
    out = str(tmp_path / "pair.b6")
    with data.session("FORAGE", insert_max=100000, mates_join=shy) as s:
        assert s.run(data.p1, out, mates=data.p2)["rc"] == 0
    assert len(calls) == 2 and calls[1] == (calls[0][0] + 7, calls[0][1]) and open(out, "rb").read() == exp
    del calls[:]
    with data.session("FORAGE", insert_max=100000, mates_join=greedy) as s:      # a joiner that never has enough: tried twice, then the session ends
        res = s.run(data.p1, out + "2", mates=data.p2)
        assert res["rc"] < 0 and s.ended and len(calls) == 2 and calls[1] == calls[0] + 1
    assert os.listdir(str(tmp_path)) == ["pair.b6"]


DB_ARGS = ["-r", ts.EDX, "-ad", "-q", ts.Q100, "-o"]
REFUSED = [
    ("mode BEST", ["--mates", ts.Q292, "-m", "BEST"]), ("mode CAPITALIST", ["--mates", ts.Q292]), ("mode ANY", ["--mates", ts.Q292, "-m", "ANY"]),
    ("-x", ["--mates", ts.Q292, "-m", "ALLPATHS", "-x"]), ("-d", ["--mates", ts.Q292, "-m", "ALLPATHS", "-d", "QUICK"]),
    ("--make-acx", ["--mates", ts.Q292, "-m", "ALLPATHS", "--make-acx", "x.acx"]), ("--gather rccl", ["--mates", ts.Q292, "-m", "ALLPATHS", "--gather", "rccl"]),
    ("serial shards", ["--mates", ts.Q292, "-m", "ALLPATHS", "--gpus", "1", "--shards", "2"]),
    ("--cigar", ["--mates", ts.Q292, "-m", "ALLPATHS", "--cigar"]), ("--coverage", ["--mates", ts.Q292, "-m", "FORAGE", "--coverage", "cov_"]),
    ("--insert-min alone", ["-m", "ALLPATHS", "--insert-min", "5"]), ("--insert-max alone", ["-m", "ALLPATHS", "--insert-max", "5"]),
    ("--mates-orientation alone", ["-m", "ALLPATHS", "--mates-orientation", "ff"]), ("--mates-report alone", ["-m", "ALLPATHS", "--mates-report", "best"]),
    ("bad orientation", ["--mates", ts.Q292, "-m", "ALLPATHS", "--mates-orientation", "fx"]), ("bad report", ["--mates", ts.Q292, "-m", "ALLPATHS", "--mates-report", "x"]),
    ("min > max", ["--mates", ts.Q292, "-m", "ALLPATHS", "--insert-min", "700", "--insert-max", "600"]),
    ("with --samples", ["--mates", ts.Q292, "-m", "ALLPATHS", "--samples", "list.tsv"]),
]


@pytest.mark.parametrize("what,extra", REFUSED, ids=[w for w, _ in REFUSED])
def test_cli_refusals(tmp_path, what, extra):
    """exit code 1 before a device is touched (there is none here), and no output file"""
    out = str(tmp_path / "out.b6")
    r = subprocess.run([ts.CLI] + DB_ARGS + [out] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 1 and "ERROR" in r.stdout, (what, r.stdout[-800:])
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    assert "Device" not in r.stdout and "hip" not in r.stdout.split("\n", 1)[1].lower().replace("burst_hip", "")


def test_cli_refuses_fasta_references_and_mates_lines_in_a_list(tmp_path):
    refs = os.path.join(gl.G, "refs.fa")
    out = str(tmp_path / "out.b6")
    r = subprocess.run([ts.CLI, "-r", refs, "-q", ts.Q100, "--mates", ts.Q292, "-o", out, "-m", "ALLPATHS"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 1 and ".edx" in r.stdout and not os.path.exists(out)
    lst = tmp_path / "list.tsv"
    lst.write_text("%s\t%s\n%s\t%s\t%s\n" % (ts.Q100, tmp_path / "a.b6", ts.Q100, tmp_path / "b.b6", ts.Q292))
    for extra in (["-m", "BEST", "-fr"], ["-m", "ALLPATHS"], ["-m", "ALLPATHS", "-fr", "--cigar"]):      # the mode; no -fr; out of scope
        r = subprocess.run([ts.CLI, "-r", ts.EDX, "-ad", "--samples", str(lst)] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 1 and "ERROR" in r.stdout and "Device" not in r.stdout, r.stdout[-800:]
    lst.write_text("%s\t%s\n" % (ts.Q100, tmp_path / "a.b6"))      # mates options without a mates line
    r = subprocess.run([ts.CLI, "-r", ts.EDX, "-ad", "--samples", str(lst), "-m", "ALLPATHS", "-fr", "--insert-max", "500"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 1 and "--mates" in r.stdout
    lst.write_text("%s\t%s\t%s\textra\n" % (ts.Q100, tmp_path / "a.b6", ts.Q292))
    r = subprocess.run([ts.CLI, "-r", ts.EDX, "-ad", "--samples", str(lst), "-m", "ALLPATHS", "-fr"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 1 and "line 1" in r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["list.tsv"]


def test_python_launcher_refuses_mates():
    import sys
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", ts.EDX, "-q", ts.Q100, "-o", "x.b6", "--mates", ts.Q292], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, cwd=gl.ROOT, timeout=300)
    assert r.returncode != 0 and "--mates" in r.stdout and "burst_hip" in r.stdout


def test_pair_numbers_follow_the_lines_not_the_reads(data, tmp_path):
    """files of 300 000 reads each of which a few hundred place (the collector alone, no search): the pair numbers the joiner gets are dense
    over the pairs that HAVE lines -- bhip_mates_join keeps a table indexed by pair for `best` and refuses numbers far beyond the line
    count -- while the statistics still count every read"""
    import ctypes as C
    from burst_amd import host
    L = host.lib()
    L.bh_mates_open.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.bh_mates_names.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint64]
    L.bh_mates_join_files.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_uint32 * 4), C.POINTER(C.c_uint64)]
    L.bh_mates_close.argtypes = [C.c_void_p]
    L.bh_mates_close.restype = None
    libc = C.CDLL(None)
    libc.fopen.restype, libc.fopen.argtypes, libc.fclose.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p], [C.c_void_p]
    b1, b2 = data.single("FORAGE")
    f1, f2, out = tmp_path / "o1.b6", tmp_path / "o2.b6", tmp_path / "paired.b6"
    f1.write_bytes(b1)
    f2.write_bytes(b2)
    n_fill = 300000
    seen = []

    def joiner(ctx, a, na, b, nb, orientation, ins_min, ins_max, report, out_a, out_b, cap, n_out):
        la = np.frombuffer((C.c_uint8 * (int(na) * 20)).from_address(a), dtype=host.capi.MATE_LINE_DTYPE)
        lb = np.frombuffer((C.c_uint8 * (int(nb) * 20)).from_address(b), dtype=host.capi.MATE_LINE_DTYPE)
        seen.append((int(max(la["pair"].max(), lb["pair"].max())), len(set(la["pair"].tolist()) | set(lb["pair"].tolist())), int(na) + int(nb), int(cap)))
        ia, ib = brute(la, lb, orientation, ins_min, ins_max, report, cap)
        C.memmove(out_a, ia.ctypes.data, 4 * len(ia))
        C.memmove(out_b, ib.ctypes.data, 4 * len(ib))
        n_out[0] = len(ia)
        return 0
    cb = host.MATES_JOIN_FN(joiner)
    m = C.c_void_p()
    assert L.bh_mates_open(None, C.byref(m)) == 0
    L.bh_mates_set_join(m, cb, None)
    try:
        for side, path in enumerate((data.p1, data.p2)):
            names = [b"unplaced%07d/%d" % (i, side + 1) for i in range(n_fill)] + md.names_of(path)
            arr = (C.c_char_p * len(names))(*names)
            assert L.bh_mates_names(m, side, arr, len(names)) == 0
        fp = libc.fopen(str(out).encode(), b"wb")
        n_lines = C.c_uint64()
        opts = (C.c_uint32 * 4)(0, 0, md.INSERT_MAX, 1)      # fr, [0, INSERT_MAX], best
        rc = L.bh_mates_join_files(m, str(f1).encode(), str(f2).encode(), fp, C.byref(opts), C.byref(n_lines))
        libc.fclose(fp)
        assert rc == 0
        st = host.BhMatesStats()
        L.bh_mates_stats(m, C.byref(st))
    finally:
        L.bh_mates_close(m)
    max_pair, distinct, n, cap = seen[0]
    assert len(seen) == 1 and max_pair == distinct - 1 and distinct <= n < n_fill      # dense over the lines; far fewer lines than reads
    c = ml.counts(b1, b2, md.names_of(data.p1), md.names_of(data.p2), "fr", 0, md.INSERT_MAX, "best")
    assert cap == c["examined"] >= c["written"]                                           # the room offered is the upper bound: no second call
    assert (st.reads1, st.reads2, st.pairsNamed, st.pairsPlaced) == (n_fill + c["reads1"], n_fill + c["reads2"], n_fill + c["named"], c["placed"])
    assert out.read_bytes() == ml.paired_text(b1, b2, "fr", 0, md.INSERT_MAX, "best") and n_lines.value == 2 * c["written"] > 0


def test_measurement_tool_splits_fragments_into_mates(tmp_path):
    """tools/mates_e2e.py makes its mate files from the synthetic-read generator's output: one sequence line per record, mate 1 = the first
    100 bases under NAME/1, mate 2 = the reverse complement of the last 100 under NAME/2"""
    import importlib.util
    from burst_amd import host
    spec = importlib.util.spec_from_file_location("mates_e2e", os.path.join(gl.ROOT, "tools", "mates_e2e.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    frag, m1, m2 = (str(tmp_path / x) for x in ("frag.fa", "m1.fa", "m2.fa"))
    host.synth_reads(os.path.join(gl.G, "refs.fa"), frag, 50, 300, [0, 1, 2], rc=True, seed=43)
    raw = open(frag).read().splitlines()
    assert len(raw) == 100 and all(raw[i].startswith(">") and not raw[i + 1].startswith(">") for i in range(0, 100, 2))      # one sequence line per record
    iupac = dict(zip("ACGTRYKMBVDH", "TGCAYRMKVBHD"))      # (S, W and N are their own complements)
    keep = [i for i in range(0, 100, 2) if len(raw[i + 1]) >= 100]      # (a fragment drawn from a reference shorter than a mate is left out)
    assert len(keep) >= 45 and sum(1 for i in keep if 298 <= len(raw[i + 1]) <= 302) >= 40
    tool.split_fragments(frag, m1, m2)
    r1, r2 = open(m1).read().splitlines(), open(m2).read().splitlines()
    assert len(r1) == len(r2) == 2 * len(keep)
    for k, i in enumerate(keep):
        name = raw[i][1:].split()[0]
        assert (r1[2 * k], r2[2 * k]) == (">%s/1" % name, ">%s/2" % name)
        assert r1[2 * k + 1] == raw[i + 1][:100] and r2[2 * k + 1] == "".join(iupac.get(c, c) for c in reversed(raw[i + 1][-100:]))
    assert ml.pair_name(r1[0][1:].encode()) == ml.pair_name(r2[0][1:].encode())
