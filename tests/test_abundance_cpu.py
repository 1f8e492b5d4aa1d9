"""--abundance without a device: bh_em_host (the definition in plain C) against the Python model (tests/emlib.py) and the hand values of
the definition, the table writer behind a solver of the test's, the refusals of the command lines, and csrc/host/bh_em.c as a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import emlib as em
from burst_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")
ONE = em.ONE


def both(case, max_iters, tol):
    """bh_em_host and the model on one input: they agree in the counts and in info[0..4]; returns the model's"""
    nh, gw, ln = case
    counts, info = host.em_host(nh, gw, ln, max_iters, tol)
    want, winfo = em.em(nh, gw, ln, max_iters, tol)
    assert [int(x) for x in counts] == want
    assert [int(x) for x in info[:5]] == winfo and [int(x) for x in info[5:]] == [0, 0, 0]
    return want, winfo


@pytest.mark.parametrize("max_iters,tol,counts,info", [
    (1, 0, [5368709120, 3221225472, 0], [1, 12, 3, 4294967296, 0]),
    (2, 0, [5905580032, 2684354560, 0], [2, 12, 3, 536870912, 0]),
    (3, 0, [6174015488, 2415919104, 0], [3, 12, 3, 268435456, 0]),
    (1000, 1024, [6442449920, 2147484672, 0], [21, 12, 3, 1024, 1]),
    (1000, 0, [6442450944, 2147483648, 0], [31, 12, 3, 0, 1]),
], ids=["t1", "t2", "t3", "tol1024", "tol0"])
def test_hand_case_1(max_iters, tol, counts, info):
    """three reads on {A}, one on {B}, four on {A, B} (one with its A line twice): 13 lines, 12 distinct pairs, 3 classes; the fixed point is
    exactly 6 and 2 reads"""
    assert both(em.CASE1, max_iters, tol) == (counts, info)
    assert 6442450944 == 6 * ONE and 2147483648 == 2 * ONE


def test_hand_cases_2_3_4():
    assert both(em.CASE2, 1000, 1024) == ([357913942, 357913941, 357913941], [2, 3, 1, 0, 1])      # the rest goes to the lowest header of equals
    assert both(em.CASE3, 1000, 1024) == ([0, 1789569710, 1789569705, 1789569705], [2, 3, 1, 0, 1])
    assert both(em.CASE4, 1000, 1024) == ([ONE, ONE], [1, 2, 2, 0, 1])


@pytest.fixture(scope="module")
def random_case():
    case = em.random_case(1)
    trace = []
    em.em(*case, max_iters=100000, tol=0, trace=trace)
    return case, trace


@pytest.mark.parametrize("max_iters,tol", [(1, 0), (7, 0), (1000, 1024), (100000, 0)])
def test_random_case(random_case, max_iters, tol):
    case, trace = random_case
    nh, gw, ln = case
    assert trace[-1][2] == 0 and len(trace) < 1000                    # the model reaches an integer fixed point well inside the cap
    assert sum(1 for w in gw if not w) > 50 and len({h for _, h in ln}) == 60 and nh == 64
    counts, info = both(case, max_iters, tol)
    t = next((t for t, _, d in trace if d <= tol), len(trace))        # (the trace: the same model, run once to its fixed point)
    t = min(t, max_iters)
    assert info[0] == t and counts == trace[t - 1][1] and info[3] == trace[t - 1][2]
    assert sum(counts) == ONE * sum(gw[g] for g in {g for g, _ in ln})
    assert all(c == 0 for c in counts[60:])


def test_golden_b6():
    """tests/golden/dna_q100_allpaths_fr.b6: 588 lines of 497 reads on 73 headers"""
    headers, gw, ln, reads = em.b6_groups(open(os.path.join(GOLDEN, "dna_q100_allpaths_fr.b6")).read())
    assert (len(ln), len(reads), len(headers)) == (588, 497, 73)
    sizes = [len(s) for s in em.candidate_sets(len(headers), gw, ln).values()]
    assert [sizes.count(k) for k in (1, 2, 3, 4)] == [427, 61, 7, 2] and len(sizes) == 497
    counts, info = both((len(headers), gw, ln), 1000, 1024)
    assert info[0] == 10 and info[2] == 94 and info[3] == 299 and info[4] == 1
    assert sum(counts) == 497 * ONE


def test_bad_arguments():
    nh, gw, ln = em.CASE4
    for args in ((nh, gw, [(0, 0), (2, 1)]), (nh, gw, [(0, 2)]), (nh, [0x7FFFFFFF, 1], ln)):
        with pytest.raises(host.HostError, match="error -1"):
            host.em_host(*args)
    with pytest.raises(host.HostError, match="error -1.*max_iters"):
        host.em_host(nh, gw, ln, max_iters=0)
    lines = capi.em_lines(ln)
    counts, info = np.zeros(nh, np.uint64), np.zeros(8, np.uint64)
    gwa = np.asarray(gw, np.uint32)
    assert host.lib().bh_em_host(None, nh, 2, gwa.ctypes.data, lines.ctypes.data, 1 << 31, 10, 0, counts.ctypes.data, info.ctypes.data) == host.E_USAGE
    # weights that sum to exactly 2^31 - 1 are taken; a group of 2^31 reads WITHOUT a line takes no part
    c, _ = host.em_host(nh, [0x7FFFFFFE, 1, 0x80000000], ln)
    assert [int(x) for x in c] == [0x7FFFFFFE * ONE, ONE]
    # nothing takes part
    c, info = host.em_host(3, [0, 0], [(0, 1), (1, 2)])
    assert not c.any() and not info.any()
    c, info = host.em_host(3, [], [])
    assert not c.any() and not info.any()


class Table:
    """bh_em.c's table behind a solver of the test's: solver(n_headers, group_w, lines, max_iters, tol) -> counts, or an int = its error"""

    def __init__(self, prefix, heads, solver, max_iters=1000, tol=1024):
        self.h = C.c_void_p()
        self.calls = []
        arr = (C.c_char_p * len(heads))(*[x.encode() for x in heads])
        rc = host.lib().bh_em_open_heads(prefix.encode(), len(heads), arr, max_iters, tol, C.byref(self.h))
        assert rc == 0, rc

        def _solve(ctx, nh, ng, gw, lines, n, iters, tol_, counts, info):
            g = np.frombuffer((C.c_uint8 * (4 * ng)).from_address(gw), np.uint32).copy() if ng else np.zeros(0, np.uint32)
            ln = np.frombuffer((C.c_uint8 * (8 * n)).from_address(lines), capi.EM_LINE_DTYPE).copy() if n else np.zeros(0, capi.EM_LINE_DTYPE)
            self.calls.append((int(nh), g, ln, int(iters), int(tol_)))
            r = solver(int(nh), g, ln, int(iters), int(tol_))
            if isinstance(r, int):
                return r
            out = np.asarray(r, np.uint64)
            C.memmove(counts, out.ctypes.data, 8 * nh)
            return 0
        self.cb = host.EM_SOLVER_FN(_solve)
        host.lib().bh_em_set_solver(self.h, C.cast(self.cb, C.c_void_p), None)

    def sample(self, name, reads, refs, weights):
        reads = np.asarray(reads, np.uint32)
        pl = np.zeros(len(refs), capi.COV_LINE_DTYPE)
        pl["ref"], pl["st"], pl["ed"], pl["w"] = refs, 1, 50, weights
        return host.lib().bh_em_sample(self.h, None, name.encode(), reads.ctypes.data, pl.ctypes.data, len(pl))

    def stats(self):
        nc, nh = C.c_uint32(), C.c_uint32()
        host.lib().bh_em_dims(self.h, C.byref(nc), C.byref(nh))
        cols = np.zeros((nc.value, nh.value), np.uint64)
        assert host.lib().bh_em_stats(self.h, cols.ctypes.data) == 0
        return cols

    def close(self):
        host.lib().bh_em_close(self.h)


def model_solver(nh, gw, ln, iters, tol):
    return em.em(nh, gw, [(int(a), int(b)) for a, b in zip(ln["group"], ln["ref"])], iters, tol)[0]


def test_table_rows_columns_and_dataset(tmp_path):
    """rows in strcmp order of the whole header, none for a header whose Dataset is zero; a failed sample's column is all zero; Dataset = the sum of the sample columns; the groups are the unique queries with their reads as weight"""
    heads = ["zeta", "Zebra x", "alpha", "alpha 2", "never"]
    prefix = str(tmp_path / "st_")
    t = Table(prefix, heads, model_solver, max_iters=1000, tol=0)
    # sample 1: query 0 (3 reads, unique flag set) on zeta; query 2 (2 reads) on {alpha, Zebra x}, alpha twice; query 5 (1 read) on alpha
    assert t.sample("/x/y/first.b6", [0, 2, 2, 2, 5], [0, 2, 1, 2, 2], [3 | 0x80000000, 2, 2, 2, 1]) == 0
    assert host.lib().bh_em_sample_failed(t.h, b"broken.sample.b6") == 0
    assert t.sample("third", [1, 9], [3, 1], [4, 1]) == 0
    nh, gw, ln, iters, tol = t.calls[0]
    assert (nh, iters, tol) == (5, 1000, 0) and list(gw) == [3, 0, 2, 0, 0, 1]
    assert sorted(zip(ln["group"].tolist(), ln["ref"].tolist())) == [(0, 0), (2, 1), (2, 2), (2, 2), (5, 2)]
    cols = t.stats()
    want1 = em.em(5, [3, 0, 2, 0, 0, 1], [(0, 0), (2, 2), (2, 1), (2, 2), (5, 2)], 1000, 0)[0]
    assert cols[1].tolist() == want1 and want1 == [3 * ONE, 0, 3 * ONE, 0, 0]
    assert not cols[2].any() and cols[3].tolist() == [0, ONE, 0, 4 * ONE, 0]
    assert (cols[0] == cols[1] + cols[2] + cols[3]).all()
    assert host.lib().bh_em_write(t.h) == 0
    t.close()
    assert sorted(os.listdir(str(tmp_path))) == ["st_abundance.txt"]
    text = open(prefix + "abundance.txt").read()
    assert text == ("#OTU ID\tDataset\tfirst\tbroken.sample\tthird\n"
                    "Zebra x\t1.0000\t0.0000\t0.0000\t1.0000\n"
                    "alpha\t3.0000\t3.0000\t0.0000\t0.0000\n"
                    "alpha 2\t4.0000\t0.0000\t0.0000\t4.0000\n"
                    "zeta\t3.0000\t3.0000\t0.0000\t0.0000\n")
    assert text == em.table_text(heads, ["first", "broken.sample", "third"], [cols[1].tolist(), cols[2].tolist(), cols[3].tolist()])


def test_table_cells_are_fractions_of_2_30(tmp_path):
    prefix = str(tmp_path / "f_")
    t = Table(prefix, ["a", "b", "c"], model_solver)
    assert t.sample("s.b6", [0, 0, 0], [0, 1, 2], [1, 1, 1]) == 0
    assert host.lib().bh_em_write(t.h) == 0
    t.close()
    assert open(prefix + "abundance.txt").read() == "#OTU ID\tDataset\ts\na\t0.3333\t0.3333\nb\t0.3333\t0.3333\nc\t0.3333\t0.3333\n"


def test_nothing_written_after_abort_or_solver_error(tmp_path):
    prefix = str(tmp_path / "ab_")
    t = Table(prefix, ["a", "b"], model_solver)
    assert t.sample("s.b6", [0], [0], [1]) == 0
    host.lib().bh_em_abort(t.h)
    assert host.lib().bh_em_write(t.h) == host.E_DEVICE
    assert t.sample("s2.b6", [0], [0], [1]) == host.E_DEVICE
    t.close()
    t = Table(prefix, ["a", "b"], lambda *a: host.E_DEVICE)
    assert t.sample("s.b6", [0], [0], [1]) == host.E_DEVICE
    assert host.lib().bh_em_write(t.h) == host.E_DEVICE      # (a solver's error is final)
    t.close()
    # without a solver and without a device handle: an error, not a table from somewhere else
    h = C.c_void_p()
    arr = (C.c_char_p * 1)(b"a")
    assert host.lib().bh_em_open_heads(prefix.encode(), 1, arr, 10, 0, C.byref(h)) == 0
    reads, pl = np.zeros(1, np.uint32), np.zeros(1, capi.COV_LINE_DTYPE)
    pl["w"] = 1
    assert host.lib().bh_em_sample(h, None, b"s.b6", reads.ctypes.data, pl.ctypes.data, 1) == host.E_DEVICE
    host.lib().bh_em_close(h)
    assert os.listdir(str(tmp_path)) == []


def test_host_solver_through_the_table(tmp_path):
    """bh_em_host as the table's solver on the golden lines: the table the model writes"""
    headers, gw, ln, reads = em.b6_groups(open(os.path.join(GOLDEN, "dna_q100_allpaths_fr.b6")).read())
    prefix = str(tmp_path / "g_")
    h = C.c_void_p()
    arr = (C.c_char_p * len(headers))(*[x.encode() for x in headers])
    assert host.lib().bh_em_open_heads(prefix.encode(), len(headers), arr, 1000, 1024, C.byref(h)) == 0
    host.lib().bh_em_set_solver(h, C.cast(host.lib().bh_em_host, C.c_void_p), None)
    uq = np.asarray([g for g, _ in ln], np.uint32)
    pl = np.zeros(len(ln), capi.COV_LINE_DTYPE)
    pl["ref"], pl["w"] = [r for _, r in ln], 1
    assert host.lib().bh_em_sample(h, None, b"out/golden.b6", uq.ctypes.data, pl.ctypes.data, len(pl)) == 0
    info, nreads = np.zeros(8, np.uint64), C.c_uint64()
    host.lib().bh_em_last_info(h, info.ctypes.data, C.byref(nreads))
    assert info[:5].tolist() == [10, 578, 94, 299, 1] and nreads.value == 497
    assert host.lib().bh_em_write(h) == 0
    host.lib().bh_em_close(h)
    want = em.em(len(headers), gw, ln, 1000, 1024)[0]
    assert open(prefix + "abundance.txt").read() == em.table_text(headers, ["golden"], [want])


REFUSALS = [
    (["-x"], "-x"),
    (["-d", "DNA"], "-d"),
    (["--make-acx", "x.acx"], "--make-acx"),
    (["--gpus", "1", "--shards", "2"], "--shards"),
    (["--mates", os.path.join(GOLDEN, "q292.fa")], "mates"),
]


@pytest.mark.parametrize("extra,word", REFUSALS, ids=[w for _, w in REFUSALS])
@pytest.mark.parametrize("samples", [False, True], ids=["single", "samples"])
def test_refusals_before_a_device_is_touched(tmp_path, extra, word, samples):
    """usage errors, exit code 1, with nothing read, no device opened (this machine may have none) and no file left"""
    out = tmp_path / "o.b6"
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\n")
    base = ["--samples", str(lst)] if samples else ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", str(out)]
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--abundance", str(tmp_path / "P")] + base + extra, capture_output=True, text=True)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --abundance" in r.stdout and word in r.stdout, r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["list.txt"]


def test_mates_line_in_a_sample_list_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\tb.fa\n")
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "-fr", "--abundance", str(tmp_path / "P"), "--samples", str(lst)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: --abundance" in r.stdout and "mates" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["list.txt"]


@pytest.mark.parametrize("extra", [["--abundance-iters", "5"], ["--abundance-tol", "0"], ["--abundance", "P", "--abundance-iters", "0"],
                                   ["--abundance", "P", "--abundance-tol", "-3"], ["--abundance"]], ids=["iters-alone", "tol-alone", "iters-0", "tol-negative", "no-prefix"])
def test_option_errors(tmp_path, extra):
    out = tmp_path / "o.b6"
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-q", os.path.join(GOLDEN, "q100.fa"), "-o", str(out)] + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "abundance" in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--abundance", "P"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--abundance is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--abundance <prefix>" in r.stdout and "--abundance-iters" in r.stdout and "--abundance-tol" in r.stdout


def test_host_file_under_sanitizers(tmp_path):
    """csrc/host/bh_em.c as a stand-alone program (tests/csrc/em_host_main.c), built with the address and the undefined-behaviour
    sanitizer: the hand cases, the refusals, the table with a failed sample"""
    exe, prefix = str(tmp_path / "em_host_main"), str(tmp_path / "t_")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "em_host_main.c"), os.path.join(CSRC, "host", "bh_em.c"), os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    r = subprocess.run([exe, prefix], capture_output=True, text=True)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "em_host_main ok" in r.stdout, r.stdout + r.stderr
    assert open(prefix + "abundance.txt").read() == ("#OTU ID\tDataset\tone\ttwo\tthree\n"
                                                     "alpha\t2.0000\t2.0000\t0.0000\t0.0000\n"
                                                     "zeta\t9.0000\t6.0000\t0.0000\t3.0000\n")


def test_exports_and_dtype():
    assert "bhip_em_run" in capi.EXPORTS and capi.EM_LINE_DTYPE.itemsize == 8 and capi.EM_LINE_DTYPE.names == ("group", "ref")
    assert capi.lib().bhip_abi_version() == 8
