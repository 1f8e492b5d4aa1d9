"""--cigar without a device: the full-matrix restatement of the canonical alignment path (tests/cigar_restate.c) pinned to the oracle's
re-scorer, the host's renderer and collector (also as a stand-alone program under the address and undefined-behaviour sanitizers), the
refusals of the command lines, and the exports."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cigarlib as cg
import oraclelib as ol

ROOT = cg.ROOT
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


def random_pairs(n, seed):
    """(query, lane, bound): reads cut from the lane with substitutions, insertions and deletions; random, homopolymer and tandem-repeat
    lanes; IUPAC symbols on both sides; trailing pads; some reads from the first and the last columns"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = ("random", "homopolymer", "tandem")[i % 3]
        n_ref = int(rng.integers(40, 260))
        lane = cg.random_lane(rng, n_ref, kind)
        if i % 4 == 0:      # ambiguity codes in the reference
            for p in rng.choice(n_ref, size=3, replace=False):
                lane[p] = int(rng.integers(5, 16))
        m = int(rng.integers(2, min(120, n_ref - 4)))
        start = 0 if i % 7 == 0 else (n_ref - m if i % 7 == 1 else int(rng.integers(0, n_ref - m + 1)))
        ns, ni, nd = (int(x) for x in rng.integers(0, 3, size=3))
        q = cg.edit_read(rng, lane, start, m, ns, ni, nd)
        if i % 5 == 0 and len(q) > 4:      # ... and in the query
            q[int(rng.integers(0, len(q)))] = int(rng.integers(5, 16))
        pads = int(rng.integers(0, 6)) if i % 2 else 0
        lane = np.concatenate([lane, np.zeros(pads, np.uint8)])
        out.append((q, lane, ns + ni + nd + int(rng.integers(0, 3))))
    return out


@pytest.mark.parametrize("z", [1, 0])
def test_restatement_is_the_oracles_rescorer_with_decisions(L, z):
    lut = ol.score_lut(z)
    n_hits = n_multi = n_gaps = 0
    for q, lane, bound in random_pairs(400, 7 + z):
        ok_o, h = ol.rescore_lane(q, lane, bound, lut)
        ok, ops, o = cg.trace(L, q, lane, bound, lut)
        assert ok == ok_o
        if not ok:
            continue
        n_hits += 1
        assert (o.ed, o.gapQ, o.gapR, o.finalPos) == (int(h["ed"]), int(h["gapQ"]), int(h["gapR"]), int(h["finalPos"]))
        if o.n_best_cols == 1:
            assert o.v_final == int(h["gapR"])      # one best end column: V of the final cell IS the record's gapR
        else:
            n_multi += 1
        # what follows by construction
        assert o.n_EQ + o.n_X + o.n_I == len(q)
        assert o.n_X + o.n_I + o.n_D == o.ed
        assert o.n_D == o.gapQ
        assert o.n_I == o.v_final
        assert 1 <= o.ref_first <= o.finalPos + 1 and o.ref_first + o.n_EQ + o.n_X + o.n_D - 1 == o.finalPos
        lens = {c: 0 for c in "=XID"}
        for w in ops:
            lens[cg.OP_CHAR[int(w) & 15]] += int(w) >> 4
        assert (lens["="], lens["X"], lens["I"], lens["D"]) == (o.n_EQ, o.n_X, o.n_I, o.n_D)
        assert all((int(a) & 15) != (int(b) & 15) for a, b in zip(ops[:-1], ops[1:])), "runs are merged"
        n_gaps += bool(o.n_I or o.n_D)
        # replay: every '=' pair costs 0 and every 'X' pair costs 1 under the table
        x, y = o.ref_first - 1, 0
        for w in ops:
            n, c = int(w) >> 4, cg.OP_CHAR[int(w) & 15]
            for _ in range(n):
                if c in "=X":
                    assert lut[16 * int(q[y]) + int(lane[x])] == (0 if c == "=" else 1)
                    x += 1; y += 1
                elif c == "I":
                    y += 1
                else:
                    x += 1
        assert (x, y) == (o.finalPos, len(q))
        # the same path when the record's end column and score are handed in, as bhip_trace_paths gets them
        ok2, ops2, o2 = cg.trace(L, q, lane, o.ed, lut, final_pos=o.finalPos)
        assert ok2 and np.array_equal(ops, ops2) and o2.ref_first == o.ref_first
        ok3, _, _ = cg.trace(L, q, lane, o.ed - 1, lut, final_pos=o.finalPos) if o.ed else (False, None, None)
        assert not ok3      # one too low: the cell does not score it
    assert n_hits > 300 and n_gaps > 100 and n_multi > 0


def test_row1_case_and_leading_insertion(L):
    lut = ol.score_lut(1)
    # the first base matches and the next reference symbol is deleted: the reference's row-1 special case (burst.c:722-739)
    lane = np.array([3, 3, 1, 4, 2, 2, 3, 1, 4, 4, 2, 1, 3, 3], np.uint8)      # G G A T C C G A T T C A G G
    q = np.array([1, 2, 2, 3, 1, 4], np.uint8)                                  # A - C C G A T: A matches column 3, T (column 4) is skipped
    ok, ops, o = cg.trace(L, q, lane, 1, lut)
    assert ok and cg.text_of(ops) == "1=1D5=" and o.ref_first == 3 and o.finalPos == 9
    # a query symbol in front of column 1: the path reaches row 0 through column 0
    lane = np.array([2, 3, 1, 4, 4, 2, 1, 3], np.uint8)
    q = np.array([1, 1, 2, 3, 1, 4, 4], np.uint8)
    ok, ops, o = cg.trace(L, q, lane, 2, lut)
    assert ok and o.ed == 2 and cg.text_of(ops).startswith("2I") and o.ref_first == 1


def test_renderer_on_hand_written_ops():
    from burst_amd import host
    assert host.cigar_text([100 << 4 | 7]) == "100="
    assert host.cigar_text([5 << 4 | 7, 1 << 4 | 8, 2 << 4 | 1, 94 << 4 | 7, 3 << 4 | 2, 1 << 4 | 7]) == "5=1X2I94=3D1="
    assert host.cigar_text(cg.ops_of("1I1D1X1=4095=")) == "1I1D1X1=4095="
    assert host.cigar_text([0xFFFFFFF << 4 | 2]) == "268435455D"
    for bad in ([4 << 4 | 0], [4 << 4 | 3], [7], []):      # M, N, a zero length, no ops: not a path
        with pytest.raises(host.HostError):
            host.cigar_text(bad)
    from burst_amd import capi
    assert capi.cigar_text(cg.ops_of("7=1X3=")) == "7=1X3="


def test_host_collector_and_renderer_under_sanitizers(tmp_path):
    """csrc/host/bh_paths.c as a stand-alone program with a fake tracer (tests/cigar_host_main.c), built with the address and the
    undefined-behaviour sanitizer: record dedup, the capacity retry, lines rewritten with their two columns, mismatched inputs refused"""
    exe, out = str(tmp_path / "cigar_host_main"), str(tmp_path / "out.txt")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(cg.HERE, "cigar_host_main.c"), os.path.join(CSRC, "host", "bh_paths.c"), os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    r = subprocess.run([exe, out], capture_output=True, text=True)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "cigar_host_main ok" in r.stdout, r.stdout + r.stderr
    lines = open(out).read().split("\n")
    assert lines[7] == "read7\tref\t7\t1008\t107=1X108=1X109=1X110="
    assert lines[0] == "read0\tref\t0\t1001\t100="
    assert lines[300] == "dup299\tref\tx\ty\t300\t399=1X400=1X401=1X402="
    assert lines[301] == "third0\t6\t100="
    assert len(lines) == 300 + 300 + 60 + 60 + 1 and lines[-1] == ""
    assert lines[660].startswith("big0\t1\t1=1X2=1X") and lines[660].count("X") == 200


REFUSALS = [
    (["-x"], "-x"),
    (["-d", "DNA"], "-d"),
    (["--make-acx", "x.acx"], "--make-acx"),
    (["--shard", "db"], "--shard db"),
    (["--shards", "2"], "--shard"),
    (["--gather", "rccl"], "rccl"),
]


@pytest.mark.parametrize("extra,word", REFUSALS, ids=[w for _, w in REFUSALS])
@pytest.mark.parametrize("samples", [False, True], ids=["single", "samples"])
def test_refusals_before_a_device_is_touched(tmp_path, extra, word, samples):
    """usage errors, exit code 1, with nothing read and no device opened (this machine has none: anything else would fail differently)"""
    out = tmp_path / "o.b6"
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\n")
    base = ["--samples", str(lst)] if samples else ["-q", os.path.join(ROOT, "tests", "golden", "q100.fa"), "-o", str(out)]
    r = subprocess.run([BURST_HIP, "-r", os.path.join(ROOT, "tests", "golden", "quick.edx"), "--cigar"] + base + extra, capture_output=True, text=True)
    assert r.returncode == 1, r.stdout + r.stderr
    assert re.search(r"ERROR: --cigar .*" + re.escape(word.split()[0]), r.stdout), r.stdout
    assert not out.exists() and not (tmp_path / "a.b6").exists()


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--cigar"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--cigar is not available" in r.stderr


def test_help_names_the_flag():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--cigar" in r.stdout


def test_exports_match_the_header():
    from burst_amd import capi
    src = open(os.path.join(ROOT, "include", "burst_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(bhip_[a-z_]+)\s*\(", src))
    assert {"bhip_trace_paths", "bhip_paths_info"} <= declared and declared == set(capi.EXPORTS)
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "bhip_trace_paths") and hasattr(lib, "bhip_paths_info")
    assert lib.bhip_abi_version() == 8 and capi.PATH_REQ_DTYPE.itemsize == 16
    hostlib = ctypes.CDLL(os.path.join(ROOT, "burst_amd", "libburst_host.so"))
    for s in ("bh_paths_open", "bh_paths_emit", "bh_paths_close", "bh_cigar_text", "bh_report_view_paths"):
        assert hasattr(hostlib, s), s


@pytest.mark.parametrize("name,threads", [("dna_q100_allpaths_y", "1"), ("quick_q292_best_fr", "5:37"), ("dna_q100_forage_tax_noacx_t1_fr", "3:50")])
def test_report_with_paths_on_the_cpu(name, threads, tmp_path, L, monkeypatch):
    """bh_report_view_paths with the restatement as its tracer (bh_paths_set_trace) over the oracle's records of a golden case: the lines
    without their last two columns are the plain report's bytes, and every CIGAR passes the checks of the GPU command-line test (sums
    against the line's own columns, the replay over refs.fa) -- also with the chunks rendered by several threads"""
    import ctypes as C
    import goldenlib as gl
    import importlib
    from burst_amd import capi, host
    cli = importlib.import_module("test_gpu_cigar_cli")
    monkeypatch.setenv("BURST_HOST_REPORT_THREADS", threads)
    c = [x for x in gl.cases() if x["name"] == name][0]
    ref, q, fr, z, shear = gl.case_args(c)
    db = host.Db.read(ref)
    qs = host.QuerySet(q, float(c["id"]), rc=bool(fr), accel=False, z=z)
    lut = ol.score_lut(z)
    clump_len = host._view(db.c.clumpLen, db.c.numRclumps, np.uint32)
    packed = host._view(db.c.packed, db.c.packedWords * 16, np.uint8)
    b = qs.batch(0, qs.n_uniq)
    h = ol.search(packed, clump_len, db.c.totR, b.codes, b.off, b.emac.astype(np.uint32), b.six, b.rc, b.n_shared, lut, c["mode"] == "FORAGE").copy()
    h["q"] = b.entry_index[h["q"]].astype(np.uint32)
    h = np.ascontiguousarray(h.view(capi.HIT_DTYPE))
    codes = host._view(qs.c.codes, int(qs.c.qoff[qs.c.numEntries]), np.uint8)
    qoff = host._view(qs.c.qoff, qs.c.numEntries + 1, np.uint64)
    coff = np.concatenate([[0], np.cumsum((clump_len.astype(np.int64) + 1) // 2)]) * 16
    calls = []

    def tracer(ctx, Q, req, n, ops, cap, off, first, gap_r):
        try:
            r = np.frombuffer((C.c_uint8 * (16 * n)).from_address(req), capi.PATH_REQ_DTYPE)
            out, tot = [], 0
            off[0] = 0
            for i in range(n):
                cl = int(r["refIx"][i]) >> 4
                rows = ol.unpack_clump(packed[int(coff[cl]):int(coff[cl + 1])], int(clump_len[cl]))
                qq = codes[int(qoff[r["q"][i]]):int(qoff[r["q"][i] + 1])]
                ok, o_ops, o = cg.trace(L, qq, rows[:, int(r["refIx"][i]) & 15], int(r["ed"][i]), lut, final_pos=int(r["finalPos"][i]))
                assert ok
                out.append(o_ops); tot += len(o_ops)
                off[i + 1] = tot; first[i] = o.ref_first; gap_r[i] = o.n_I
            calls.append((n, tot, cap))
            if tot > cap:
                return -6      # BH_E_CAPACITY
            for i in range(n):
                for k, w in enumerate(out[i]):
                    ops[int(off[i]) + k] = int(w)
            return 0
        except Exception:      # (an exception must not cross the C frame)
            import traceback
            traceback.print_exc()
            return -4
    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    cb = FN(tracer)
    lib = host.lib()
    lib.bh_paths_set_trace.argtypes = [C.c_void_p, FN, C.c_void_p]
    lib.bh_paths_set_trace.restype = None
    tax, bs, strict, cut = gl.tax_args(c)
    T, to = host.BhTax(), host.BhTaxOpts()
    if tax:
        assert lib.bh_tax_load(tax.encode(), C.byref(T)) == 0
        to.tax, to.suppress, to.strict, to.taxacut = C.pointer(T), bs, strict, cut
    outs = {}
    for flag in (False, True):
        path = str(tmp_path / ("cigar.b6" if flag else "plain.b6"))
        f = host.libc.fopen(path.encode(), b"wb")
        paths = C.c_void_p()
        if flag:
            assert lib.bh_paths_open(None, C.byref(paths)) == 0
            lib.bh_paths_set_trace(paths, cb, None)
        view = host.BhRunView()
        view.base, view.n_runs, view.total = h.ctypes.data, 1, len(h)
        view.off[0], view.n[0] = 0, len(h)
        nl = C.c_uint64()
        rc = lib.bh_report_view_paths(f, C.byref(db.c), C.byref(qs.c), C.byref(view), host.MODES[c["mode"]], host.REP_MERGED_LIST, C.byref(to) if tax else None, C.byref(nl), None, paths)
        host.libc.fclose(f)
        assert rc == 0, lib.bh_last_error()
        if flag:
            nr, no, nln = C.c_uint64(), C.c_uint64(), C.c_uint64()
            lib.bh_paths_totals(paths, C.byref(nr), C.byref(no), C.byref(nln))
            assert nln.value == nl.value == c["lines"] and 0 < nr.value <= len(h) and nr.value == sum(x[0] for x in calls if x[1] <= x[2])
            lib.bh_paths_close(paths)
        outs[flag] = open(path, "rb").read()
    cli.check_lines(outs[True], outs[False], c["queries"], bool(tax), z == 1, L)
