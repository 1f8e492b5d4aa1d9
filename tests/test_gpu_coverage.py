"""Coverage and count tables on the MI355X (burst_hip --coverage; csrc/bhip_cov.hip, host/bh_cov.c): the device's integer statistics
against dense numpy depth arrays (tests/covlib.py), coordinates up to 2^32 - 1, the lane extents, the command line against the
reference's bcov tables (tests/golden/cov) and a study of three samples against the numpy restatement of the definitions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covlib
import goldenlib as gl
from test_coverage_cpu import COV, LEN, db_headers, default_lengths, lane_lengths

pytestmark = pytest.mark.gpu
CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
Q100, Q292 = os.path.join(gl.G, "q100.fa"), os.path.join(gl.G, "q292.fa")
LENGTHS = [1, 2, 37, 1600, 70000]
_dev, _case = {}, {}


def small_device():
    """a handle on a small database: the coverage calls need a handle, not its references"""
    if "d" not in _dev:
        import dbutil
        import oraclelib as ol
        from burst_amd import capi
        rng = np.random.default_rng(5)
        seqs = [rng.integers(1, 5, size=int(n), dtype=np.uint8) for n in rng.integers(90, 400, size=40)]
        packed, clump_len, tot = dbutil.pack_clumps(seqs)
        _dev["d"] = capi.Device(packed, clump_len, tot, ol.score_lut(1))
        _dev["seqs"] = seqs
    return _dev["d"]


def lines_of(ref, st, ed, w, uniq):
    from burst_amd import capi
    a = np.zeros(len(ref), capi.COV_LINE_DTYPE)
    a["ref"], a["st"], a["ed"] = ref, st, ed
    a["w"] = np.asarray(w, np.uint32) | (np.asarray(uniq, np.uint32) << 31)
    return a


def study():
    """three samples (the second empty) of about 20 000 lines over five references of lengths 1, 2, 37, 1 600 and 70 000: ranges clamped
    at both ends, empty ranges, st > ed, weights > 1, 3 000 identical lines on the 37-base reference (depth^2 = 9 * 10^6 > 2^23), and on
    the 70 000-base reference coordinates from a grid, so that the events are many and the distinct positions few (the compaction case)"""
    if "s" in _case:
        return _case["s"]
    rng = np.random.default_rng(11)

    def block(ref, st, ed, w=None, uniq=None):
        n = len(st)
        return [np.full(n, ref, np.int64), np.asarray(st, np.int64), np.asarray(ed, np.int64), np.ones(n, np.int64) if w is None else np.asarray(w, np.int64),
                rng.integers(0, 2, n).astype(bool) if uniq is None else np.asarray(uniq, bool)]

    def spread(n, ref, L, grid):
        st = 1 + grid * rng.integers(0, L // grid + 3, n)              # (the last grid points lie beyond the reference's end)
        ed = st + rng.choice([0, 49, 99, 150, 291], n)
        flip = rng.integers(0, 2, n).astype(bool)
        return block(ref, np.where(flip, ed, st), np.where(flip, st, ed), rng.integers(1, 6, n))
    s0 = [block(0, np.ones(1000), np.r_[np.full(950, 2), np.ones(50)]),           # the 1-base reference: [0, 1), and 50 empty ranges (with pad 0)
          block(1, np.ones(300), rng.integers(2, 5, 300)),                        # the 2-base reference, clamped at its end
          block(2, np.full(3000, 3), np.full(3000, 30), uniq=np.ones(3000)),
          spread(1000, 3, 1600, 1), spread(8800, 4, 70000, 137)]
    s2 = [block(0, np.ones(20), np.full(20, 2)), block(1, np.full(30, 2), np.ones(30)), spread(1500, 3, 1600, 1), spread(4500, 4, 70000, 137)]
    _case["s"] = [tuple(np.concatenate([b[k] for b in s]) for k in range(5)) for s in (s0, s2)]
    return _case["s"]


def expected(pad):
    """[Dataset, sample 0, sample 1 (empty), sample 2] -> (shared, unique) from dense depth arrays, computed once per pad"""
    if ("e", pad) not in _case:
        s0, s2 = study()
        zero = (np.zeros((5, 4), np.uint64), np.zeros((5, 4), np.uint64))
        _case[("e", pad)] = [covlib.dense_stats(*(np.concatenate([a, b]) for a, b in zip(s0, s2)), LENGTHS, pad), covlib.dense_stats(*s0, LENGTHS, pad), zero,
                             covlib.dense_stats(*s2, LENGTHS, pad)]
    return _case[("e", pad)]


@pytest.mark.parametrize("pad,cap", [(0, 0), (5, 0), (0, 320 << 10)])
def test_device_statistics_against_dense_depth_arrays(pad, cap):
    """5: tot, cov, sq and lines exactly equal for every reference, in every sample column and Dataset, shared and unique; once more with
    cov_event_cap below one sample's events: the compaction runs and nothing changes"""
    dev = small_device()
    s0, s2 = study()
    dev.set_option("cov_event_cap", cap)
    dev.cov_begin(LENGTHS, pad)
    try:
        dev.cov_add(0, lines_of(*s0))
        info = dev.cov_info()
        # the shared column of sample 0: the 70 000-base reference's segment spans several blocks of the statistics kernel, and a block
        # boundary falls inside the 2-base reference's segment
        ev = [2 * sum(1 for s, e in zip(s0[1][s0[0] == h], s0[2][s0[0] == h]) if (lambda r: r[0] < r[1])(covlib.interval(int(s), int(e), LENGTHS[h], pad))) for h in range(5)]
        assert ev[0] < info["events_per_block"] < ev[0] + ev[1] and ev[4] > 4 * info["events_per_block"]
        dev.cov_add(1, lines_of(*(x[:0] for x in s0)))
        dev.cov_add(2, lines_of(*s2))
        got = [dev.cov_stats(None), dev.cov_stats(0), dev.cov_stats(1), dev.cov_stats(2)]
        never = dev.cov_stats(7)
        info = dev.cov_info()
    finally:
        dev.cov_end()
        dev.set_option("cov_event_cap", 0)
    for (gs, gu), (es, eu) in zip(got, expected(pad)):
        assert np.array_equal(gs, es) and np.array_equal(gu, eu)
    assert int(got[0][0][2][2]) >= 3000 * 3000 * 27 and not never[0].any() and not never[1].any()
    if cap:
        raw0 = 16 * sum(ev)      # (the shared events of sample 0 alone, 16 bytes each)
        assert info["cap_bytes"] == cap < raw0 and info["compactions"] > 0 and info["peak_bytes"] <= cap
    else:
        assert info["compactions"] == 0 and info["events"] > 40000


def test_event_buffer_that_cannot_be_compacted_is_a_device_error():
    """the compacted sets do not fit either: BHIP_E_DEVICE with a message that says so (distinct positions, 16 bytes an event, cap 4 KB)"""
    from burst_amd import capi
    dev = small_device()
    dev.set_option("cov_event_cap", 4096)
    dev.cov_begin([70000], 0)
    try:
        st = 1 + 10 * np.arange(2000)
        with pytest.raises(capi.BurstHipError) as e:
            dev.cov_add(0, lines_of(np.zeros(2000, np.int64), st, st + 5, np.ones(2000), np.ones(2000)))
        assert e.value.code == capi.BHIP_E_DEVICE and "cov_event_cap" in str(e.value)
    finally:
        dev.cov_end()
        dev.set_option("cov_event_cap", 0)


def test_coordinates_up_to_2_32():
    """6: one reference of length 2^32 - 1; two overlapping lines that end at its last base, a reverse line of weight 3 at its start; the
    expected integers by hand.  pad 10: A = [L - 111, L), B = [L - 61, L), C = [0, 29) x 3; pad 0: A = [L - 101, L - 1), B = [L - 51, L - 1),
    C = [4, 19) x 3.  A and C are unique."""
    dev = small_device()
    L = 2 ** 32 - 1
    ln = lines_of([0, 0, 0], [L - 100, L - 50, 20], [L, L, 5], [1, 1, 3], [1, 0, 1])
    for pad, sh, un in ((10, (50 + 2 * 61 + 3 * 29, 111 + 29, 50 + 4 * 61 + 9 * 29, 5), (111 + 3 * 29, 111 + 29, 111 + 9 * 29, 4)),
                        (0, (50 + 2 * 50 + 3 * 15, 100 + 15, 50 + 4 * 50 + 9 * 15, 5), (100 + 3 * 15, 100 + 15, 100 + 9 * 15, 4))):
        dev.cov_begin([L], pad)
        try:
            dev.cov_add(0, ln)
            for gs, gu in (dev.cov_stats(0), dev.cov_stats(None)):
                assert tuple(int(x) for x in gs[0]) == sh and tuple(int(x) for x in gu[0]) == un
        finally:
            dev.cov_end()


def test_lane_extents():
    """7: bhip_lane_extents on quick.edx and dna.edx = the lane lengths numpy finds in the file's clump area; the default lengths the
    host derives from them = max(refStart + lane length) over every header's fragments; and on a hand-packed database of known lengths"""
    from burst_amd import host
    dev = small_device()
    want = np.zeros(16 * dev.n_clumps, np.uint32)
    want[:len(_dev["seqs"])] = [len(s) for s in _dev["seqs"]]
    assert np.array_equal(dev.lane_extents(), want)
    for name in ("quick.edx", "dna.edx"):
        db = host.Db.read(os.path.join(gl.G, name))
        d = db.open_device(0)
        try:
            ext = d.lane_extents()
        finally:
            d.close()
        assert np.array_equal(ext, lane_lengths(db)) and ext.max() > 32
        got = np.zeros(db.c.numRefHeads, np.uint32)
        assert host.lib().bh_cov_lengths_from_extents(C.byref(db.c), ext.ctypes.data, got.ctypes.data) == 0
        assert np.array_equal(got, default_lengths(db, lane_lengths(db)))
        db.close()


def run_cli(args):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    return r.returncode, r.stdout


def read_tables(prefix):
    return {k: open(prefix + k, "rb").read() for k in covlib.KINDS}


def test_command_line_against_bcov(tmp_path):
    """8: the dna_q100_best golden case's own flags with -ad and --coverage: the .b6 is the golden's; shared.txt and shared_binary.txt are
    bcov's tables byte for byte in their Dataset column, and the one sample's column (which bcov does not print without SPLIT) repeats
    it; the unique tables equal the shared ones (one line per read in BEST)"""
    c = [x for x in gl.cases() if x["name"] == "dna_q100_best"][0]
    out, p = str(tmp_path / "best.b6"), str(tmp_path / "P")
    code, text = run_cli(["-r", EDX, "-ad", "-q", Q100, "-o", out, "-m", c["mode"], "-i", c["id"]] + gl.cli_extra(c) + ["--coverage", p, "--coverage-lengths", LEN])
    assert code == 0 and "Coverage tables written" in text, text[-2000:]
    assert sorted(open(out, "rb").read().splitlines()) == gl.golden_lines(c)
    t = read_tables(p)
    for kind in ("shared", "shared_binary"):
        rows = [ln.split(b"\t") for ln in t[kind + ".txt"].splitlines()]
        assert rows[0] == [b"#Coverage", b"Dataset", b"best"] and all(len(r) == 3 and r[1] == r[2] for r in rows[1:])
        assert b"".join(b"\t".join(r[:2]) + b"\n" for r in rows) == open(os.path.join(COV, "dna_q100_best_%s.txt" % kind), "rb").read()
    assert t["unique.txt"] == t["shared.txt"] and t["unique_binary.txt"] == t["shared_binary.txt"]
    counts = [ln.split(b"\t") for ln in t["counts.txt"].splitlines()[1:]]
    assert sum(int(r[1]) for r in counts) == c["lines"] and len(counts) == 64
    assert sorted(os.listdir(str(tmp_path))) == sorted(["best.b6"] + ["P" + k for k in covlib.KINDS])


def study_run(tmp_path, tag, mode, files, coverage=True):
    d = tmp_path / tag
    d.mkdir()
    outs = [str(d / ("o%d.b6" % i)) for i in range(len(files))]
    lst = str(d / "list.txt")
    open(lst, "w").write("".join("%s\t%s\n" % p for p in zip(files, outs)))
    code, text = run_cli(["-r", EDX, "-ad", "--samples", lst, "-m", mode, "-i", "0.95", "-fr"] + (["--coverage", str(d / "C_"), "--coverage-lengths", LEN] if coverage else []))
    return code, text, outs, str(d / "C_")


@pytest.mark.parametrize("mode", ["ALLPATHS", "CAPITALIST"])
def test_study_of_three_samples(mode, tmp_path):
    """9: --samples over (q100, q292, q100) with -fr: all five tables equal the numpy restatement of the definitions computed from the three
    .b6 files this run wrote; four columns, the first and third samples' identical; Dataset cov <= the sum of the samples' with strict
    inequality somewhere; the .b6 files are those of a run without --coverage"""
    code, text, outs, prefix = study_run(tmp_path, "cov", mode, [Q100, Q292, Q100])
    assert code == 0, text[-2000:]
    lens = covlib.read_lengths(LEN)
    headers = sorted(lens, key=lambda h: h.encode())
    lengths = [lens[h] for h in headers]
    sh, un = covlib.b6_columns(outs, headers, lengths)
    want = covlib.tables(headers, lengths, ["o0", "o1", "o2"], sh, un)
    got = read_tables(prefix)
    assert got == want
    for k in covlib.KINDS:
        rows = [ln.split(b"\t") for ln in got[k].splitlines()]
        assert rows[0][1:] == [b"Dataset", b"o0", b"o1", b"o2"]
        assert len(rows) > 60 and all(len(r) == 5 for r in rows) and all(r[2] == r[4] for r in rows[1:])
    assert (sh[0, :, 1] <= sh[1:, :, 1].sum(0)).all() and (sh[0, :, 1] < sh[1:, :, 1].sum(0)).any()
    if mode == "ALLPATHS":
        assert got["unique.txt"] != got["shared.txt"] and (un[0, :, 3] < sh[0, :, 3]).any()
    code2, text2, outs2, _ = study_run(tmp_path, "plain", mode, [Q100, Q292, Q100], coverage=False)
    assert code2 == 0 and [open(o, "rb").read() for o in outs] == [open(o, "rb").read() for o in outs2]


def test_session_returns_the_same_integers(tmp_path):
    """9: host.Session(coverage=...) over the same list, without a lengths table: the default lengths are the database's own extents, the
    integers are the restatement's from the .b6 files the session wrote, and closing it writes the tables"""
    from burst_amd import host
    db = host.Db.read(EDX)
    heads = db_headers(db)
    lengths = default_lengths(db, lane_lengths(db))
    dev = db.open_device(0, build_K=12)
    outs = [str(tmp_path / ("s%d.b6" % i)) for i in range(3)]
    prefix = str(tmp_path / "S_")
    try:
        with host.Session(db, dev, mode="ALLPATHS", thres=0.95, rc=True, accel=True, K=12, coverage=prefix) as s:
            for q, o in zip((Q100, Q292, Q100), outs):
                assert s.run(q, o)["rc"] == 0
            gs, gu = s.coverage()
            assert np.array_equal(s.coverage_lengths(), lengths)
    finally:
        dev.close()
    sh, un = covlib.b6_columns(outs, heads, lengths)
    assert np.array_equal(gs, sh) and np.array_equal(gu, un) and gs.shape == (4, len(heads), 4)
    assert read_tables(prefix) == covlib.tables(heads, lengths, ["s0", "s1", "s2"], sh, un)
    db.close()


def test_unreadable_sample_is_a_zero_column(tmp_path):
    """9: a list whose second sample cannot be read: its column is all zero and named on standard output, the exit code is the sample's
    as without --coverage, and the tables are those of the two samples that were written"""
    missing = str(tmp_path / "missing.fa")
    code, text, outs, prefix = study_run(tmp_path, "bad", "BEST", [Q100, missing, Q100])
    assert code == 2 and "its column is all zero" in text and not os.path.exists(outs[1]), text[-2000:]
    lens = covlib.read_lengths(LEN)
    headers = sorted(lens, key=lambda h: h.encode())
    lengths = [lens[h] for h in headers]
    sh, un = covlib.b6_columns(outs, headers, lengths)
    assert not sh[2].any() and sh[1].any() and read_tables(prefix) == covlib.tables(headers, lengths, ["o0", "o1", "o2"], sh, un)
