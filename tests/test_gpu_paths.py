"""bhip_trace_paths against the full-matrix restatement of the canonical alignment path (tests/cigar_restate.c): the ops, the leftmost
column and the I count of every request, byte for byte.  The expected paths are computed once, on the CPU (cigarlib.build_pool), for
query lengths 2 .. 1 100 and edit distances 0 .. 30 either side of the band classes (one decision word per row up to ed = 7, bands of
more than 64 rows in the scratch from ed = 32), reads from both ends of a lane, the row-1 case, leading insertions, repeats where the
tie-breaks decide, IUPAC symbols under both tables, both strands."""
import ctypes as C

import numpy as np
import pytest

import cigarlib as cg
import dbutil
import oraclelib as ol

pytestmark = pytest.mark.gpu


class Pool:
    def __init__(self, L, z, iupac_only=False):
        from burst_amd import capi
        self.lut = ol.score_lut(z)
        self.seqs, queries, rcs, self.cases = cg.build_pool(L, self.lut, iupac_only=iupac_only)
        self.packed, self.clump_len, self.tot = dbutil.pack_clumps(self.seqs)
        self.q = capi.Queries(queries, [254] * len(queries), list(range(len(queries))), rcs)
        self.dev = capi.Device(self.packed, self.clump_len, self.tot, self.lut, device=0)

    def requests(self, idx):
        from burst_amd import capi
        r = np.zeros(len(idx), capi.PATH_REQ_DTYPE)
        for k, i in enumerate(idx):
            c = self.cases[i]
            r[k] = (c["q"], c["refIx"], c["finalPos"], c["ed"])
        return r

    def check(self, idx, got):
        ops, off, first, gap_r = got
        assert len(off) == len(idx) + 1 and off[0] == 0
        for k, i in enumerate(idx):
            c = self.cases[i]
            mine = ops[int(off[k]):int(off[k + 1])]
            assert mine.tobytes() == c["ops"].tobytes(), (c["kind"], c["m"], c["ed"], cg.text_of(mine), cg.text_of(c["ops"]))
            assert (int(first[k]), int(gap_r[k])) == (c["ref_first"], c["n_I"]), (c["kind"], c["m"], c["ed"])
        assert int(off[len(idx)]) == sum(len(self.cases[i]["ops"]) for i in idx)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


@pytest.fixture(scope="module")
def pool(L):
    p = Pool(L, 1)
    yield p
    p.dev.close()


def test_every_case_alone_and_together(pool):
    """the whole pool in one call (several requests per lane, all classes in one call), then each kind on its own"""
    idx = list(range(len(pool.cases)))
    before = pool.dev.paths_info()
    room = lambda sub: sum(2 * pool.cases[i]["ed"] + 1 for i in sub)      # (no capacity retry: the totals below count calls)
    pool.check(idx, pool.dev.trace_paths(pool.q, pool.requests(idx), cap=room(idx)))
    kinds = sorted(set(c["kind"] for c in pool.cases))
    assert {"row1", "leading_I", "begins_at_column_1", "end_exact", "first_columns", "last_columns", "repeat", "iupac", "m2_e0", "m1100_e30"} <= set(kinds)
    for kd in kinds:
        sub = [i for i in idx if pool.cases[i]["kind"] == kd]
        pool.check(sub, pool.dev.trace_paths(pool.q, pool.requests(sub), cap=room(sub)))
    info = pool.dev.paths_info()
    assert info["requests"] - before["requests"] == 2 * len(idx) and info["ops"] - before["ops"] == 2 * sum(len(c["ops"]) for c in pool.cases)
    assert info["us_total"] - before["us_total"] >= info["us_last"] > 0


def test_the_cases_are_what_they_are_named(pool):
    """the pool holds the situations it is meant to hold (decided on the CPU, no device involved)"""
    by = lambda kd: [c for c in pool.cases if c["kind"] == kd]
    assert all(cg.text_of(c["ops"]).startswith("1=1D") for c in by("row1")) and len(by("row1")) >= 10
    assert sum(cg.text_of(c["ops"]).startswith("1I") and c["ref_first"] == 1 for c in by("leading_I")) >= 3
    at_1 = [c for c in by("begins_at_column_1") if c["refIx"] != 3]      # (in the tandem repeat of lane 3 an exact read ends in the LAST of its many columns)
    assert len(at_1) >= 5 and all(c["ref_first"] == 1 and c["ed"] == 0 and c["finalPos"] == c["m"] for c in at_1)
    assert any(c["finalPos"] == int(pool.clump_len[c["refIx"] >> 4]) for c in by("end_exact"))             # an end at ClumpLen
    assert any(c["finalPos"] < int(pool.clump_len[c["refIx"] >> 4]) and c["finalPos"] == len(pool.seqs[c["refIx"]]) for c in by("end_exact"))   # trailing pads behind it
    eds = set(c["ed"] for c in pool.cases)
    assert {0, 1, 7, 8, 15, 16, 30} <= eds and {2, 31, 32, 33, 64, 65, 100, 292, 1100} <= set(c["m"] for c in pool.cases)
    assert sum(pool.q.rc[c["q"]] for c in pool.cases) > 30 and sum(1 - pool.q.rc[c["q"]] for c in pool.cases) > 30                # both strands


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_request_counts(pool, n):
    rng = np.random.default_rng(n)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=n)]
    pool.check(idx, pool.dev.trace_paths(pool.q, pool.requests(idx)))


def test_multi_column_share_and_gap_r(pool):
    """Requests whose last row attains the best (score, H) in more than one column: there the path's I count (V of the FINAL cell) may
    differ from the record's gapR (V of the FIRST such column).  The repeat cases must hold such requests, and some that do differ."""
    rep = [i for i, c in enumerate(pool.cases) if c["kind"] == "repeat"]
    multi = [i for i in rep if pool.cases[i]["n_best_cols"] > 1]
    differ = [i for i in multi if pool.cases[i]["n_I"] != pool.cases[i]["gapR"]]
    share = len(multi) / len(rep)
    print("repeat cases: %d, more than one best end column: %d (%.0f %%), I != record gapR: %d" % (len(rep), len(multi), 100 * share, len(differ)))
    assert share > 0.25 and len(differ) >= 3
    _, _, _, gap_r = pool.dev.trace_paths(pool.q, pool.requests(rep))
    for k, i in enumerate(rep):
        c = pool.cases[i]
        assert int(gap_r[k]) == c["n_I"]
        if c["n_best_cols"] == 1:
            assert int(gap_r[k]) == c["gapR"]      # one best end column: the path's I count IS the record's gapR
    assert any(int(gap_r[k]) != pool.cases[i]["gapR"] for k, i in enumerate(rep))


def test_capacity_then_success(pool):
    from burst_amd import capi
    idx = list(range(0, len(pool.cases), 3))
    req = pool.requests(idx)
    need = sum(len(pool.cases[i]["ops"]) for i in idx)
    off = np.zeros(len(idx) + 1, np.uint64)
    first, gap_r = np.zeros(len(idx), np.uint32), np.zeros(len(idx), np.uint32)
    small = np.zeros(need - 1, np.uint32)
    call = lambda ops: capi.lib().bhip_trace_paths(pool.dev._h, capi._ptr(pool.q.codes), capi._ptr(pool.q.off), pool.q.n, capi._ptr(req), len(req),
                                                    capi._ptr(ops), len(ops), capi._ptr(off), capi._ptr(first), capi._ptr(gap_r))
    assert call(small) == capi.BHIP_E_CAPACITY and int(off[len(idx)]) == need
    ops = np.zeros(need, np.uint32)
    assert call(ops) == capi.BHIP_OK
    pool.check(idx, (ops, off, first, gap_r))


def test_validation_comes_first_and_leaves_the_handle_usable(pool):
    from burst_amd import capi
    good = pool.requests([0, 5, 9])
    n_clumps = len(pool.clump_len)
    bad_rows = [
        (pool.q.n, 0, 10, 0),                                   # query out of range
        (0, pool.tot, 10, 0),                                   # a dead lane of the last clump
        (0, 16 * n_clumps, 10, 0),                              # beyond the clumps
        (0, 0, 0, 0),                                           # end column 0
        (0, 16, int(pool.clump_len[1]) + 1, 0),                 # end column beyond the clump
        (0, 0, 10, 255),                                        # beyond the 8-bit recurrence
    ]
    for row in bad_rows:
        req = np.concatenate([good, np.array([row], capi.PATH_REQ_DTYPE)])
        with pytest.raises(capi.BurstHipError) as e:
            pool.dev.trace_paths(pool.q, req)
        assert e.value.code == capi.BHIP_E_ARG, row
        assert "request 3" in str(e.value)
    pool.check([0, 5, 9], pool.dev.trace_paths(pool.q, good))


def test_an_edit_distance_one_too_low_is_named(pool):
    from burst_amd import capi
    idx = [i for i, c in enumerate(pool.cases) if c["ed"] >= 1][:40]
    req = pool.requests(idx)
    req["ed"][17] -= 1
    req["ed"][30] -= 1
    with pytest.raises(capi.BurstHipError) as e:
        pool.dev.trace_paths(pool.q, req)
    assert e.value.code == capi.BHIP_E_RESCORE and "request 17 " in str(e.value)
    pool.check(idx, pool.dev.trace_paths(pool.q, pool.requests(idx)))


@pytest.mark.parametrize("z", [0, 1])
def test_iupac_under_both_tables(L, z):
    """ambiguity codes in the query and in the reference, with N free (-y) and penalised (-n)"""
    p = Pool(L, z, iupac_only=True)
    try:
        assert len(p.cases) >= 30 and any("X" in cg.text_of(c["ops"]) for c in p.cases)
        idx = list(range(len(p.cases)))
        p.check(idx, p.dev.trace_paths(p.q, p.requests(idx)))
    finally:
        p.dev.close()


def test_a_wide_band_goes_through_the_scratch(L):
    """ed = 40: 81 diagonals, more band rows than the kernel keeps in LDS; m = 300 and 1 400 in one block"""
    from burst_amd import capi
    rng = np.random.default_rng(5)
    lane = cg.random_lane(rng, 1700)
    lut = ol.score_lut(1)
    qs, cases = [], []
    for m in (300, 1400, 130):
        st = int(rng.integers(0, 1700 - m - 50))
        q = cg.edit_read(rng, lane, st, m, 16, 12, 12)
        ok, _, o = cg.trace(L, q, lane, 40, lut)
        assert ok and o.ed >= 33
        ok, ops, e = cg.trace(L, q, lane, o.ed, lut, final_pos=o.finalPos)
        qs.append(q)
        cases.append((o, ops, e))
    packed, clump_len, tot = dbutil.pack_clumps([lane])
    dev = capi.Device(packed, clump_len, tot, lut, device=0)
    try:
        Q = capi.Queries(qs, [254] * 3)
        ops, off, first, gap_r = dev.trace_paths(Q, [(k, 0, c[0].finalPos, c[0].ed) for k, c in enumerate(cases)])
        for k, (o, exp, e) in enumerate(cases):
            assert ops[int(off[k]):int(off[k + 1])].tobytes() == exp.tobytes()
            assert (int(first[k]), int(gap_r[k])) == (e.ref_first, e.n_I)
    finally:
        dev.close()
