"""bhip_mates_join against the brute-force join of tests/mateslib.py on seeded random lines.  Values are drawn small so that collisions are
common (pair < 40, ref < 6, positions < 300, insert bounds that cut through the data): equal keys, equal edit sums, fragments at the
bounds, lines on one side only all occur in every array."""
import numpy as np
import pytest

import dbutil
import mateslib as ml
import oraclelib as ol

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 5000)


@pytest.fixture(scope="module")
def dev():
    from burst_amd import capi
    rng = np.random.default_rng(5)
    seqs = [rng.integers(1, 5, size=200, dtype=np.uint8) for _ in range(3)]
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    d = capi.Device(packed, clump_len, tot, ol.score_lut(1), device=0)
    yield d
    d.close()


def lines(rng, n, n_pairs=40, n_refs=6, pos=300, neg=False):
    from burst_amd import capi
    out = np.zeros(n, capi.MATE_LINE_DTYPE)
    out["pair"] = rng.integers(0, n_pairs, n)
    out["ref"] = rng.integers(0, n_refs, n)
    st = rng.integers(-40 if neg else 1, pos, n)
    span = rng.integers(0, 60, n)
    rev = rng.integers(0, 2, n).astype(bool)
    out["st"] = np.where(rev, st + span, st)
    out["ed"] = np.where(rev, st, st + span)
    out["edits"] = rng.integers(0, 4, n)
    return out


def rows(x):
    return [tuple(int(v) for v in r) for r in x.tolist()]


def check(dev, a, b, orientation, ins_min, ins_max, report, **kw):
    exp = ml.join(rows(a), rows(b), orientation, ins_min, ins_max, report)
    ga, gb = dev.mates_join(a, b, orientation, ins_min, ins_max, report, **kw)
    assert list(zip(ga.tolist(), gb.tolist())) == exp, (len(a), len(b), orientation, ins_min, ins_max, report)
    return exp


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(11)
    return lines(rng, 5000), lines(rng, 5000)


@pytest.mark.parametrize("report", ml.REPORTS)
@pytest.mark.parametrize("orientation", ml.ORIENTATIONS)
def test_line_counts(dev, big, orientation, report):
    """(na, nb) over SIZES x SIZES: prefixes of one pair of arrays, so that every size sees the same collisions"""
    a, b = big
    n_found = 0
    for na in SIZES:
        for nb in SIZES:
            n_found += len(check(dev, a[:na], b[:nb], orientation, 60, 180, report))
    assert n_found > (1000 if report == "all" else 200)      # (`best`: at most one per pair and call)


def test_the_data_is_not_vacuous(big):
    """decided on the CPU: the big arrays hold what the tests above are meant to meet"""
    a, b = rows(big[0]), rows(big[1])
    for o in ml.ORIENTATIONS:
        wide, cut = ml.join(a, b, o, 0, 1000, "all"), ml.join(a, b, o, 60, 180, "all")
        best = ml.join(a, b, o, 60, 180, "best")
        assert len(wide) > len(cut) > len(best) > 30      # (the bounds cut through the data; pairs have several combinations)
        frag = [ml.fragment(ml.Line(*a[i]), ml.Line(*b[j]), o)[1] for i, j in cut]
        assert 60 in frag and 180 in frag                  # a fragment exactly at each bound
        sums = {}
        for i, j in cut:
            sums.setdefault(a[i][0], []).append(a[i][4] + b[j][4])
        assert sum(1 for v in sums.values() if v.count(min(v)) > 1) > 10      # ties on the edit sum for `best` to break


@pytest.mark.parametrize("orientation", ml.ORIENTATIONS)
def test_bounds_and_negative_positions(dev, orientation):
    """ins_min == ins_max; each length next to a bound; st below zero (column 9 is printed with %d)"""
    rng = np.random.default_rng(3)
    a, b = lines(rng, 700, neg=True), lines(rng, 700, neg=True)
    assert (a["st"] < 0).sum() > 20 and (b["ed"] < 0).sum() > 5
    for lo, hi in ((100, 100), (99, 101), (0, 0), (1, 1), (0, 4000000000), (4000000000, 4000000000)):
        for report in ml.REPORTS:
            check(dev, a, b, orientation, lo, hi, report)
    assert len(ml.join(rows(a), rows(b), orientation, 100, 100, "all")) > 0
    # hand-made: the same fragment of length 150 at, inside and outside each bound; a line with st == ed is forward
    A = np.zeros(3, a.dtype); B = np.zeros(3, a.dtype)
    A[0] = (0, 0, -20, 29, 1); B[0] = (0, 0, 129, 80, 0)        # fr: forward [-20, 29], reverse [80, 129]: length 150, leftmost -20
    A[1] = (1, 0, 7, 7, 0); B[1] = (1, 0, 9, 8, 0)              # st == ed: forward
    A[2] = (2, 0, 50, 10, 0); B[2] = (2, 0, 30, 60, 0)          # rf: reverse [10, 50], forward [30, 60]: length 51
    for lo, hi in ((150, 150), (149, 150), (150, 151), (151, 200), (0, 149), (3, 3), (51, 51), (0, 1000)):
        check(dev, A, B, orientation, lo, hi, "all")
    if orientation == "fr":
        assert ml.join(rows(A), rows(B), "fr", 150, 150, "all") == [(0, 0)] and ml.join(rows(A), rows(B), "fr", 3, 3, "all") == [(1, 1)]
    if orientation == "rf":
        assert ml.join(rows(A), rows(B), "rf", 51, 51, "all") == [(2, 2)]


@pytest.mark.parametrize("report", ml.REPORTS)
def test_long_run(dev, report):
    """one key whose run holds 3 000 lines of b (it crosses the blocks of every kernel), between ordinary keys"""
    rng = np.random.default_rng(7)
    a, b = lines(rng, 600), lines(rng, 4000)
    b["pair"][500:3500] = 17
    b["ref"][500:3500] = 2
    a["pair"][::7] = 17
    a["ref"][::7] = 2
    for orientation in ml.ORIENTATIONS:
        exp = check(dev, a, b, orientation, 50, 250, report)
        if report == "all":
            assert max(np.bincount([i for i, _ in exp])) > 300


def test_pairs_on_one_side_only(dev):
    rng = np.random.default_rng(9)
    a, b = lines(rng, 300), lines(rng, 300)
    a["pair"] = a["pair"] * 2                      # even pairs 0 .. 78
    b["pair"] = b["pair"] * 3                      # multiples of 3: the two meet in the multiples of 6 only
    for report in ml.REPORTS:
        exp = check(dev, a, b, "fr", 0, 1000, report)
        assert exp and all(int(a["pair"][i]) % 6 == 0 for i, _ in exp)
    b["pair"] += 200                               # nothing in common
    assert check(dev, a, b, "fr", 0, 1000, "all") == []
    assert check(dev, a, b, "fr", 0, 1000, "best") == []


def test_best_ties(dev):
    """equal edit sums: the smallest a wins, then the smallest b; a later a with a smaller sum beats both"""
    from burst_amd import capi
    F, R = (10, 60), (160, 111)      # a forward and a reverse placement: fragment 151
    mk = lambda rws: np.array([tuple(r) for r in rws], capi.MATE_LINE_DTYPE)
    a = mk([(0, 1, *F, 2), (0, 1, *F, 1), (0, 2, *F, 1), (1, 1, *F, 3), (1, 1, *F, 0), (2, 1, *F, 0)])
    b = mk([(0, 2, *R, 1), (0, 1, *R, 1), (0, 1, *R, 0), (0, 1, *R, 1), (1, 1, *R, 5), (1, 1, *R, 2), (2, 1, *F, 0)])
    exp = check(dev, a, b, "fr", 0, 1000, "best")
    # pair 0: sums (a0: 3, 2, 3), (a1: 2, 1, 2), (a2 on ref 2: 2) -> a1 with b2; pair 1: a3: 8, 5; a4: 5, 2 -> a4 with b5; pair 2: not concordant
    assert exp == [(1, 2), (4, 5)]
    a["edits"][1] = 2                # now a0 + b2 = 2 = a1 + b1 = a1 + b3 = a2 + b0 ... the smallest a, then its smallest b
    assert check(dev, a, b, "fr", 0, 1000, "best") == [(0, 2), (4, 5)]
    b["edits"][2] = 1                # a0: 3, 3, 3; a1: 3, 3, 3; a2 + b0 = 2
    assert check(dev, a, b, "fr", 0, 1000, "best") == [(2, 0), (4, 5)]
    b["edits"][0] = 2                # everything 3: a0 with b1
    assert check(dev, a, b, "fr", 0, 1000, "best") == [(0, 1), (4, 5)]


def test_capacity_then_success_and_counters(dev, big):
    from burst_amd import capi
    a, b = big[0][:2000], big[1][:2000]
    exp = ml.join(rows(a), rows(b), "fr", 0, 1000, "all")
    assert len(exp) > 100
    L = capi.lib()
    n = capi.C.c_uint64(0)
    oa, ob = np.full(len(exp), 0xFFFFFFFF, np.uint32), np.full(len(exp), 0xFFFFFFFF, np.uint32)
    before = dev.mates_info()
    rc = L.bhip_mates_join(dev._h, capi._ptr(a), len(a), capi._ptr(b), len(b), 0, 0, 1000, 0, capi._ptr(oa), capi._ptr(ob), len(exp) - 1, capi.C.byref(n))
    assert rc == capi.BHIP_E_CAPACITY and n.value == len(exp) and np.all(oa == 0xFFFFFFFF) and np.all(ob == 0xFFFFFFFF)
    mid = dev.mates_info()
    assert (mid["lines"], mid["combinations"]) == (before["lines"], before["combinations"]) and mid["us_last"] > 0
    rc = L.bhip_mates_join(dev._h, capi._ptr(a), len(a), capi._ptr(b), len(b), 0, 0, 1000, 0, capi._ptr(oa), capi._ptr(ob), len(exp), capi.C.byref(n))
    assert rc == capi.BHIP_OK and n.value == len(exp) and list(zip(oa.tolist(), ob.tolist())) == exp
    after = dev.mates_info()
    assert after["lines"] - before["lines"] == 4000 and after["combinations"] - before["combinations"] == len(exp)
    assert after["us_total"] - mid["us_total"] == after["us_last"] > 0
    # the wrapper retries once with the wanted room
    ga, gb = dev.mates_join(a, b, "fr", 0, 1000, "all", cap=3)
    assert list(zip(ga.tolist(), gb.tolist())) == exp
    # an empty side: no launch, the counters stay
    ga, gb = dev.mates_join(a, b[:0])
    assert len(ga) == 0 and len(gb) == 0 and dev.mates_info()["lines"] == after["lines"] + 4000


def test_bad_arguments_leave_the_handle_usable(dev, big):
    from burst_amd import capi
    a, b = big[0][:300], big[1][:300]
    L = capi.lib()
    n = capi.C.c_uint64(7)
    oa, ob = np.zeros(4096, np.uint32), np.zeros(4096, np.uint32)
    call = lambda na, nb, o, lo, hi, rep: L.bhip_mates_join(dev._h, capi._ptr(a), na, capi._ptr(b), nb, o, lo, hi, rep, capi._ptr(oa), capi._ptr(ob), 4096, capi.C.byref(n))
    for args in ((300, 300, 3, 0, 1000, 0), (300, 300, 0, 0, 1000, 2), (300, 300, 0, 11, 10, 0), (1 << 32, 300, 0, 0, 1000, 0), (300, 1 << 32, 0, 0, 1000, 0)):
        assert call(*args) == capi.BHIP_E_ARG, args
        assert b"bhip_mates_join" in L.bhip_last_error()
        check(dev, a, b, "fr", 0, 1000, "all")
    sparse = a.copy()
    sparse["pair"][5] = 0xFFFFFFF0      # `best` keeps a table indexed by pair: numbers that are not dense are refused, `all` takes them
    assert L.bhip_mates_join(dev._h, capi._ptr(sparse), 300, capi._ptr(b), 300, 0, 0, 1000, 1, capi._ptr(oa), capi._ptr(ob), 4096, capi.C.byref(n)) == capi.BHIP_E_ARG
    check(dev, sparse, b, "fr", 0, 1000, "all")
    check(dev, a, b, "fr", 0, 1000, "best")
    with pytest.raises(capi.BurstHipError):
        dev.mates_join(a, b, "fr", 5, 4)
