"""bhip_pile_run against pilelib, the dictionary count of the definition: the sites it returns, site for site and byte for byte, on
cigarlib's pool of lanes and paths (21 lanes in two clumps, reads of 2 .. 1 100 symbols, 0 .. 30 edits) with two lanes of one clump on one
header at offsets that overlap and mixed weights; then the thresholds on a planted pile-up, the boundaries of the stabbing count, the
insertion marks, ambiguous codes on both sides, capacity, arguments and the call's figures."""
import ctypes as C

import numpy as np
import pytest

import cigarlib as cg
import pilecases
import pilelib

pytestmark = pytest.mark.gpu


def site_bytes(rows):
    from burst_amd import capi
    a = np.zeros(len(rows), capi.PILE_SITE_DTYPE)
    for k, r in enumerate(rows):
        a[k] = (r[0], r[1], r[2], r[3], r[4:10], r[10])
    return a.tobytes()


class Pool(pilecases.PileCases):
    def __init__(self, L, z=1, iupac_only=False):
        from burst_amd import capi
        super().__init__(L, z, iupac_only)
        self.q = capi.Queries(self.queries, [254] * len(self.queries), list(range(len(self.queries))), self.rcs)
        self.dev = capi.Device(self.packed, self.clump_len, self.tot, self.lut, device=0)

    def check(self, idx, min_depth=1, min_alt=1, weights=None):
        """the device's sites of the cases idx = the model's, byte for byte; returns (rows, all sites of the model)"""
        lines, ops = self.arrays(idx, weights)
        got = self.dev.pile_run(self.q, lines, ops, min_depth, min_alt)
        sites = pilelib.pile(self.model_lines(idx, weights))
        exp = pilelib.reported(sites, min_depth, min_alt)
        assert pilecases.rows_of(got) == exp
        assert got.tobytes() == site_bytes(exp)
        info = self.dev.pile_info()
        assert (info["events"], info["candidates"], info["sites"]) == pilelib.figures(sites) + (len(exp),)
        return exp, sites


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


@pytest.fixture(scope="module")
def pool(L):
    p = Pool(L, 1)
    yield p
    p.dev.close()


def test_whole_pool_then_every_kind(pool):
    """the whole pool in one call at min_depth = min_alt = 1, then every kind alone; two lanes share a header where lines of both observe"""
    assert pool.shared is not None and pool.shared[3] >= 1, "no two lanes of the second clump agree where their lines overlap"
    A, B = pool.shared[0], pool.shared[1]
    assert A >> 4 == B >> 4 and pool.header[A] == pool.header[B]
    idx = list(range(len(pool.cases)))
    rows, sites = pool.check(idx)
    assert len(rows) > 500 and any(r[10] for r in rows) and any(r[8] for r in rows) and any(r[9] for r in rows)      # Ins, Del, Other all occur
    # a position of the shared header that lines of both lanes observe is among the candidates' neighbours: the depth there counts both lanes
    both = {}
    for i in idx:
        c = pool.cases[i]
        if c["refIx"] in (A, B):
            first = pool.off[c["refIx"]] + c["ref_first"]
            for p in range(first, first + pilecases.span_of(c["ops"])):
                both.setdefault(p, set()).add(c["refIx"])
    assert sum(1 for s in both.values() if len(s) == 2) == pool.shared[3]
    kinds = sorted(set(c["kind"] for c in pool.cases))
    assert {"row1", "leading_I", "repeat", "iupac", "m2_e0", "m1100_e30"} <= set(kinds)
    for kd in kinds:
        pool.check([i for i in idx if pool.cases[i]["kind"] == kd])
    assert pool.dev.pile_info()["device_us"] > 0 and pool.dev.pile_info()["peak_bytes"] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_line_counts(pool, n):
    rng = np.random.default_rng(n)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=n)]
    pool.check(idx, min_depth=1 if n < 5000 else 3, min_alt=1 if n < 5000 else 2)


def test_a_permutation_of_the_lines_gives_identical_bytes(pool):
    rng = np.random.default_rng(3)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=700)]
    lines, ops = pool.arrays(idx)
    a = pool.dev.pile_run(pool.q, lines, ops, 2, 1)
    b = pool.dev.pile_run(pool.q, lines[rng.permutation(len(lines))], ops, 2, 1)
    assert len(a) > 50 and a.tobytes() == b.tobytes()


# ---- hand-made lines on the pool's lanes (pilecases.Hand and the scenarios the CPU tests share) ----------------------------------------
def run_hand(pool, h, min_depth=1, min_alt=1):
    from burst_amd import capi
    q = capi.Queries(h.queries, [254] * len(h.queries))
    got = pool.dev.pile_run(q, h.rows, h.ops, min_depth, min_alt)
    sites = pilelib.pile(h.model)
    exp = pilelib.reported(sites, min_depth, min_alt)
    assert got.tobytes() == site_bytes(exp), (pilecases.rows_of(got), exp)
    info = pool.dev.pile_info()
    assert (info["events"], info["candidates"], info["sites"]) == pilelib.figures(sites) + (len(exp),)
    return exp


@pytest.mark.parametrize("min_depth,min_alt", [(4, 2), (10, 3)])
def test_planted_pile_up_either_side_of_both_thresholds(pool, min_depth, min_alt):
    """exact reads of 33 symbols share a window of lane 0; k of them carry one substitution in column 120"""
    for n_lines, k, want in pilecases.planted_cases(min_depth, min_alt):
        rows = run_hand(pool, pilecases.planted(pool, n_lines, k), min_depth, min_alt)
        pilecases.check_planted(rows, n_lines, k, want)


def test_boundaries_of_the_stabbing_count(pool):
    """one line is not plain at column p = 300; plain lines begin at p, end at p, end at p - 1 and begin at p + 1"""
    pilecases.check_boundaries(run_hand(pool, pilecases.boundaries(pool)))


def test_interior_and_end_insertions(pool):
    pilecases.check_insertions(run_hand(pool, pilecases.insertions(pool)))
    # the pool's own leading insertions
    idx = [i for i, c in enumerate(pool.cases) if c["kind"] == "leading_I"]
    assert sum(cg.text_of(pool.cases[i]["ops"]).startswith("1I") for i in idx) >= 3
    rows, _ = pool.check(idx, weights=[1] * len(idx))
    assert not pool.before_paths(idx) & {(r[0], r[1]) for r in rows}      # no mark on the position in front of a path


@pytest.mark.parametrize("z", [0, 1])
def test_ambiguous_codes_on_both_sides(L, z):
    """the iupac pool: an '=' over an ambiguous query code counts as Other; a site on an ambiguous reference code is never returned"""
    p = Pool(L, z, iupac_only=True)
    try:
        idx = list(range(len(p.cases)))
        assert len(idx) >= 30
        rows, sites = p.check(idx)
        eq_amb = 0
        for ln in p.model_lines(idx):
            j = 0
            for n, op in ln["ops"]:
                if op == "=":
                    eq_amb += sum(1 for t in range(n) if not 1 <= int(ln["query"][j + t]) <= 4)
                j += n if op != "D" else 0
        assert eq_amb > 0 and any(r[9] for r in rows)
        amb_ref = [k for k, s in sites.items() if not 1 <= s["ref"] <= 4 and s["events"]]
        assert amb_ref and not set(amb_ref) & {(r[0], r[1]) for r in rows} and all(1 <= r[2] <= 4 for r in rows)
    finally:
        p.dev.close()


def test_capacity_then_success(pool):
    from burst_amd import capi
    idx = list(range(0, len(pool.cases), 2))
    lines, ops = pool.arrays(idx)
    exp = pilelib.reported(pilelib.pile(pool.model_lines(idx)), 1, 1)
    n, info = C.c_uint64(0), np.zeros(8, np.uint64)
    small = np.frombuffer(bytes([0xAB]) * (44 * (len(exp) - 1)), np.uint8).copy()
    call = lambda buf, cap: capi.lib().bhip_pile_run(pool.dev._h, capi._ptr(pool.q.codes), capi._ptr(pool.q.off), pool.q.n, capi._ptr(lines), len(lines), capi._ptr(ops), len(ops),
                                                    1, 1, capi._ptr(buf), cap, C.byref(n), capi._ptr(info))
    assert call(small, len(exp) - 1) == capi.BHIP_E_CAPACITY and n.value == len(exp)
    assert set(small.tolist()) == {0xAB}      # nothing was written
    full = np.zeros(len(exp), capi.PILE_SITE_DTYPE)
    assert call(full, len(exp)) == capi.BHIP_OK and n.value == len(exp) and full.tobytes() == site_bytes(exp)


def test_no_lines_launch_nothing(pool):
    from burst_amd import capi
    before = pool.dev.pile_info()
    got = pool.dev.pile_run(pool.q, np.zeros(0, capi.PILE_LINE_DTYPE), np.zeros(0, np.uint32), 1, 1)
    info = pool.dev.pile_info()
    assert len(got) == 0 and info["device_us"] == 0 and info["events"] == 0 and before is not None


def test_every_bad_argument_is_named_and_leaves_the_handle_usable(pool):
    from burst_amd import capi
    good = [0, 5, 9]
    lines, ops = pool.arrays(good)
    n_clumps = len(pool.clump_len)
    cl0 = int(pool.clump_len[0])

    def bad(field=None, value=None, ops_edit=None, min_depth=1, min_alt=1, extra=None):
        ln, op = lines.copy(), ops.copy()
        if field:
            ln[field][2] = value
        if ops_edit:
            ops_edit(ln, op)
        if extra is not None:
            ln = np.concatenate([ln, extra])
        with pytest.raises(capi.BurstHipError) as e:
            pool.dev.pile_run(pool.q, ln, op, min_depth, min_alt)
        assert e.value.code == capi.BHIP_E_ARG, (field, value)
        return str(e.value)

    assert "line 2" in bad("q", pool.q.n)                                   # a query out of range
    assert "line 2" in bad("refIx", pool.tot)                               # a dead lane of the last clump
    assert "line 2" in bad("refIx", 16 * n_clumps)                          # beyond the clumps
    assert "line 2" in bad("op_off", len(ops))                              # an op range outside ops
    assert "line 2" in bad("n_ops", len(ops) + 1)
    k = next(j for j in range(int(lines["op_off"][2]), int(lines["op_off"][2]) + int(lines["n_ops"][2])) if int(ops[j]) & 15 == 7)      # an '=' run of line 2

    def set_op(word):
        def f(ln, op):
            op[k] = word
        return f
    assert "line 2" in bad(ops_edit=set_op(5 << 4 | 3))                     # not I / D / = / X
    assert "line 2" in bad(ops_edit=set_op(0 << 4 | 7))                     # length 0
    assert "line 2" in bad(ops_edit=set_op((int(ops[k]) >> 4) + 1 << 4 | int(ops[k]) & 15))      # ops that do not consume the query's length
    assert "line 2" in bad("ref_first", 0)                                  # columns that leave 1 .. ClumpLen
    assert "line 2" in bad("ref_first", cl0)
    assert "line 2" in bad("pos", 0)
    assert "line 2" in bad("pos", 0xFFFFFFFF)                               # pos + span beyond 2^32 - 1
    assert "line 2" in bad("w", 0)
    heavy = lines[:1].copy()
    heavy["w"] = 0x7FFFFFFF
    assert "2^31" in bad(extra=heavy)                                       # summed weights beyond 2^31 - 1
    bad(min_depth=0)
    bad(min_alt=0)
    exp = pilelib.reported(pilelib.pile(pool.model_lines(good)), 1, 1)
    assert pool.dev.pile_run(pool.q, lines, ops, 1, 1).tobytes() == site_bytes(exp)
