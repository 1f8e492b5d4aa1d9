"""bhip_consensus_run against conslib, the dictionary model of the definition: segments, letters and figures byte for byte, on cigarlib's
pool of lanes and paths (two lanes of one clump share a header where lines of both observe; mixed weights), line counts either side of a
wave and a block, a permutation of the lines, min_depth 1, 2 and 1000; the hand-made segment shapes and calling rules of conscases;
both capacities, every bad argument, no lines, the call's figures -- and bhip_pile_run on the same handle afterwards, which shares scratch
buffers and stages with it."""
import ctypes as C

import numpy as np
import pytest

import cigarlib as cg
import conscases
import conslib
import pilecases
import pilelib

pytestmark = pytest.mark.gpu


class Pool(pilecases.PileCases):
    def __init__(self, L, z=1, iupac_only=False):
        from burst_amd import capi
        super().__init__(L, z, iupac_only)
        self.q = capi.Queries(self.queries, [254] * len(self.queries), list(range(len(self.queries))), self.rcs)
        self.dev = capi.Device(self.packed, self.clump_len, self.tot, self.lut, device=0)

    def check(self, idx, min_depth=1, weights=None):
        """the device's segments and letters of the cases idx = the model's, byte for byte; returns the model's"""
        lines, ops = self.arrays(idx, weights)
        segs, letters = self.dev.consensus_run(self.q, lines, ops, min_depth)
        model = self.model_lines(idx, weights)
        sites = pilelib.pile(model)
        exp_segs, exp_letters = conslib.consensus(model, min_depth, sites)
        assert letters == exp_letters.encode()
        assert segs.tobytes() == conslib.seg_bytes(exp_segs)
        info = self.dev.consensus_info()
        assert (info["events"], info["candidates"], info["segments"], info["covered"]) == conslib.info(model, exp_segs, sites)
        return exp_segs, exp_letters


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


@pytest.fixture(scope="module")
def pool(L):
    p = Pool(L, 1)
    yield p
    p.dev.close()


def test_whole_pool_then_every_kind(pool):
    assert pool.shared is not None and pool.shared[3] >= 1, "no two lanes of the second clump agree where their lines overlap"
    idx = list(range(len(pool.cases)))
    segs, letters = pool.check(idx)
    assert len(segs) >= 10 and "-" in letters and sum(g["subst"] for g in segs) > 0 and sum(g["ins_major"] for g in segs) > 0
    for kd in sorted(set(c["kind"] for c in pool.cases)):
        pool.check([i for i in idx if pool.cases[i]["kind"] == kd])
    info = pool.dev.consensus_info()
    assert info["device_us"] > 0 and info["peak_bytes"] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_line_counts(pool, n):
    rng = np.random.default_rng(n)
    pool.check([int(i) for i in rng.integers(0, len(pool.cases), size=n)], min_depth=1 if n < 5000 else 3)


@pytest.mark.parametrize("min_depth", [1, 2, 1000])
def test_min_depth(pool, min_depth):
    segs, letters = pool.check(list(range(0, len(pool.cases), 3)), min_depth)
    if min_depth == 1000:
        assert set(letters) == {"N"} and not any(g["called"] for g in segs)
    else:
        assert any(g["called"] for g in segs)


def test_a_permutation_of_the_lines_gives_identical_bytes(pool):
    rng = np.random.default_rng(3)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=700)]
    lines, ops = pool.arrays(idx)
    a = pool.dev.consensus_run(pool.q, lines, ops, 2)
    b = pool.dev.consensus_run(pool.q, lines[rng.permutation(len(lines))], ops, 2)
    assert len(a[0]) > 5 and a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


def test_equal_weights_and_the_lanes_that_share_a_header(pool):
    A, B = pool.shared[0], pool.shared[1]
    idx = [i for i, c in enumerate(pool.cases) if c["refIx"] in (A, B)]
    segs, _ = pool.check(idx, 2, weights=[1] * len(idx))
    assert all(g["header"] == pool.header[A] for g in segs)
    pool.check(idx, 2)


def run_hand(pool, h, min_depth):
    from burst_amd import capi
    q = capi.Queries(h.queries, [254] * len(h.queries))
    segs, letters = pool.dev.consensus_run(q, h.rows, h.ops, min_depth)
    exp_segs, exp_letters = conslib.consensus(h.model, min_depth)
    assert letters == exp_letters.encode() and segs.tobytes() == conslib.seg_bytes(exp_segs), (segs, letters, exp_segs, exp_letters)
    info = pool.dev.consensus_info()
    assert (info["events"], info["candidates"], info["segments"], info["covered"]) == conslib.info(h.model, exp_segs)
    return exp_segs, exp_letters


@pytest.mark.parametrize("shape", conscases.SHAPES, ids=lambda f: f.__name__)
def test_segment_shapes(pool, shape):
    h, check = shape(pool)
    for m in (1, 2):
        segs, letters = run_hand(pool, h, m)
        assert check(segs, letters)


@pytest.mark.parametrize("rule", conscases.RULES, ids=lambda f: f.__name__)
def test_calling_rules(pool, rule):
    h, check = rule(pool)
    segs, letters = run_hand(pool, h, conscases.MIN_DEPTH)
    assert check(segs, letters)


@pytest.mark.parametrize("z", [0, 1])
def test_an_ambiguous_reference_column_keeps_its_letter(L, z):
    p = Pool(L, z, iupac_only=True)
    try:
        segs, letters = p.check(list(range(len(p.cases))))
        assert sum(g["ambig"] for g in segs) > 0 and set(letters) - set("ACGTN-"), "no ambiguity code among the letters"
    finally:
        p.dev.close()


def test_both_capacities_then_success(pool):
    from burst_amd import capi
    idx = list(range(0, len(pool.cases), 2))
    lines, ops = pool.arrays(idx)
    exp_segs, exp_letters = conslib.consensus(pool.model_lines(idx), 1)
    ns, nl, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)

    def call(seg_cap, letter_cap):
        segs, letters = np.full(max(seg_cap, 1) * 48, 0xAB, np.uint8), np.full(max(letter_cap, 1), 0xAB, np.uint8)
        rc = capi.lib().bhip_consensus_run(pool.dev._h, capi._ptr(pool.q.codes), capi._ptr(pool.q.off), pool.q.n, capi._ptr(lines), len(lines), capi._ptr(ops), len(ops), 1,
                                           capi._ptr(segs), seg_cap, C.byref(ns), capi._ptr(letters), letter_cap, C.byref(nl), capi._ptr(info))
        return rc, segs, letters
    for seg_cap, letter_cap in ((len(exp_segs) - 1, len(exp_letters)), (len(exp_segs), len(exp_letters) - 1)):
        rc, segs, letters = call(seg_cap, letter_cap)
        assert rc == capi.BHIP_E_CAPACITY and (ns.value, nl.value) == (len(exp_segs), len(exp_letters))
        assert set(segs.tolist()) == {0xAB} and set(letters.tolist()) == {0xAB}      # nothing was written
    rc, segs, letters = call(len(exp_segs), len(exp_letters))
    assert rc == capi.BHIP_OK and segs.tobytes() == conslib.seg_bytes(exp_segs) and letters.tobytes() == exp_letters.encode()


def test_no_lines_launch_nothing(pool):
    from burst_amd import capi
    segs, letters = pool.dev.consensus_run(pool.q, np.zeros(0, capi.PILE_LINE_DTYPE), np.zeros(0, np.uint32), 1)
    info = pool.dev.consensus_info()
    assert len(segs) == 0 and letters == b"" and info["device_us"] == 0 and info["segments"] == 0 and info["events"] == 0


def test_every_bad_argument_is_named_and_leaves_the_handle_usable(pool):
    from burst_amd import capi
    good = [0, 5, 9]
    lines, ops = pool.arrays(good)
    n_clumps = len(pool.clump_len)
    cl0 = int(pool.clump_len[0])

    def bad(field=None, value=None, ops_edit=None, min_depth=1, extra=None):
        ln, op = lines.copy(), ops.copy()
        if field:
            ln[field][2] = value
        if ops_edit:
            ops_edit(ln, op)
        if extra is not None:
            ln = np.concatenate([ln, extra])
        with pytest.raises(capi.BurstHipError) as e:
            pool.dev.consensus_run(pool.q, ln, op, min_depth)
        assert e.value.code == capi.BHIP_E_ARG, (field, value)
        assert "bhip_consensus_run" in str(e.value)
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
    assert "min_depth" in bad(min_depth=0)
    exp_segs, exp_letters = conslib.consensus(pool.model_lines(good), 1)
    segs, letters = pool.dev.consensus_run(pool.q, lines, ops, 1)
    assert segs.tobytes() == conslib.seg_bytes(exp_segs) and letters == exp_letters.encode()


def test_the_variants_on_the_same_handle_afterwards(pool):
    """bhip_pile_run shares scratch buffers and stages with bhip_consensus_run: after a consensus call it returns what test_gpu_variants pins"""
    from burst_amd import capi
    idx = list(range(len(pool.cases)))
    lines, ops = pool.arrays(idx)
    pool.dev.consensus_run(pool.q, lines, ops, 1)
    got = pool.dev.pile_run(pool.q, lines, ops, 1, 1)
    sites = pilelib.pile(pool.model_lines(idx))
    exp = pilelib.reported(sites, 1, 1)
    a = np.zeros(len(exp), capi.PILE_SITE_DTYPE)
    for k, r in enumerate(exp):
        a[k] = (r[0], r[1], r[2], r[3], r[4:10], r[10])
    assert got.tobytes() == a.tobytes() and len(exp) > 500
    info = pool.dev.pile_info()
    assert (info["events"], info["candidates"], info["sites"]) == pilelib.figures(sites) + (len(exp),)
    pool.check(idx[::2], 2)      # and the consensus after the variants
