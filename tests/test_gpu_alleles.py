"""bhip_alleles_run against vcflib, the dictionary count of the definition: the alleles it returns and the codes of its deletions, byte for
byte, on cigarlib's pool of lanes and paths (two lanes of one clump on one header, mixed weights), on lines written by hand for every rule
of the definition, on a planted pile-up whose lines all carry one deletion, under a permutation of the lines; then capacity, no lines,
arguments and the call's figures."""
import ctypes as C

import numpy as np
import pytest

import cigarlib as cg
import pilecases
import vcfcases
import vcflib

pytestmark = pytest.mark.gpu


class Pool(pilecases.PileCases):
    def __init__(self, L, z=1):
        from burst_amd import capi
        super().__init__(L, z)
        self.q = capi.Queries(self.queries, [254] * len(self.queries), list(range(len(self.queries))), self.rcs)
        self.dev = capi.Device(self.packed, self.clump_len, self.tot, self.lut, device=0)

    def check(self, idx, min_depth=1, min_alt=1, weights=None):
        """the device's alleles of the cases idx = the model's, byte for byte, and so are the figures"""
        lines, ops = self.arrays(idx, weights)
        got, codes = self.dev.alleles_run(self.q, lines, ops, min_depth, min_alt)
        rows, fig = vcfcases.expect(self.model_lines(idx, weights), min_depth, min_alt)
        vcfcases.same(got, codes, rows)
        vcfcases.info_matches(self.dev.alleles_info(), fig, len(rows))
        return rows, fig


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


@pytest.fixture(scope="module")
def pool(L):
    p = Pool(L, 1)
    yield p
    p.dev.close()


def run_hand(pool, h, min_depth=1, min_alt=1):
    from burst_amd import capi
    q = capi.Queries(h.queries, [254] * len(h.queries))
    got, codes = pool.dev.alleles_run(q, h.rows, h.ops, min_depth, min_alt)
    rows, fig = vcfcases.expect(h.model, min_depth, min_alt)
    vcfcases.same(got, codes, rows)
    vcfcases.info_matches(pool.dev.alleles_info(), fig, len(rows))
    return rows, fig


def test_whole_pool_then_every_kind(pool):
    assert pool.shared is not None and pool.shared[3] >= 1, "no two lanes of the second clump agree where their lines overlap"
    idx = list(range(len(pool.cases)))
    rows, fig = pool.check(idx)
    assert any(r[5] == vcflib.DEL for r in rows) and any(r[5] == vcflib.INS for r in rows) and fig["end"] >= 1
    assert any(r[0] == pool.header[pool.shared[0]] for r in rows)      # an allele on the header two lanes share
    for kd in sorted(set(c["kind"] for c in pool.cases)):
        pool.check([i for i in idx if pool.cases[i]["kind"] == kd])
    info = pool.dev.alleles_info()
    assert info["device_us"] > 0 and info["peak_bytes"] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_line_counts(pool, n):
    rng = np.random.default_rng(n)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=n)]
    pool.check(idx, min_depth=1 if n < 5000 else 3, min_alt=1 if n < 5000 else 2)


def test_every_rule_on_lines_written_by_hand(pool):
    for name, h, check in vcfcases.scenarios(pool):
        rows, fig = run_hand(pool, h)
        check(rows, fig)


@pytest.mark.parametrize("min_depth,min_alt", [(4, 2), (10, 3)])
def test_planted_deletion_either_side_of_both_thresholds(pool, min_depth, min_alt):
    for n_lines, k, want in pilecases.planted_cases(min_depth, min_alt):
        rows, _ = run_hand(pool, vcfcases.planted_del(pool, n_lines, k), min_depth, min_alt)
        vcfcases.check_planted_del(rows, n_lines, k, want)


def test_a_pile_up_of_3000_lines_on_one_deletion(pool):
    """the run length the reduction must not walk serially: 3000 lines, spread over 20 start columns, all carry one deletion"""
    rows, fig = run_hand(pool, vcfcases.planted_del(pool, 3000, 3000, n_del=3), 4, 2)
    vcfcases.check_planted_del(rows, 3000, 3000, 1, n_del=3)
    assert fig["events"] == 3000 and fig["distinct"] == 1 and rows[0][4] == 3000


def test_a_permutation_of_the_lines_gives_identical_bytes(pool):
    rng = np.random.default_rng(3)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=700)]
    lines, ops = pool.arrays(idx)
    a, ca = pool.dev.alleles_run(pool.q, lines, ops, 2, 1)
    b, cb = pool.dev.alleles_run(pool.q, lines[rng.permutation(len(lines))], ops, 2, 1)
    assert len(a) > 50 and len(ca) > 10 and a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()


def test_capacity_of_either_buffer_then_success(pool):
    from burst_amd import capi
    idx = list(range(0, len(pool.cases), 2))
    lines, ops = pool.arrays(idx)
    rows, _ = vcfcases.expect(pool.model_lines(idx))
    exp, exp_codes = vcfcases.arrays_of(rows)
    assert len(exp) > 1 and len(exp_codes) > 1
    na, nc, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)
    call = lambda out, cap, codes, code_cap: capi.lib().bhip_alleles_run(pool.dev._h, capi._ptr(pool.q.codes), capi._ptr(pool.q.off), pool.q.n, capi._ptr(lines), len(lines),
                                                                        capi._ptr(ops), len(ops), 1, 1, capi._ptr(out), cap, C.byref(na), capi._ptr(codes), code_cap, C.byref(nc),
                                                                        capi._ptr(info))
    for cap, code_cap in [(len(exp) - 1, len(exp_codes)), (len(exp), len(exp_codes) - 1)]:
        out = np.frombuffer(bytes([0xAB]) * (40 * len(exp)), np.uint8).copy()
        codes = np.frombuffer(bytes([0xCD]) * len(exp_codes), np.uint8).copy()
        assert call(out, cap, codes, code_cap) == capi.BHIP_E_CAPACITY and (na.value, nc.value) == (len(exp), len(exp_codes))
        assert set(out.tolist()) == {0xAB} and set(codes.tolist()) == {0xCD}      # nothing was written
    out, codes = np.zeros(len(exp), capi.ALLELE_DTYPE), np.zeros(len(exp_codes), np.uint8)
    assert call(out, len(exp), codes, len(exp_codes)) == capi.BHIP_OK and (na.value, nc.value) == (len(exp), len(exp_codes))
    assert out.tobytes() == exp.tobytes() and codes.tobytes() == exp_codes.tobytes()


def test_no_lines_launch_nothing(pool):
    from burst_amd import capi
    got, codes = pool.dev.alleles_run(pool.q, np.zeros(0, capi.PILE_LINE_DTYPE), np.zeros(0, np.uint32), 1, 1)
    info = pool.dev.alleles_info()
    assert len(got) == 0 and len(codes) == 0 and info["device_us"] == 0 and info["events"] == 0


def test_every_bad_argument_is_named_and_leaves_the_handle_usable(pool):
    """only inputs the host check rejects: nothing reaches the device"""
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
            pool.dev.alleles_run(pool.q, ln, op, min_depth, min_alt)
        assert e.value.code == capi.BHIP_E_ARG, (field, value)
        assert "bhip_alleles_run" in str(e.value)
        return str(e.value)

    assert "line 2" in bad("q", pool.q.n)
    assert "line 2" in bad("refIx", pool.tot)
    assert "line 2" in bad("refIx", 16 * n_clumps)
    assert "line 2" in bad("op_off", len(ops))
    assert "line 2" in bad("n_ops", len(ops) + 1)
    k = next(j for j in range(int(lines["op_off"][2]), int(lines["op_off"][2]) + int(lines["n_ops"][2])) if int(ops[j]) & 15 == 7)      # an '=' run of line 2

    def set_op(word):
        def f(ln, op):
            op[k] = word
        return f
    assert "line 2" in bad(ops_edit=set_op(5 << 4 | 3))                     # not I / D / = / X
    assert "line 2" in bad(ops_edit=set_op(0 << 4 | 7))                     # length 0
    assert "line 2" in bad(ops_edit=set_op((int(ops[k]) >> 4) + 1 << 4 | int(ops[k]) & 15))      # ops that do not consume the query's length
    assert "line 2" in bad("ref_first", 0)
    assert "line 2" in bad("ref_first", cl0)
    assert "line 2" in bad("pos", 0)
    assert "line 2" in bad("pos", 0xFFFFFFFF)
    assert "line 2" in bad("w", 0)
    heavy = lines[:1].copy()
    heavy["w"] = 0x7FFFFFFF
    assert "2^31" in bad(extra=heavy)
    for md, ma in [(0, 1), (1, 0), (1 << 31, 1), (1, 1 << 31)]:
        bad(min_depth=md, min_alt=ma)
    rows, _ = vcfcases.expect(pool.model_lines(good))
    got, codes = pool.dev.alleles_run(pool.q, lines, ops, 1, 1)
    vcfcases.same(got, codes, rows)
