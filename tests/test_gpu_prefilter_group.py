"""k_prefilter_cq with eight queries per wave (8 lanes each, option prefilter_group = 8) against four (16 lanes each, = 16) and the oracle:
the same records, the same lane tasks and clump pairs, at the smallest shapes at which the group geometry can go wrong -- partial octets,
1 .. 8 lists per query, streams around the 64-record rows and beyond the two resident ones, survivor counts around a round of 8, the
16-slot exact table, the BIG pass and the dense fallback, a last clump of fewer than 16 sequences, clumps on the BadList, and a row of
16 words (which runs 16 lanes whatever the option says).

List records read: a query that overflows the first pass's exact table is read once more by the BIG pass, and that table holds 16 clumps
with 8 lanes per query and 32 with 16.  So the counter is equal wherever the two widths report the same number of overflowed queries, and
larger for 8 lanes where more queries overflowed; lane tasks and clump pairs are equal everywhere."""
import re

import numpy as np
import pytest

import dbutil
import oraclelib as ol
from burst_amd import synth
from test_gpu_kernels import assert_hits_equal, budget, family_db, make_queries, oracle_hits, staged_call, with_debug_lines  # noqa: F401

pytestmark = pytest.mark.gpu

K = 12
WIDTH = {8: "eight queries per wave, 8 lanes each", 16: "four queries per wave, 16 lanes each"}


def fwd_queries(reads, E):
    from burst_amd import capi
    n = len(reads)
    q = capi.Queries(reads, list(E), list(range(n)), [0] * n)
    q.flags = np.zeros(q.n, np.uint8)
    return q


def device(seqs, **kw):
    from burst_amd import capi
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=K, **kw)
    dev.set_option("prefilter_stride", K)
    return dev, (packed, clump_len, tot, lut), (lens, entries, offs)


def run(dev, q, group, all_hits, capfd, monkeypatch):
    """one batch under BHIP_DEBUG: records, the statistics that must not depend on the width, what the debug lines say"""
    dev.set_option("prefilter_group", group)
    got, lines = with_debug_lines(capfd, monkeypatch, lambda: dev.align_batch(q, all_hits=all_hits))
    st = dev.stats()
    kern = [ln for ln in lines if "prefilter kernel:" in ln]
    ovf = [re.search(r"(\d+) queries overflowed the first prefilter pass, (\d+) the second", ln) for ln in lines]
    ovf = [m for m in ovf if m]
    routed = [re.search(r"prefiltered (\d+) exhaustive (\d+)", ln) for ln in lines]
    info = dict(kernel_lines=kern, n_fb=sum(int(m.group(1)) for m in ovf), n_fb2=sum(int(m.group(2)) for m in ovf),
                prefiltered=sum(int(m.group(1)) for m in routed if m), exhaustive=sum(int(m.group(2)) for m in routed if m))
    return got, dict(records_read=st["acx_entries_read"], lane_tasks=st["n_lane_tasks"], clump_pairs=st["n_pairs"]), info


def both_widths(dev, q, exp, all_hits, capfd, monkeypatch, ran8=8):
    """prefilter_group = 8 and = 16: equal records (and the oracle's), statistics as the module's docstring says, the width named in the debug line"""
    out = {}
    for group in (8, 16):
        got, st, info = run(dev, q, group, all_hits, capfd, monkeypatch)
        assert_hits_equal(got, exp)
        want = WIDTH[ran8 if group == 8 else 16]
        assert info["kernel_lines"] and all(want in ln for ln in info["kernel_lines"]), (group, info["kernel_lines"])
        out[group] = (st, info)
    dev.set_option("prefilter_group", 0)
    (s8, i8), (s16, i16) = out[8], out[16]
    print("group 8:", s8, {k: v for k, v in i8.items() if k != "kernel_lines"}, "| group 16:", s16, {k: v for k, v in i16.items() if k != "kernel_lines"})
    assert i8["prefiltered"] == i16["prefiltered"] and i8["n_fb2"] == i16["n_fb2"]
    assert s8["lane_tasks"] == s16["lane_tasks"] and s8["clump_pairs"] == s16["clump_pairs"]
    assert i8["n_fb"] >= i16["n_fb"]
    assert s8["records_read"] == s16["records_read"] if i8["n_fb"] == i16["n_fb"] else s8["records_read"] > s16["records_read"]
    return out


def modes(dev):
    """BEST / minimum and every hit, with and without the deferred second sweep"""
    for all_hits in (False, True):
        for prune in (1, 0):
            dev.set_option("prune", prune)
            yield all_hits
    dev.set_option("prune", 1)


# ---- partial octets, three lanes, the last clump ----
@pytest.fixture(scope="module")
def small():
    seqs = family_db(701, 6, 11, 400)                       # 66 sequences: four clumps of 16 and one of 2
    assert len(seqs) % 16 == 2
    dev, db, _ = device(seqs)
    reads, _ = synth.make_reads(seqs, 16, 100, [0, 1, 2], 702)
    reads = [np.array(seqs[-1][40:140], np.uint8)] + reads   # the first query's best hit sits in the last, short clump
    E = [budget(0.97, 100)] * len(reads)
    exp = {}
    for n in (1, 7, 8, 9, 15, 16, 17):
        q = fwd_queries(reads[:n], E[:n])
        exp[n] = (q, {ah: oracle_hits(*db[:3], q, db[3], ah) for ah in (False, True)})
    yield dev, seqs, exp
    dev.close()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17])
def test_partial_octets(small, n, capfd, monkeypatch):
    """n queries in the list: idle groups in the last wave, a last octet whose idle groups read clamped addresses"""
    dev, seqs, exp = small
    q, e = exp[n]
    assert np.any(e[True]["q"] == 0) and len(e[True]) >= n // 2 + 1      # (query 0 was cut from the last sequence: a candidate in the short clump)
    for all_hits in modes(dev):
        out = both_widths(dev, q, e[all_hits], all_hits, capfd, monkeypatch)
        assert out[8][1]["prefiltered"] == n and out[8][1]["exhaustive"] == 0


def test_three_lanes(small, capfd, monkeypatch):
    """the queries spread over three sub-pipelines: three short lists, each with its own partial octet"""
    dev, _, exp = small
    q, e = exp[17]
    dev.set_option("lane_min_entries", 4); dev.set_option("lanes", 3)
    try:
        for all_hits in modes(dev):
            out = both_widths(dev, q, e[all_hits], all_hits, capfd, monkeypatch)
            assert len(out[8][1]["kernel_lines"]) >= 2           # (more than one lane did launch)
    finally:
        dev.set_option("lanes", 1)


# ---- 1 .. 8 lists per query, one of them without a single list ----
def test_list_counts(capfd, monkeypatch):
    """Reads of 12 w + 5 symbols sample w = 1 .. 8 words at stride K = 12.  Budgets: w - 3 edits for w >= 3, so that the guaranteed count
    (one edit destroys one word) is 3 at each of those counts; w = 1 and 2 cannot guarantee 3 words and get a budget of 0 (need = w).
    A random read, none of whose words has a list, sits between live neighbours."""
    seqs = family_db(731, 8, 6, 400, rate=0.02)
    dev, db, (lens, entries, offs) = device(seqs)
    rng = np.random.default_rng(735)
    reads, E = [], []
    for rep in range(3):
        for w in range(1, 9):
            r, _ = synth.make_reads(seqs, 1, 12 * w + 5, [0, 1] if w >= 4 else [0], 740 + 10 * rep + w)
            reads += r; E.append(max(0, w - 3))
            if w == 4:
                reads.append(rng.integers(1, 5, size=101, dtype=np.uint8)); E.append(3)

    def list_len(read, p):
        w = 0
        for c in np.asarray(read[p:p + K], np.int64) - 1:
            w = (w << 2) | int(c)
        return int(lens[w])
    dead = [i for i, r in enumerate(reads) if len(r) == 101 and all(list_len(r, p) == 0 for p in range(0, 101 - K + 1, K))]
    assert len(dead) == 3 and all(0 < i < len(reads) - 1 for i in dead), dead
    q = fwd_queries(reads, E)
    for all_hits in modes(dev):
        exp = oracle_hits(*db[:3], q, db[3], all_hits)
        assert len(exp) >= 16
        out = both_widths(dev, q, exp, all_hits, capfd, monkeypatch)
        assert out[8][1]["prefiltered"] >= 3 * 6 + 3             # every read with w >= 3 words and the three dead ones go through the prefilter
    dev.close()


# ---- stream lengths and survivor counts ----
CLASSES = ("none", "le8", "9to16", "gt16", "gt32", "dense")


def mixed_inputs():
    """One database with word lists of 1, 2, ~12, ~25, ~55 and > 300 clumps: singletons, pairs, families of 12 / 25 / 60 and one of 5 200,
    shuffled over 338 clumps (the last one holds 7 sequences).  Reads of 100 symbols with a budget of 3 (8 words at stride 12, need 5), the
    longest lists never left out (seed_min_need 0), so that a query's stream and its surviving clumps follow from dbutil.build_acx's lists."""
    rng = np.random.default_rng(710)
    fams = {"single": family_db(711, 45, 1, 300), "pair": family_db(712, 4, 2, 300, rate=0.004), "f12": family_db(713, 3, 12, 300, rate=0.01),
            "f25": family_db(714, 2, 25, 300, rate=0.01), "f60": family_db(715, 1, 60, 300, rate=0.01), "big": family_db(141, 1, 5200, 300, rate=0.02)}
    seqs = [s for f in fams.values() for s in f]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    assert len(seqs) % 16 == 7
    lens, entries, offs = dbutil.build_acx(seqs, K)
    E3 = 3

    def model(read):
        """(records of the stream, surviving records, distinct surviving clumps) from the clump lists: one record per (word, clump)"""
        cnt, T = {}, 0
        for p in range(0, len(read) - K + 1, K):
            w, ok = 0, True
            for c in np.asarray(read[p:p + K], np.int64) - 1:
                ok &= 0 <= c < 4; w = (w << 2) | int(c & 3)
            if not ok:
                continue
            lst = entries[int(offs[w]):int(offs[w + 1])]
            T += len(lst)
            for c in lst:
                cnt[int(c)] = cnt.get(int(c), 0) + 1
        need = 8 - E3
        surv = [v for v in cnt.values() if v >= need]
        return T, sum(surv), len(surv)
    pools = {}
    singles = fams["single"]
    chim = [np.concatenate([np.asarray(singles[(8 * i + j) % len(singles)][20 + 12 * j:32 + 12 * j], np.uint8) for j in range(8)] + [np.array([1, 2, 3, 4], np.uint8)]) for i in range(6)]
    pools["none"] = chim
    pools["le8"] = synth.make_reads(fams["single"], 6, 100, [0, 1], 716)[0] + [np.array(seqs[-1][30:130], np.uint8)]
    pools["9to16"] = synth.make_reads(fams["pair"], 6, 100, [0], 717)[0]
    pools["gt16"] = synth.make_reads(fams["f25"], 6, 100, [0, 1], 718)[0]
    pools["gt32"] = synth.make_reads(fams["f60"], 6, 100, [0, 1], 719)[0]
    pools["dense"] = synth.make_reads(fams["big"], 6, 100, [0, 1], 720)[0]
    pools["f12"] = synth.make_reads(fams["f12"], 6, 100, [0, 1], 721)[0]
    keep = dict(none=lambda T, S, D: T > 0 and S == 0, le8=lambda T, S, D: 1 <= S <= 8 and T <= 64, **{"9to16": lambda T, S, D: 9 <= S <= 16 and D <= 16},
                gt16=lambda T, S, D: 16 < D <= 32 and T > 128, gt32=lambda T, S, D: 32 < D <= 128, dense=lambda T, S, D: D > 128, f12=lambda T, S, D: 64 < T <= 128)
    sel = {k: [r for r in pools[k] if keep[k](*model(r))] for k in pools}
    assert all(len(v) >= 2 for v in sel.values()), {k: (len(v), [model(r) for r in pools[k]]) for k, v in sel.items()}
    # every class beside a query without survivors inside every run of eight: the classes in a cycle of seven, "none" twice
    order = ["none", "le8", "9to16", "none", "gt16", "f12", "gt32", "dense"]
    reads = [sel[k][i % len(sel[k])] for i in range(3) for k in order]
    counts = dict(gt16=sum(1 for r in reads if 16 < model(r)[2]), gt32=sum(1 for r in reads if 32 < model(r)[2]), dense=sum(1 for r in reads if 128 < model(r)[2]))
    return seqs, reads, counts


@pytest.fixture(scope="module")
def mixed():
    seqs, reads, counts = mixed_inputs()
    dev, db, _ = device(seqs)
    dev.set_option("seed_min_need", 0)
    assert budget(0.97, 100) == 3
    q = fwd_queries(reads, [3] * len(reads))
    exp = {ah: oracle_hits(*db[:3], q, db[3], ah) for ah in (False, True)}
    yield dev, q, exp, counts
    dev.close()


def test_streams_and_survivors(mixed, capfd, monkeypatch):
    """Streams of <= 64, 65 .. 128 and > 128 records and queries with no, <= 8, 9 .. 16 survivor records, more surviving clumps than the
    exact table holds (16 with 8 lanes, 32 with 16: the BIG pass) and more than 128 (dense fallback) in one batch, interleaved.  The
    overflow counters of the debug line must reach what the clump lists say (false survivors can only add)."""
    dev, q, exp, counts = mixed
    assert counts["dense"] >= 3 and counts["gt32"] > counts["dense"] and counts["gt16"] > counts["gt32"]
    for all_hits in modes(dev):
        assert len(exp[all_hits]) >= 16
        out = both_widths(dev, q, exp[all_hits], all_hits, capfd, monkeypatch)
        assert out[8][1]["n_fb"] >= counts["gt16"] and out[16][1]["n_fb"] >= counts["gt32"]
        assert out[8][1]["n_fb2"] >= counts["dense"]
        assert out[8][1]["n_fb"] > out[16][1]["n_fb"]            # the 16-slot table did overflow where the 32-slot one held


# ---- clumps on the BadList ----
def test_ambiguous_clumps_every_lane_once(capfd, monkeypatch):
    """A reference with a run of 70 three-way ambiguity codes (59 windows of 3^12 words: more than the 2^24 a clump may expand to) puts its
    clump on the BadList of the accelerator the device builds: every query is swept against all 16 lanes of that clump, lanes 8 .. 15
    included -- with 8 lanes per query in two halves.  Same records, same number of lane tasks and pairs as with 16 lanes, and at
    least 16 tasks per query."""
    from burst_amd import capi
    clean = family_db(721, 6, 8, 360)
    dirty = family_db(722, 2, 8, 360, iupac=0.01)
    for s in dirty[:2]:
        s[100:170] = 12                                                   # B = C, G or T
    seqs = clean[:32] + dirty + clean[32:] + family_db(723, 1, 7, 360)      # clump 2 is the ambiguous one; the last clump holds 7 sequences
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, K=K, build_acx=True)
    dev.set_option("prefilter_stride", K)
    reads, _ = synth.make_reads(clean, 11, 100, [0, 1, 2], 724)
    q = fwd_queries(reads, [budget(0.97, 100)] * len(reads))
    for all_hits in modes(dev):
        exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        assert len(exp) >= len(reads)
        out = both_widths(dev, q, exp, all_hits, capfd, monkeypatch)
        assert out[8][1]["prefiltered"] == len(reads)
        assert out[8][0]["lane_tasks"] >= 16 * len(reads)               # (the 16 lanes of the clump on the BadList, for every query)
    dev.close()


# ---- a row of 16 words ----
def test_wide_rows_run_sixteen_lanes(capfd, monkeypatch):
    """150-symbol reads sample 12 words at stride 12: rows of 16 words, slot mode 1.  prefilter_group = 8 does not fail and does not run 8
    lanes: the debug line names four queries per wave, and the records are the oracle's."""
    seqs = family_db(741, 6, 9, 420)
    dev, db, _ = device(seqs)
    q, _ = make_queries(seqs, 20, 150, [0, 1, 2, 4], 742, thres=0.97)
    q.flags = np.zeros(q.n, np.uint8)
    for all_hits in (False, True):
        exp = oracle_hits(*db[:3], q, db[3], all_hits)
        assert len(exp) >= 20
        both_widths(dev, q, exp, all_hits, capfd, monkeypatch, ran8=16)
    dev.close()
