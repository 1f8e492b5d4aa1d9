"""The constructed sweep cells (sweeplib.CELLS) judged from the reference side alone: what a run of test_gpu_sweep_variants.py relies
on -- every (NW, NWP) pair in a cell of its own, every planted placement a record of the ORACLE, every band class a window of the plain
full-matrix MODEL of the prefix stage -- holds without a device, so a weak builder fails here and cannot pass there.  The model is held
against an independent numpy matrix and against the oracle (every record lies in a lane the model flags: the two-stage argument), and the
oracle's records of two cells against the compiled reference (where oracle/_ref is built)."""
import numpy as np
import pytest

import dbutil
import oraclelib as ol
import rescorelib as rl
import sweeplib as sl

PAIRS = [c for c in sl.CELLS if c.feeder == "pairs"]
TWO_STAGE = [c for c in PAIRS if c.nwp]


def ids(cells):
    return [c.name for c in cells]


def own_records(cell, recs):
    """per read: the oracle's records of the entry that carries it as cut, on the lane it was cut from"""
    return [recs[(recs["q"] == cell.entry_of(i)) & (recs["refIx"] == r.lane)] for i, r in enumerate(cell.reads())]


# ---- the matrix and the restated rules --------------------------------------------------------------------------------------------
def test_prefix_words_rule():
    """class_prefix_words: (6 E + 31) // 32 words out of {1, 2, 3, 4, 6}, none beyond 6, fewer than the query's, none without option
    two_stage or beyond 32 words"""
    assert [sl.prefix_words(e, 32) for e in (0, 1, 5, 6, 10, 11, 16, 17, 21, 22, 32, 33, 254)] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 0, 0]
    assert [sl.prefix_words(16, nw) for nw in (2, 4, 6)] == [0, 3, 3] and sl.prefix_words(22, 6) == 0 and sl.prefix_words(22, 8) == 6
    assert sl.prefix_words(5, 8, two_stage=0) == 0 and sl.prefix_words(5, 33) == 0
    for nwp, (lo, hi) in sl.E_RANGE.items():
        assert sl.prefix_words(lo, 32) == sl.prefix_words(hi, 32) == nwp
        assert sl.prefix_words(lo - 1, 32) != nwp or lo == 1
        assert sl.prefix_words(hi + 1, 32) != nwp


def test_matrix_is_the_rule_and_complete():
    assert sl.TWO_STAGE == sl.rule_matrix()
    pairs = {(nw, nwp) for nw in sl.CLASS_NW for nwp in (1, 2, 3, 4, 6) if nwp < nw}
    assert len(pairs) == 28 and len(sl.TWO_STAGE) == 56
    for pr in pairs:
        rows = [r for r in sl.TWO_STAGE if r[:2] == pr]
        assert len(rows) == 2 and rows[0][2] == sl.LOWER_EDGE[pr[0]] and rows[1][2] == 32 * pr[0], pr
        assert (rows[0][3], rows[1][3]) == sl.E_RANGE[pr[1]][::-1]
    assert all(3 * e < m for _, _, m, e in sl.TWO_STAGE)
    assert (4, 3, 65, 16) in sl.TWO_STAGE                    # P = m: the prefix is the whole query
    for c in sl.CELLS:
        nw = (c.m + 31) // 32 if c.m > 1024 else min(n for n in sl.CLASS_NW if c.m <= 32 * n)
        assert nw == c.nw and sl.prefix_words(c.emax, nw, c.options.get("two_stage", 1)) == c.nwp, c.name
        assert ("_p%d_" % c.nwp) in c.name
    assert {(c.nw, c.nwp) for c in TWO_STAGE} == pairs
    one = [c for c in PAIRS if c.kind == "one_stage"]
    assert sorted((c.nw, c.m) for c in one if c.emax == 33) == [(nw, 32 * nw) for nw in sl.CLASS_NW if nw != 2]
    assert sorted((c.nw, c.m) for c in one if c.options.get("two_stage") == 0) == [(nw, sl.LOWER_EDGE[nw]) for nw in sl.CLASS_NW]
    assert sorted(c.m for c in PAIRS if c.kind == "long") == [1025, 1056, 1057, 4095]


def test_win_class_limits():
    """diags = 8 (g_last - g_first) + 8 + 2 E against 26, 58 and 90"""
    assert [sl.win_class(0, 0, e) for e in (0, 9, 10, 25, 26, 41, 42)] == [0, 0, 1, 1, 2, 2, 3]
    assert [sl.win_class(5, 5 + d, 1) for d in (0, 2, 3, 6, 7, 10, 11)] == [0, 0, 1, 1, 2, 2, 3]


def test_seed_need_and_the_tasks_twins():
    """need = W - E * ceil(K / stride) for reads of A/C/G/T: the widest stride that leaves three words, else the best; the `tasks` cells
    are exactly the two-stage cells whose largest budget keeps one"""
    K = sl.K_ACX
    assert sl.seed_need(100, 3) == (100 - K) // K + 1 - 3             # stride K: 8 words, 3 lost
    assert sl.seed_need(100, 6) == (100 - K) // 6 + 1 - 6 * 2         # stride 12 .. 7 leave fewer than 3: stride 6 does (15 - 12)
    assert sl.seed_need(65, 16) == 0 and sl.seed_need(11, 0) == 0
    assert sl.seed_need(4095, 10) == (4095 - K) // 17 + 1 - 10        # more than 255 words at stride 16: the first stride is 17
    twins = {c.name for c in sl.CELLS if c.feeder == "tasks"}
    assert twins == {c.name.replace("_pairs", "_tasks") for c in TWO_STAGE if sl.seed_need(c.m, c.emax) >= 1}
    # the rows that lose the prefilter route, written out (sweeplib.PAIRS_ONLY): a change of seed_need or K_ACX that drops a twin fails here
    assert tuple(r for r in sl.TWO_STAGE if sl.seed_need(r[2], r[3]) < 1) == sl.PAIRS_ONLY and len(sl.PAIRS_ONLY) == 16
    assert twins == {"nw%d_p%d_m%d_e%d_tasks" % r for r in sl.TWO_STAGE if r not in sl.PAIRS_ONLY} and len(twins) == 40
    assert {(c.nw, c.nwp) for c in TWO_STAGE} - {(c.nw, c.nwp) for c in sl.CELLS if c.feeder == "tasks"} == {(4, 3), (6, 4), (8, 6)}
    assert {c.nwp for c in sl.CELLS if c.feeder == "tasks"} == {1, 2, 3, 4, 6}
    for c in sl.CELLS:
        if c.feeder == "tasks":
            assert sl.twin_source(c).batch().codes.tobytes() == c.batch().codes.tobytes() and c.batch().flags is not None


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_model_equals_an_independent_matrix():
    """sw_prefix_rows against rescorelib.last_rows (numpy, written for the re-scorer tests) on random lanes with pads and IUPAC codes"""
    rng = np.random.default_rng(5)
    lut = sl.lut()
    for P in (1, 7, 32, 65, 192):
        lanes = np.zeros((5, 96 + 32 * (P % 3)), np.uint8)
        for z in range(5):
            n = lanes.shape[1] - int(rng.integers(0, 40))
            lanes[z, :n] = rng.integers(1, 5, size=n)
            lanes[z, rng.integers(0, n, size=3)] = rng.integers(5, 16, size=3)
        q = rng.integers(1, 5, size=P + 9).astype(np.uint8)
        q[P // 2] = 8
        st = int(rng.integers(0, 20))
        q[:min(P, 60)] = np.where(rng.random(min(P, 60)) < 0.9, lanes[0, st:st + min(P, 60)], q[:min(P, 60)])
        q[q == 0] = 1
        got = sl.prefix_rows(q, P, lanes, lut)
        for z in range(5):
            assert np.array_equal(got[z], rl.last_rows([q[:P]], lanes[z], lut, lanes.shape[1])[0]), (P, z)


def test_model_on_a_worked_example():
    """ACGT against TTACGTTT padded to 16 columns: exact in column 6 (group 0); with a budget of 1 group 1 is flagged too (column 9 costs
    3, 8 costs 2, 7 costs 1 -- all in group 0 -- so it is not); the pads never match"""
    lut = sl.lut()
    lane = np.zeros((1, 16), np.uint8)
    lane[0, :8] = [4, 4, 1, 2, 3, 4, 4, 4]
    row = sl.prefix_rows(np.array([1, 2, 3, 4], np.uint8), 4, lane, lut)[0]
    assert row.tolist() == [3, 3, 3, 2, 1, 0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4]
    assert (row.reshape(-1, 8).min(axis=1) <= 1).tolist() == [True, False]


# ---- the cells ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", PAIRS, ids=ids(PAIRS))
def test_cell_is_built_as_specified(cell):
    """entries, budgets, lengths, start columns and lanes of the planted reads.
    The cells of 513 symbols and more hold 8 reads (2 at 4 095 symbols) instead of 24, to keep the oracle's side short, and that is a
    deliberate cut: they leave out the plain column-1 read (the one with its first symbol inserted stays), the substitutions-only read
    with Emax edits, the starts at columns 1 modulo 8 and 32 / 33 modulo 64, and at 4 095 symbols everything but the prefix and the
    suffix read -- no over-budget read there.  The assertions below are the weaker for those sizes; the 24-read cells of the classes
    up to 512 symbols carry the full list."""
    db, rs, b = sl.class_db(cell.key), cell.reads(), cell.batch()
    assert len(rs) == (2 if cell.m == 4095 else 8 if cell.m >= 513 else 24) and b.n == 2 * len(rs)
    assert all(len(s) == cell.m for s in b.seqs) and int(b.emac.max()) == cell.emax
    assert all((s >= 1).all() and (s <= 4).all() for s in b.seqs)
    es = [r.e for r in rs]
    assert 2 * es.count(cell.emax) >= len(rs) and set(es) <= set(cell.budgets)
    if len(rs) > 2:
        assert set(es) == set(cell.budgets)
    assert db.tot == 46 and len(db.clump_len) == 3 and len(db.repeat) == 12
    assert all(3 <= len(db.unit) <= 8 and 40 <= n <= 160 for _, n in db.repeat.values())
    for r in rs:
        assert 0 <= r.start and r.start + cell.m - r.k - 2 <= db.lens[r.lane]
    cols8 = {(r.start + 1) % 8 for r in rs}
    cols64 = {(r.start + 1) % 64 for r in rs}
    if len(rs) == 24:
        assert {0, 1, 7} <= cols8 and {31, 32, 33} <= cols64
    elif len(rs) == 8:
        assert {0, 7} <= cols8 and 31 in cols64
    if len(rs) > 2:
        short = [r for r in rs if r.place == "end_short"]
        full = [r for r in rs if r.place == "end_full"]
        assert short and all(db.lens[r.lane] + 30 <= db.clump_len[r.lane >> 4] and r.start + cell.m == db.lens[r.lane] for r in short)
        assert full and all(db.lens[r.lane] == db.clump_len[r.lane >> 4] and r.start + cell.m == db.lens[r.lane] for r in full)
        assert any(r.start == 0 for r in rs)
    rep = [r for r in rs if r.lane in db.repeat and r.start == db.repeat[r.lane][0]]
    assert len(rep) >= (1 if cell.m == 4095 else 2)


@pytest.mark.parametrize("cell", PAIRS, ids=ids(PAIRS))
def test_oracle_returns_what_the_cell_is_for(cell):
    """records with ed = Emax; a record on its own lane for every planted placement; ends on the last column of a lane as long as its clump
    and of a shorter one; a read with one edit more than its budget that returns nothing on its own lane"""
    db, rs = sl.class_db(cell.key), cell.reads()
    recs = sl.expected(cell, True)
    own = own_records(cell, recs)
    assert (recs["ed"] == cell.emax).sum() >= 2
    assert (recs["rc"] == 1).any() and (recs["rc"] == 0).any()
    for i, r in enumerate(rs):
        if r.place == "over":
            continue
        assert len(own[i]) == 1 and own[i]["ed"][0] <= r.k, (r.place, i)
    places = {r.place for r in rs}
    want = {"prefix", "suffix"} if cell.m == 4095 else {"prefix", "suffix", "boundary_del", "boundary_ins", "col1_ins", "end_full", "end_short", "over"}
    if len(rs) == 24:
        want |= {"col1", "subs", "exact", "repeat"}
    assert want <= places
    if len(rs) > 2:
        assert any(len(own[i]) == 0 for i, r in enumerate(rs) if r.place == "over")
        for place in ("end_full", "end_short"):
            assert any(own[i]["finalPos"][0] == db.lens[r.lane] for i, r in enumerate(rs) if r.place == place), place
        assert any(own[i]["ed"][0] == 1 for i, r in enumerate(rs) if r.place == "col1_ins")
    if cell.nwp and cell.m - 1 - cell.P >= cell.emax:          # room for Emax edits behind the prefix
        assert any(r.strict and r.k == r.e == cell.emax and len(own[i]) == 1 for i, r in enumerate(rs) if r.place == "suffix")
    if cell.nwp and cell.P < cell.m:
        assert any(r.strict for r in rs if r.place == "boundary_del")
    if cell.nwp:
        assert any(r.strict and r.k == r.e == cell.emax and len(own[i]) == 1 for i, r in enumerate(rs) if r.place == "prefix")


@pytest.mark.parametrize("cell", TWO_STAGE, ids=ids(TWO_STAGE))
def test_model_windows_populate_every_band_class(cell):
    """The windows of the plain model: every band class the cell can have (Cell.band_classes, from the formula) has one, the smallest
    class of the LARGEST budget is reached by an entry of that budget, and every record of the oracle lies in a lane the model flags --
    an alignment within budget holds an alignment of the prefix within budget."""
    b = cell.batch()
    g_first, g_last, cls = sl.model(cell)
    assert ((g_first >= 0) == (cls >= 0)).all() and (g_last >= g_first).all()
    assert np.array_equal(cls[cls >= 0], [sl.win_class(a, z, e) for a, z, e in
                                          zip(g_first[cls >= 0], g_last[cls >= 0], np.broadcast_to(b.emac[:, None], cls.shape)[cls >= 0])])
    hist = [int((cls == k).sum()) for k in range(4)]
    print(cell.name, "windows per band class", hist)
    if cell.nw == 2:
        assert cell.band_classes == ()
    else:
        assert cell.band_classes == (0, 1, 2, 3)
        assert all(hist[k] > 0 for k in cell.band_classes), hist
        top = cls[b.emac == cell.emax]
        assert (top == sl.win_class(0, 0, cell.emax)).any()
        assert (top[top >= 0] >= sl.win_class(0, 0, cell.emax)).all()
    for all_hits in (True, False):
        recs = sl.expected(cell, all_hits)
        assert (g_first[recs["q"], recs["refIx"]] >= 0).all()
    dead = np.arange(cls.shape[1]) >= sl.class_db(cell.key).tot
    assert not dead.any()                                    # (the model runs over live lanes only)


def test_siblings_fall_inside_the_larger_budgets():
    """class_rate: with budgets from 16 up a read that leaves half its budget unspent also meets references of its lane's family"""
    for cell in PAIRS:
        if cell.kind == "long" or cell.emax < 16:
            continue
        rs, recs = cell.reads(), sl.expected(cell, True)
        planted = np.array([rs[int(q) % len(rs)].lane for q in recs["q"]])
        n = int((recs["refIx"] != planted).sum())
        print(cell.name, "records on other lanes:", n)
        assert n >= 1, cell.name


def test_all_hits_false_is_the_minimum_of_all_hits_true():
    """the two modes of the oracle on one cell per class: the minimum-only records are those of every-hit mode at the slot's minimum"""
    for nw in sl.CLASS_NW:
        cell = next(c for c in TWO_STAGE if c.nw == nw)
        every, least = sl.expected(cell, True), sl.expected(cell, False)
        best = {}
        for r in every:
            s = int(r["q"]) % cell.batch().n_shared
            best[s] = min(best.get(s, 255), int(r["ed"]))
        keep = np.array([int(r["ed"]) == best[int(r["q"]) % cell.batch().n_shared] for r in every])
        assert len(least) == keep.sum() and np.array_equal(least[["q", "refIx", "ed"]], every[keep][["q", "refIx", "ed"]])


@pytest.mark.skipif(not ol.have_reference(), reason="oracle/_ref/libref_harness.so not built")
@pytest.mark.parametrize("name", ["nw4_p3_m65_e16_pairs", "nw10_p6_m257_e32_pairs"])
def test_oracle_matches_the_compiled_reference_on_two_cells(name):
    """the lanes within budget and their records (every-hit mode: re-scored under the budget) from the reference's own kernels"""
    cell = sl.BY_NAME[name]
    db, b, lut = sl.class_db(cell.key), cell.batch(), sl.lut()
    recs = sl.expected(cell, True)
    ol.reference().ref_setscore(1)
    n = 0
    for c in range(len(db.clump_len)):
        rows = dbutil.clump_rows(db.seqs, c)
        for j in range(b.n):
            q, E = b.seqs[j], int(b.emac[j])
            ret, mins, score, fin, gr, gq = ol.ref_align_clump(rows, q, E, variant=0, bound_override=E)
            oret, omins = ol.aded_clump(rows, q, E, lut)
            assert ret == oret and np.array_equal(mins, omins), (j, c)
            mine = recs[(recs["q"] == j) & (recs["refIx"] >> 4 == c)]
            lanes = [z for z in range(16) if 16 * c + z < db.tot and mins[z] <= E]
            assert mine["refIx"].tolist() == [16 * c + z for z in lanes], (j, c)
            for h, z in zip(mine, lanes):
                assert (h["ed"], h["gapQ"], h["gapR"], h["finalPos"]) == (mins[z], gq[z], gr[z], fin[z]), (j, c, z)
                assert h["score"].tobytes() == score[z].tobytes(), (j, c, z)
                n += 1
    assert n == len(recs) and n > 30
