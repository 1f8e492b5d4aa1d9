"""The constructed re-scorer cases (rescorelib.build_cases) judged from the reference side alone: the conditions a run of
test_gpu_rescore.py must meet -- every band width on both sides of every register limit, every matrix edge per variant,
enough ties -- hold for the ORACLE's records and the plain DP, so a weak builder cannot make the GPU test pass; and the
oracle itself is pinned on these cases against the compiled reference kernels (where oracle/_ref is built)."""
import numpy as np
import pytest

import dbutil
import oraclelib as ol
import rescorelib as rl


@pytest.fixture(scope="module")
def cs():
    return rl.build_cases()


@pytest.fixture(scope="module")
def runs(cs):
    """(batch, {all_hits: (oracle records, their bands from the DP)}) of the whole case set under score table 1"""
    batch = cs.batch(cs.cases)
    out = {}
    for all_hits in (True, False):
        recs = ol.search(cs.packed, cs.clump_len, cs.tot, batch.codes, batch.off, batch.emac.astype(np.uint32), batch.six, batch.rc,
                         batch.n_shared, cs.lut, all_hits)
        out[all_hits] = (recs, rl.record_bands(recs, batch, cs, cs.lut))
    return batch, out


def family_mask(cs, recs, *families):
    fam = np.array([c.family for c in cs.cases])
    return np.array([any(f.startswith(p) for p in families) for f in fam])[recs["q"]]


def test_bucket_is_the_classifier_table():
    """k_rescore_classify: Wd <= 4, 6, 8, 12, 16, 24, 32, 40, 48 -> the register variants, else the LDS band while Wd <= band_rows,
    else scratch; without the register variants everything up to band_rows is the LDS band's"""
    assert [rl.bucket(w, 48) for w in (3, 4, 5, 12, 13, 48, 49)] == ["4", "4", "6", "12", "16", "48", "scratch"]
    assert [rl.bucket(w, 16, use_reg=False) for w in (3, 16, 17)] == ["lds", "lds", "scratch"]
    assert rl.bucket(40, 16) == "40" and rl.bucket(49, 16) == "scratch"          # a register variant takes a band beyond the LDS plan
    assert [rl.band_rows_of(e) for e in (0, 3, 18, 19, 24, 254)] == [10, 16, 46, 48, 48, 48]


def test_last_row_on_a_worked_example():
    """ACGT against a lane TTACGTTT padded to 10: exact at column 6 only; with one substitution the pads count as mismatches"""
    lut = ol.score_lut(1)
    lane = np.array([4, 4, 1, 2, 3, 4, 4, 4], np.uint8)
    row, ed, e1, e2 = rl.last_row([1, 2, 3, 4], lane, lut, 10)
    assert (ed, e1, e2) == (0, 6, 6) and row.tolist() == [3, 3, 3, 2, 1, 0, 1, 2, 3, 4]
    # the read hangs two symbols over the lane's end: two insertions ending at column 8, or two mismatches against pads ending at 10
    row, ed, e1, e2 = rl.last_row([3, 4, 4, 4, 2, 2], lane, lut, 10)
    assert (ed, e1, e2) == (2, 8, 10) and row[7:].tolist() == [2, 2, 2]
    # a query symbol of code 0 is one edit wherever the alignment ends
    row0, ed0, f0, l0 = rl.last_row([1, 2, 0, 3, 4], lane, lut, 10)
    assert (ed0, f0, l0) == (1, 6, 6) and np.array_equal(row0, rl.last_row([1, 2, 3, 4], lane, lut, 10)[0] + 1)


@pytest.mark.parametrize("all_hits", [True, False])
@pytest.mark.parametrize("ladder", ["ladder_edits", "ladder_span"])
def test_width_coverage(cs, runs, ladder, all_hits):
    """every target width occurs among the oracle's records of each ladder, in both modes: each register limit exactly and one beyond"""
    recs, bands = runs[1][all_hits]
    got = set(bands["Wd"][family_mask(cs, recs, ladder) & (bands["ed"] > 0)].tolist())
    assert set(rl.WIDTHS) <= got, sorted(set(rl.WIDTHS) - got)
    for lim in rl.REG_LIMITS:
        assert lim in got and lim + 1 in got
    if ladder == "ladder_span":
        sel = family_mask(cs, recs, ladder)
        assert (bands["ed"][sel] == 1).all()


@pytest.mark.parametrize("all_hits", [True, False])
def test_edge_coverage(cs, runs, all_hits):
    """per register variant: a band with cells left of column 1, a record ending at the last symbol of a lane with pads behind it,
    a band that runs into the pads, and a record ending on a lane of 256 / 257 / 287 symbols (clump or lane length)"""
    recs, bands = runs[1][all_hits]
    lane_len = np.array([len(s) for s in cs.seqs])[recs["refIx"]]
    L = cs.clump_len[recs["refIx"] >> 4].astype(np.int64)
    bk = np.array([rl.bucket(int(w), 48) for w in bands["Wd"]])
    live = bands["ed"] > 0
    for lim in rl.REG_LIMITS:
        b = live & (bk == str(lim))
        assert (b & (bands["dlo"] < 0)).sum() >= 1, lim
        assert (b & (lane_len < L) & (recs["finalPos"] == lane_len)).sum() >= 1, lim
        assert (b & (lane_len < L) & (bands["e_last"] > lane_len)).sum() >= 1, lim
        for n in (256, 257, 287):
            assert (b & (lane_len == n) & (recs["finalPos"] == n)).sum() >= 1, (lim, n)
            assert (b & (L == n) & (recs["finalPos"] == n)).sum() >= 1, (lim, n)


@pytest.mark.parametrize("all_hits", [True, False])
def test_tie_coverage(cs, runs, all_hits):
    recs, bands = runs[1][all_hits]
    live = bands["ed"] > 0
    several = live & (bands["e_last"] > bands["e_first"])
    counts = {"several best end columns": int(several.sum()), "gapQ > 0": int((recs["gapQ"] > 0).sum()), "gapR > 0": int((recs["gapR"] > 0).sum()),
              "gapQ > 0 and gapR > 0": int(((recs["gapQ"] > 0) & (recs["gapR"] > 0)).sum())}
    print(counts)
    assert all(v >= 20 for v in counts.values()), counts


def test_up_before_left_decides_some_records(cs, runs):
    """The last step of the tie order (diagonal, then up, then left) shows only where an upward and a leftward path meet with equal
    score and equal gapQ but different gapR.  For the early-swap family: the cell-by-cell restatement gives the oracle's record,
    and with up and left ranked equal it gives another one for at least 20 of them."""
    batch, out = runs
    recs, bands = out[True]
    mine = np.flatnonzero(family_mask(cs, recs, "tie_early") & (recs["refIx"] == np.array([c.target for c in cs.cases])[recs["q"]]))
    assert len(mine) > 100
    decisive = 0
    for i in mine:
        q, lane, b = batch.seqs[int(recs["q"][i])], cs.seqs[int(recs["refIx"][i])], bands[i]
        lo = max(0, int(b["dlo"]) - 2)                       # the band's columns and two more on the left (no optimal path leaves the band)
        win = lane[lo:min(len(lane), int(b["e_last"]) + int(b["ed"]) + 1)]
        ed, gq, gr, fin = rl.rescore_cells(q, win, int(b["ed"]), cs.lut)
        assert (ed, gq, gr, fin + lo) == (recs["ed"][i], recs["gapQ"][i], recs["gapR"][i], recs["finalPos"][i]), cs.cases[int(recs["q"][i])].name
        decisive += rl.rescore_cells(q, win, int(b["ed"]), cs.lut, rule="uptie") != (ed, gq, gr, fin)
    print("records resting on up before left:", decisive, "of", len(mine))
    assert decisive >= 20


def test_dp_agrees_with_the_oracle(cs):
    """last_row's ed equals orc_aded_clump's minimum for every lane of every case's clump (the budget set to the read's length, so that
    the oracle reports every lane's minimum)"""
    by_clump = {}
    for c in cs.cases:
        by_clump.setdefault(c.target >> 4, []).append(c)
    for clump, cases in by_clump.items():
        rows = dbutil.clump_rows(cs.seqs, clump)
        L = rows.shape[0]
        omins = np.array([ol.aded_clump(rows, c.q, 254, cs.lut)[1] for c in cases]).astype(np.int64)
        for z in range(min(16, cs.tot - 16 * clump)):
            ed = rl.last_rows([c.q for c in cases], cs.seqs[16 * clump + z], cs.lut, L).min(axis=1)
            assert np.array_equal(np.minimum(ed, 255), omins[:, z]), (clump, z)


@pytest.mark.skipif(not ol.have_reference(), reason="oracle/_ref/libref_harness.so not built")
@pytest.mark.parametrize("z", [1, 0])
def test_oracle_matches_the_compiled_reference_on_every_case(cs, z):
    """as test_aded_and_rescore_match_reference: both sweep variants, re-scoring bounded by the lane's own minimum and by the budget"""
    lut = ol.score_lut(z)
    ol.reference().ref_setscore(z)
    try:
        n_hits = 0
        rows_of = {c: dbutil.clump_rows(cs.seqs, c) for c in range(len(cs.clump_len))}
        for case in cs.cases:
            rows, q, E = rows_of[case.target >> 4], case.q, case.emac
            for variant in (0, 1):
                ret, mins, score, fin, gr, gq = ol.ref_align_clump(rows, q, E, variant=variant)
                oret, omins = ol.aded_clump(rows, q, E, lut)
                assert np.array_equal(mins, omins) and ret == oret, (case.name, variant)
            if ret > E:
                continue
            for zl in range(16):
                if mins[zl] > ret:
                    continue
                lane = rows[:, zl].copy()
                ok, h = ol.rescore_lane(q, lane, ret, lut)
                assert ok, case.name
                assert (h["ed"], h["gapQ"], h["gapR"], h["finalPos"]) == (mins[zl], gq[zl], gr[zl], fin[zl]), (case.name, zl)
                assert h["score"].tobytes() == score[zl].tobytes(), (case.name, zl)
                ok2, h2 = ol.rescore_lane(q, lane, E, lut)
                assert ok2 and h2.tobytes()[8:] == h.tobytes()[8:], (case.name, zl)
                n_hits += 1
            ret2, mins2, score2, fin2, gr2, gq2 = ol.ref_align_clump(rows, q, E, variant=0, bound_override=E)
            for zl in range(16):
                if mins2[zl] > E:
                    continue
                ok, h = ol.rescore_lane(q, rows[:, zl].copy(), E, lut)
                assert ok and (h["ed"], h["gapQ"], h["gapR"], h["finalPos"]) == (mins2[zl], gq2[zl], gr2[zl], fin2[zl]), (case.name, zl)
                assert h["score"].tobytes() == score2[zl].tobytes(), (case.name, zl)
        assert n_hits >= len(cs.cases) * 0.9
    finally:
        ol.reference().ref_setscore(1)
