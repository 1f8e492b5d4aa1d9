"""Option "fetch_once": the register-band re-scorer takes a hit's packed query from a private LDS column copied once, or 16 bytes per 32
rows where the class is too long for that.  Only where the operand comes from changes: every batch runs with fetch_once 1 and 0, the
records are byte-equal to each other and to the oracle, and the library's BHIP_DEBUG line "re-scorer query fetch ..." says which form ran."""
import re

import numpy as np
import pytest

import dbutil
import oraclelib as ol
import rescorelib as rl
from burst_amd import synth
from test_gpu_kernels import assert_hits_equal, budget, family_db, make_queries, oracle_hits, staged_call, with_debug_lines

pytestmark = pytest.mark.gpu

QF_LINE = re.compile(r"re-scorer query fetch 4-8:(\w+)/(\d+) 12:(\w+)/(\d+) 16-24:(\w+)/(\d+) 32-48:(\w+)/(\d+)")
BANDS_LINE = re.compile(r"re-scorer bands " + " ".join("%s:(\\d+)" % b for b in rl.BUCKETS))


def run(dev, q, all_hits, fetch_once, capfd, monkeypatch):
    """the batch through bhip_align_staged under fetch_once, twice at most (the first call of a handle may grow buffers and redo):
    (records, query-fetch forms per register set [(form, LDS bytes)] x 4, variant histogram)"""
    from burst_amd import capi
    dev.set_option("fetch_once", fetch_once)
    dev.stage(q)
    buf = np.zeros(1 << 17, dtype=capi.HIT_DTYPE)
    for _ in range(2):
        (rc, n), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, int(all_hits), buf))
        assert rc == capi.BHIP_OK, (rc, capi.lib().bhip_last_error(), lines)
        if not [ln for ln in lines if "redo:" in ln]:
            break
    else:
        raise AssertionError("the second call redid the chain again: %r" % lines)
    qf = [m for m in map(QF_LINE.search, lines) if m]
    assert qf, lines
    forms = [[(m.group(2 * i + 1), int(m.group(2 * i + 2))) for i in range(4)] for m in qf]
    assert all(f == forms[0] for f in forms)
    found = [m for m in map(BANDS_LINE.search, lines) if m]
    hist = {b: sum(int(m.group(i + 1)) for m in found) for i, b in enumerate(rl.BUCKETS)}
    return buf[:n].copy(), forms[0], hist


def both(dev, q, exp, all_hits, capfd, monkeypatch):
    """fetch_once 1 and 0: records equal to each other and to the oracle, the old forms under 0; the forms and histogram under 1"""
    got1, qf1, hist = run(dev, q, all_hits, 1, capfd, monkeypatch)
    got0, qf0, hist0 = run(dev, q, all_hits, 0, capfd, monkeypatch)
    dev.set_option("fetch_once", 1)
    assert got1.tobytes() == got0.tobytes()
    assert_hits_equal(got1, exp)
    assert qf0 == [("dword", 0)] * 4 and hist == hist0
    return qf1, hist


def edge_reads(seqs, qlen, rng, hang):
    """reads at the edges of a lane: cut from its first and last columns, one column in, and hanging over either end by `hang` symbols
    (the band then starts left of column 1 / the read ends in the pads behind a short lane)"""
    out = []
    for i in range(0, len(seqs), 5):
        sq = np.array(seqs[i], np.uint8)
        if len(sq) < qlen + 2:
            continue
        out += [sq[:qlen].copy(), sq[len(sq) - qlen:].copy(), sq[1:qlen + 1].copy()]
        if hang and qlen > 2 * hang:
            out += [np.concatenate([rng.integers(1, 5, size=hang, dtype=np.uint8), sq[:qlen - hang]]),
                    np.concatenate([sq[len(sq) - (qlen - hang):], rng.integers(1, 5, size=hang, dtype=np.uint8)])]
    return out


@pytest.mark.parametrize("qlen", [8, 9, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129])
def test_query_lengths_at_the_fetch_boundaries(qlen, capfd, monkeypatch):
    """the dword (8), 16-byte (32 symbols) and 32-row boundaries of the query fetch and the edge of set 0's LDS form (128 symbols = 16
    dwords): reads with edits from inside the references and at the edges of lanes (dlo < 0, reads hanging into the pads of short lanes),
    an ambiguity code at the first and the last position of a staged dword, both score tables"""
    from burst_amd import capi
    rng = np.random.default_rng(9000 + qlen)
    seqs = family_db(9100 + qlen, 3, 5, qlen + 90, short=True)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    E = max(2, budget(0.95, qlen)) if qlen > 9 else 2
    reads, _ = synth.make_reads(seqs, 16, qlen, [0, 1, 2, E], 9200 + qlen, rc_frac=0.0)
    reads = [np.array(r, np.uint8) for r in reads] + edge_reads(seqs, qlen, rng, 1 if qlen < 31 else 2)
    for i, r in enumerate(reads[:12]):          # ambiguity codes: first / last symbol of a dword, of the first, a middle and the last dword
        d = (0, (len(r) - 1) // 16, (len(r) - 1) // 8)[i % 3]
        p = min(len(r) - 1, 8 * d + (7 if i % 2 else 0))
        if p:
            r[p] = 15 if i % 4 < 2 else int(rng.integers(5, 15))
    n = len(reads)
    allq = reads + [synth.revcomp(r) for r in reads]
    q = capi.Queries(allq, [E] * (2 * n), list(range(n)) * 2, [0] * n + [1] * n)
    qw = (max(len(r) for r in allq) + 7) // 8
    for z in (1, 0):
        lut = ol.score_lut(z)
        dev = capi.Device(packed, clump_len, tot, lut)
        for all_hits in (True, False):
            exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
            qf, hist = both(dev, q, exp, all_hits, capfd, monkeypatch)
            print(qlen, z, all_hits, qf, hist)
            assert sum(hist[b] for b in ("4", "6", "8")) > 10          # hits that were re-scored, in set 0
            assert qf[0] == ("lds", qw * 256)                          # up to 128 symbols certainly; 129 = 17 dwords still fit beside 7 waves
        dev.close()


def test_long_class_takes_the_chunk_form(capfd, monkeypatch):
    """600-symbol reads, 75 dwords a row (no multiple of four: rows start at every dword of a 16-byte chunk): too long for an LDS column
    beside the resident waves, so the wide register sets take the query 16 bytes per 32 rows; budgets of 12 put hits into them"""
    from burst_amd import capi
    seqs = family_db(9301, 3, 5, 760, short=True)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    q, _ = make_queries(seqs, 20, 600, [0, 3, 8, 12], 9302, thres=0.98)
    assert int(q.emac.max()) == 12
    dev = capi.Device(packed, clump_len, tot, lut)
    for all_hits in (True, False):
        exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        qf, hist = both(dev, q, exp, all_hits, capfd, monkeypatch)
        print(all_hits, qf, hist)
        assert qf[0][0] != "lds" and qf[2] == ("chunk", 0) and qf[3] == ("chunk", 0)
        assert hist["24"] + hist["16"] > 0 and hist["32"] + hist["40"] + hist["48"] > 0
    dev.close()


@pytest.fixture(scope="module")
def cs():
    return rl.build_cases()


@pytest.mark.parametrize("z", [1, 0])
def test_rescore_cases_under_both_settings(cs, z, capfd, monkeypatch):
    """rescorelib's constructed cases (width ladder, matrix edges, phase, ties) once more: every register set with the LDS form, the LDS
    band and the scratch variant unchanged beside them in the same launches"""
    from burst_amd import capi
    lut = ol.score_lut(z)
    dev = capi.Device(cs.packed, cs.clump_len, cs.tot, lut)
    # reads of up to 152 symbols (19 dwords): an LDS column in every register set.  The whole set has reads of 160: set 0 then has no room
    # for 20 dwords beside its seven waves per SIMD and keeps the dword form; the wider sets still take theirs from LDS
    short = [c for c in (cs.cases if z else cs.select("phase", "tie", "edge")) if len(c.q) <= 152]
    for key, cases in (("short", short), ("all", cs.cases))[:2 if z else 1]:
        batch = cs.batch(cases)
        qw = (max(len(s) for s in batch.seqs) + 7) // 8
        assert qw == (19 if key == "short" else 20)
        for all_hits in (True, False):
            exp = oracle_hits(cs.packed, cs.clump_len, cs.tot, batch, lut, all_hits)
            qf, hist = both(dev, batch, exp, all_hits, capfd, monkeypatch)
            print(z, key, all_hits, qf, hist)
            assert hist == rl.expected_histogram(exp, batch, cs, lut)
            assert qf[1:] == [("lds", qw * 256)] * 3 and qf[0] in ((("lds", qw * 256),) if key == "short" else (("lds", qw * 256), ("dword", 0)))
            assert not z or all(hist[str(w)] > 0 for w in rl.REG_LIMITS[:-1])
            if key == "all":
                assert hist["scratch"] > 0 and hist["48"] > 0
    dev.close()
