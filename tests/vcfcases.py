"""The inputs the VCF tests share: hand-made lines on pilecases.Hand for every rule of the allele definition, a planted pile-up, and the
model's rows as the library's arrays.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import pilecases
import pilelib
import vcflib


def expect(model_lines, min_depth=1, min_alt=1):
    """(rows of vcflib.returned, figures dict with `distinct` added) of the lines"""
    table, fig = vcflib.alleles(model_lines)
    rows = vcflib.returned(table, pilelib.pile(model_lines), min_depth, min_alt)
    return rows, dict(fig, distinct=len(table))


def arrays_of(rows):
    """the model's rows as (capi.ALLELE_DTYPE array, codes uint8): what bhip_alleles_run and bh_alleles_host return"""
    from burst_amd import capi
    a, codes = np.zeros(len(rows), capi.ALLELE_DTYPE), []
    for k, (h, p, ref, depth, count, kind, n, ins, deleted) in enumerate(rows):
        a[k] = (h, p, vcflib.word(kind, n, ins), ref, depth, count, 0, len(codes))      # (code_off: the running sum, also for an Ins, which owns no codes)
        codes += list(deleted)
    return a, np.array(codes, np.uint8)


def same(got, got_codes, rows):
    exp, exp_codes = arrays_of(rows)
    assert len(got) == len(exp), (len(got), len(exp))
    assert got.tobytes() == exp.tobytes(), next((g, e) for g, e in zip(got, exp) if g != e)
    assert np.asarray(got_codes, np.uint8).tobytes() == exp_codes.tobytes()


def info_matches(info, fig, n_rows):
    """info: events, distinct, returned, skipped end / adjacent / long (a sequence or capi's dict)"""
    if isinstance(info, dict):
        info = [info[k] for k in ("events", "distinct", "alleles", "skipped_end", "skipped_adjacent", "skipped_long")]
    assert [int(x) for x in info[:6]] == [fig["events"], fig["distinct"], n_rows, fig["end"], fig["adjacent"], fig["long"]], (list(info[:6]), fig, n_rows)


# ---- hand-made lines ---------------------------------------------------------------------------------------------------------------------
def put(h, col, parts, w=1):
    """a line of Hand h that starts at 1-based lane column col.  parts: ("=", n) copies the lane, ("X", n) another base per column, ("I", codes)
    inserts the codes, ("D", n) skips n columns"""
    seq, q, ops, c = h.pool.seqs[h.lane], [], [], col - 1
    for op, v in parts:
        if op == "I":
            q += list(v)
            ops.append((len(v), "I"))
            continue
        if op == "=":
            q += [int(x) for x in seq[c:c + v]]
        elif op == "X":
            q += [int(x) % 4 + 1 for x in seq[c:c + v]]
        ops.append((v, op))
        c += v
    h.add(col, np.array(q, np.uint8), ops, w)


def scenarios(pool):
    """[(name, Hand, check(rows, fig))]: every rule of the definition on lines written by hand (lane 0, header 77, positions 500 + column)"""
    out = []

    def case(name, check):
        h = pilecases.Hand(pool)
        out.append((name, h, check))
        return h

    ins15, ins16 = [1 + t % 4 for t in range(15)], [1 + t % 4 for t in range(16)]

    def chk(rows, fig):
        assert len(rows) == 1 and rows[0][5:8] == (vcflib.INS, 15, tuple(ins15)) and rows[0][1] == 500 + 119 and fig["long"] == 1 and fig["events"] == 1
    h = case("an insertion of 15 symbols is an allele, one of 16 is long", chk)
    put(h, 100, [("=", 20), ("I", ins15), ("=", 20)])
    put(h, 100, [("=", 20), ("I", ins16), ("=", 20)])

    def chk(rows, fig):
        assert [(r[1], r[5], r[7], r[4]) for r in rows] == [(619, vcflib.INS, (1, 2), 2), (619, vcflib.INS, (2, 1), 3), (619, vcflib.INS, (1, 1, 1), 1)]
    h = case("two insertions of equal length on one anchor, a longer one behind them", chk)
    put(h, 100, [("=", 20), ("I", [2, 1]), ("=", 20)], w=3)
    put(h, 100, [("=", 20), ("I", [1, 1, 1]), ("=", 20)])
    put(h, 105, [("=", 15), ("I", [1, 2]), ("=", 20)], w=2)

    def chk(rows, fig):
        assert [(r[1], r[5], r[6], r[4], len(r[8])) for r in rows] == [(619, vcflib.DEL, 1, 2, 1), (619, vcflib.DEL, 3, 5, 3), (619, vcflib.INS, 1, 1, 0)]
    h = case("Del(1) and Del(3) on one anchor, before an insertion there", chk)
    put(h, 100, [("=", 20), ("D", 3), ("=", 20)], w=5)
    put(h, 100, [("=", 20), ("I", [4]), ("=", 20)])
    put(h, 110, [("=", 10), ("D", 1), ("=", 20)], w=2)

    def chk(rows, fig):
        assert len(rows) == 1 and rows[0][4] == 2 and rows[0][3] == 2 and fig["events"] == 2 and fig["distinct"] == 1
    h = case("the same insertion from two query entries (a forward line, a reverse line's reverse-complement entry) is one allele", chk)
    put(h, 200, [("=", 30), ("I", [3, 3]), ("=", 12)])
    put(h, 215, [("=", 15), ("I", [3, 3]), ("=", 30)])

    def chk(rows, fig):
        assert [(r[1], r[5]) for r in rows] == [(500 + 309, vcflib.INS), (500 + 409, vcflib.DEL), (500 + 459, vcflib.INS)] and fig["adjacent"] == 2 and fig["events"] == 3
    h = case("an indel behind X is an allele, one behind the other indel kind is adjacent", chk)
    put(h, 300, [("=", 9), ("X", 1), ("I", [1, 1]), ("=", 10)])
    put(h, 400, [("=", 10), ("D", 1), ("I", [2]), ("=", 20)])
    put(h, 450, [("=", 10), ("I", [2, 4]), ("D", 2), ("=", 20)])

    def chk(rows, fig):
        assert rows == [] and fig["end"] == 4 and fig["events"] == 0
    h = case("an indel as the first op and as the last op", chk)
    put(h, 600, [("I", [1]), ("=", 31)])
    put(h, 600, [("=", 31), ("I", [2, 2])])
    put(h, 600, [("D", 2), ("=", 20)])
    put(h, 600, [("=", 20), ("D", 1)])

    def chk(rows, fig):
        assert len(rows) == 1 and rows[0][3] == 2 + 3 + 5 + 7 and rows[0][4] == 2 and rows[0][1] == 500 + 299
    h = case("an anchor whose other observers are plain: the depth is the stabbing count; mixed weights", chk)
    put(h, 280, [("=", 20), ("D", 2), ("=", 20)], w=2)
    h.exact(299, 25, w=3)      # begins at the anchor
    h.exact(270, 30, w=5)      # ends at the anchor
    h.exact(260, 80, w=7)      # covers it
    h.exact(270, 29, w=11)     # ends before it
    h.exact(300, 25, w=13)     # begins behind it

    def chk(rows, fig):
        assert len(rows) == 1 and rows[0][7] == (5, 6, 1)
    h = case("an inserted code outside A/C/G/T stays a code (the file prints N)", chk)
    put(h, 500, [("=", 20), ("I", [5, 6, 1]), ("=", 20)])
    return out


def planted_del(pool, n_lines, k, n_del=2):
    """n_lines reads of 33 columns share a window of lane 0; k of them delete the n_del columns behind column 120"""
    h = pilecases.Hand(pool)
    for i in range(n_lines):
        col = 115 - (i % 20)      # every read covers columns 115 .. 127
        if i < k:
            put(h, col, [("=", 121 - col), ("D", n_del), ("=", 33 - (121 - col) - n_del)])
        else:
            h.exact(col, 33)
    return h


def check_planted_del(rows, n_lines, k, want, n_del=2):
    assert len(rows) == want, (n_lines, k)
    if want:
        assert rows[0][:2] == (77, 620) and rows[0][3:7] == (n_lines, k, vcflib.DEL, n_del)
