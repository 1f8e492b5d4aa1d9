"""Hand-made pile-ups the consensus tests share (pilecases.Hand on the pool's lane 0): the smallest shapes at which the segments and the
calling rules can go wrong.  Every scenario returns (Hand, check) where check(segments, letters) asserts on conslib's model of it -- the
callers compare the code under test with that model byte for byte.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import pilecases

MIN_DEPTH = 2      # of the calling-rule scenarios


def window(pool, n, lane=0, start=1, want=None):
    """the first 1-based column >= start of the lane from which n columns are all A/C/G/T (and the middle one holds code `want`)"""
    seq = np.asarray(pool.seqs[lane])
    for col in range(start, len(seq) - n + 2):
        w = seq[col - 1:col - 1 + n]
        if ((w >= 1) & (w <= 4)).all() and (want is None or int(w[n // 2]) == want):
            return col
    raise AssertionError("lane %d has no such window of %d columns" % (lane, n))


def letter_at(segs, letters, header, pos):
    for g in segs:
        if g["header"] == header and g["pos"] <= pos < g["pos"] + g["len"]:
            return letters[g["off"] + pos - g["pos"]]
    return None


def merge(hands):
    """several Hands (other headers, other offsets) as one: (queries, rows, ops, model)"""
    queries, rows, ops, model = [], [], [], []
    for h in hands:
        for r in h.rows:
            rows.append((r[0] + len(queries),) + tuple(r[1:7]) + (r[7] + len(ops),))
        queries += h.queries
        ops += h.ops
        model += h.model
    return queries, rows, ops, model


class Merged:
    def __init__(self, hands):
        self.queries, self.rows, self.ops, self.model = merge(hands)

    def q_arrays(self):
        off = np.zeros(len(self.queries) + 1, np.uint64)
        off[1:] = np.cumsum([len(q) for q in self.queries])
        return np.concatenate(self.queries).astype(np.uint8), off


# ---- segment shapes -------------------------------------------------------------------------------------------------------------------
def end_to_start(pool):
    h = pilecases.Hand(pool)
    h.exact(100, 10); h.exact(110, 10)
    return h, lambda s, l: _segs(s, [(77, 600, 20)])


def gap_of_one(pool):
    h = pilecases.Hand(pool)
    h.exact(100, 10); h.exact(111, 10)
    return h, lambda s, l: _segs(s, [(77, 600, 10), (77, 611, 10)])


def nested(pool):
    """a short line inside a long one that started earlier: the running maximum must not drop"""
    h = pilecases.Hand(pool)
    h.exact(100, 40); h.exact(105, 5); h.exact(138, 10)
    return h, lambda s, l: _segs(s, [(77, 600, 48)])


def only_the_first_reaches_the_third(pool):
    h = pilecases.Hand(pool)
    h.exact(100, 30); h.exact(102, 3); h.exact(130, 5)
    return h, lambda s, l: _segs(s, [(77, 600, 35)])


def header_boundary(pool):
    """header 77 with a line that ends at position 2^32 - 2, header 78 with a line that starts at position 1"""
    a = pilecases.Hand(pool, header=77, off=(1 << 32) - 1 - 12 - 50)      # column 50, 12 columns: pos + span = 2^32 - 1
    a.exact(50, 12)
    b = pilecases.Hand(pool, header=78, off=1 - 50)
    b.exact(50, 12)
    return Merged([a, b]), lambda s, l: _segs(s, [(77, (1 << 32) - 13, 12), (78, 1, 12)])


def single_symbol(pool):
    h = pilecases.Hand(pool)
    h.exact(100, 1)
    return h, lambda s, l: _segs(s, [(77, 600, 1)])


def insertions_at_both_ends(pool):
    seq = pool.seqs[0]
    h = pilecases.Hand(pool)
    h.add(200, np.concatenate([[2], seq[199:209], [3]]).astype(np.uint8), [(1, "I"), (10, "="), (1, "I")])
    return h, lambda s, l: _segs(s, [(77, 700, 10)]) and s[0]["ins_major"] == 0


def _segs(segs, want):
    assert [(g["header"], g["pos"], g["len"]) for g in segs] == want, segs
    return True


SHAPES = [end_to_start, gap_of_one, nested, only_the_first_reaches_the_third, header_boundary, single_symbol, insertions_at_both_ends]


# ---- calling rules: reads of 21 symbols whose middle column carries the case -------------------------------------------------------------
def _sub(h, col, code, w):
    """a read over columns col .. col + 20 that shows `code` in column col + 10"""
    q = np.array(h.pool.seqs[0][col - 1:col + 20], np.uint8)
    q[10] = code
    h.add(col, q, [(10, "="), (1, "X"), (10, "=")], w)


def _del(h, col, w):
    seq = h.pool.seqs[0]
    h.add(col, np.concatenate([seq[col - 1:col + 9], seq[col + 10:col + 20]]).astype(np.uint8), [(10, "="), (1, "D"), (10, "=")], w)


def _ins(h, col, w):
    """a symbol inserted behind column col + 10"""
    seq = h.pool.seqs[0]
    h.add(col, np.concatenate([seq[col - 1:col + 10], [1], seq[col + 10:col + 20]]).astype(np.uint8), [(11, "="), (1, "I"), (10, "=")], w)


def _rule(pool, build, want_letter, want, ref_code=None):
    col = window(pool, 21, want=ref_code)
    ref = int(pool.seqs[0][col + 9])
    h = pilecases.Hand(pool)
    build(h, col, ref)

    def check(segs, letters):
        assert len(segs) == 1 and segs[0]["len"] == 21
        assert letter_at(segs, letters, 77, 500 + col + 10) == (want_letter if want_letter else "ACGT"[ref - 1])
        assert {f: segs[0][f] for f in want} == want, segs
        return True
    return h, check


def tie_without_ref(pool):
    """A and C tie, Ref is G: the first in the order wins"""
    def build(h, col, ref):
        _sub(h, col, 1, 2); _sub(h, col, 2, 2); h.exact(col, 21, 1)
    return _rule(pool, build, "A", dict(called=21, same=20, subst=1, ins_major=0), ref_code=3)


def tie_with_ref(pool):
    def build(h, col, ref):
        _sub(h, col, ref % 4 + 1, 2); h.exact(col, 21, 2)
    return _rule(pool, build, None, dict(called=21, same=21, subst=0))


def del_majority(pool):
    def build(h, col, ref):
        _del(h, col, 3); h.exact(col, 21, 1)
    return _rule(pool, build, "-", {"called": 21, "same": 20, "del": 1})


def del_tied_with_ref(pool):
    def build(h, col, ref):
        _del(h, col, 2); h.exact(col, 21, 2)
    return _rule(pool, build, None, {"called": 21, "same": 21, "del": 0})


def other_never_wins(pool):
    """five reads show N, one shows the reference: Other is part of Depth and never wins"""
    def build(h, col, ref):
        _sub(h, col, 5, 5); h.exact(col, 21, 1)
    return _rule(pool, build, None, dict(called=21, same=21, subst=0))


def ins_half_is_not_a_majority(pool):
    def build(h, col, ref):
        _ins(h, col, 2); h.exact(col, 21, 2)      # 2 * Ins == Depth
    return _rule(pool, build, None, dict(called=21, same=21, ins_major=0))


def ins_majority(pool):
    def build(h, col, ref):
        _ins(h, col, 3); h.exact(col, 21, 2)      # 2 * Ins == Depth + 1
    return _rule(pool, build, None, dict(called=21, same=21, ins_major=1))


def under_min_depth(pool):
    """one read of weight 1 beside the pile: its own columns stay N inside the segment"""
    def build(h, col, ref):
        h.exact(col, 21, 2); h.exact(col + 21, 5, 1)
    col = window(pool, 26)
    h = pilecases.Hand(pool)
    build(h, col, 0)

    def check(segs, letters):
        assert len(segs) == 1 and segs[0]["len"] == 26 and segs[0]["called"] == 21 and letters[21:26] == "NNNNN" and "N" not in letters[:21]
        return True
    return h, check


RULES = [tie_without_ref, tie_with_ref, del_majority, del_tied_with_ref, other_never_wins, ins_half_is_not_a_majority, ins_majority, under_min_depth]
