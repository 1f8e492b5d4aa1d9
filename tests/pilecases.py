"""The inputs the variants tests share: cigarlib's pool of lanes, query entries and expected paths turned into lines of a pile-up -- every
lane on a header at an offset, two lanes of one clump on ONE header at offsets that overlap -- once as the library's arrays and once as
pilelib's plain lines.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import cigarlib as cg
import dbutil
import oraclelib as ol

OP_CHAR = {1: "I", 2: "D", 7: "=", 8: "X"}


def span_of(ops):
    return sum(int(w) >> 4 for w in ops if int(w) & 15 != 1)


def find_shared(seqs, cases, lanes):
    """(A, B, d, n): lanes A < B and a shift d (column x of A = column x - d of B) such that the columns observed by lines of BOTH lanes
    are as many as possible (n >= 1) while the two lanes hold the same code on every one of them -- lanes that share positions of a header
    are cuts of one sequence.  None when there is no such pair."""
    cov = {}
    for c in cases:
        a = cov.setdefault(c["refIx"], np.zeros(len(seqs[c["refIx"]]) + 64, bool))
        a[c["ref_first"] - 1:c["ref_first"] - 1 + span_of(c["ops"])] = True
    best = None
    for A in lanes:
        for B in lanes:
            if A >= B or A not in cov or B not in cov:
                continue
            sa, sb = np.asarray(seqs[A]), np.asarray(seqs[B])
            ca, cb = cov[A][:len(sa)], cov[B][:len(sb)]
            for d in range(-(len(sb) - 1), len(sa)):
                lo, hi = max(0, d), min(len(sa), d + len(sb))
                both = ca[lo:hi] & cb[lo - d:hi - d]
                n = int(both.sum())
                if n and (best is None or n > best[3]) and np.array_equal(sa[lo:hi][both], sb[lo - d:hi - d][both]):
                    best = (A, B, d, n)
    return best


class PileCases:
    def __init__(self, L, z=1, iupac_only=False):
        self.lut = ol.score_lut(z)
        self.seqs, self.queries, self.rcs, self.cases = cg.build_pool(L, self.lut, iupac_only=iupac_only)
        self.packed, self.clump_len, self.tot = dbutil.pack_clumps(self.seqs)
        n = len(self.seqs)
        # every lane on a header of its own at an offset of its own ...
        self.header = [3 * k + 1 for k in range(n)]
        self.off = [7 * k + (100000 if k == 5 else 0) for k in range(n)]
        # ... but for two lanes of the second clump, which share one header at offsets that overlap
        self.shared = None if iupac_only else find_shared(self.seqs, self.cases, range(16, n))
        if self.shared:
            A, B, d, _ = self.shared
            self.header[B] = self.header[A]
            self.off[B] = self.off[A] + d + 2000      # (a lane may lie left of its partner: keep every position >= 1)
            self.off[A] += 2000
        self.q_off = np.zeros(len(self.queries) + 1, np.uint64)
        self.q_off[1:] = np.cumsum([len(q) for q in self.queries])
        self.q_codes = np.concatenate(self.queries).astype(np.uint8)

    def weight(self, i):
        return 1 + (5 * i) % 4      # mixed weights, 1 .. 4

    def arrays(self, idx, weights=None):
        """(PILE_LINE_DTYPE lines, ops) of the cases idx"""
        from burst_amd import capi
        lines = np.zeros(len(idx), capi.PILE_LINE_DTYPE)
        ops, at = [], 0
        for k, i in enumerate(idx):
            c = self.cases[i]
            lines[k] = (c["q"], c["refIx"], c["ref_first"], self.header[c["refIx"]], self.off[c["refIx"]] + c["ref_first"],
                        self.weight(i) if weights is None else weights[k], len(c["ops"]), at)
            ops.append(c["ops"])
            at += len(c["ops"])
        return lines, (np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32))

    def before_paths(self, idx):
        """(header, position in front of the path) of the cases idx"""
        return {(self.header[self.cases[i]["refIx"]], self.off[self.cases[i]["refIx"]] + self.cases[i]["ref_first"] - 1) for i in idx}

    def lane_ref(self, lane):
        seq, off = self.seqs[lane], self.off[lane]
        return lambda p: int(seq[p - off - 1]) if 0 <= p - off - 1 < len(seq) else 0

    def model_lines(self, idx, weights=None):
        """the same lines for pilelib"""
        out = []
        for k, i in enumerate(idx):
            c = self.cases[i]
            out.append(dict(header=self.header[c["refIx"]], pos=self.off[c["refIx"]] + c["ref_first"],
                            ops=[(int(w) >> 4, OP_CHAR[int(w) & 15]) for w in c["ops"]], query=self.queries[c["q"]],
                            ref=self.lane_ref(c["refIx"]), w=self.weight(i) if weights is None else weights[k]))
        return out


def rows_of(sites):
    """library sites (capi.PILE_SITE_DTYPE) as pilelib's rows"""
    return [(int(s["header"]), int(s["pos"]), int(s["ref"]), int(s["depth"])) + tuple(int(x) for x in s["n"]) + (int(s["ins"]),) for s in sites]


# ---- hand-made lines on the pool's lanes ---------------------------------------------------------------------------------------------
class Hand:
    """lines written by hand: reads of lane `lane` of a PileCases pool with their own query entries.  rows / ops: what the library takes
    (rows of capi.PILE_LINE_DTYPE), model: the same lines for pilelib"""
    def __init__(self, pool, lane=0, header=77, off=500):
        self.pool, self.lane, self.header, self.off = pool, lane, header, off
        self.queries, self.rows, self.ops, self.model = [], [], [], []

    def add(self, col, query, ops, w=1):
        """a path that starts at 1-based lane column col; ops = [(n, op char)]"""
        code = {"I": 1, "D": 2, "=": 7, "X": 8}
        self.queries.append(np.asarray(query, np.uint8))
        self.rows.append((len(self.queries) - 1, self.lane, col, self.header, self.off + col, w, len(ops), len(self.ops)))
        self.ops += [n << 4 | code[c] for n, c in ops]
        self.model.append(dict(header=self.header, pos=self.off + col, ops=ops, query=self.queries[-1], ref=self.ref, w=w))

    def ref(self, p):
        seq = self.pool.seqs[self.lane]
        return int(seq[p - self.off - 1]) if 0 <= p - self.off - 1 < len(seq) else 0

    def exact(self, col, m, w=1):
        self.add(col, self.pool.seqs[self.lane][col - 1:col - 1 + m], [(m, "=")], w)

    def q_arrays(self):
        off = np.zeros(len(self.queries) + 1, np.uint64)
        off[1:] = np.cumsum([len(q) for q in self.queries])
        return np.concatenate(self.queries).astype(np.uint8), off


def planted_cases(min_depth, min_alt):
    """(lines, lines that carry the substitution, sites expected): k and the line count either side of their thresholds"""
    return [(40, min_alt - 1, 0), (40, min_alt, 1), (min_depth - 1, min_alt, 0), (min_depth, min_alt, 1)]


def planted(pool, n_lines, k):
    """n_lines exact reads of 33 symbols share a window of lane 0; k of them carry the same substitution in column 120"""
    seq = pool.seqs[0]
    h = Hand(pool)
    for i in range(n_lines):
        col = 120 - (i % 30)      # every read covers column 120
        if i < k:
            q = np.array(seq[col - 1:col + 32], np.uint8)
            q[120 - col] = q[120 - col] % 4 + 1
            h.add(col, q, [(n, c) for n, c in ((120 - col, "="), (1, "X"), (32 - (120 - col), "=")) if n])
        else:
            h.exact(col, 33)
    return h


def check_planted(rows, n_lines, k, want):
    assert len(rows) == want, (n_lines, k)
    if want:
        r = rows[0]
        assert (r[0], r[1], r[3]) == (77, 500 + 120, n_lines) and r[3] - r[4 + r[2] - 1] == k and r[10] == 0


def boundaries(pool):
    """one line is not plain at column p = 300; plain lines begin at p, end at p, end at p - 1 and begin at p + 1"""
    seq = pool.seqs[0]
    h = Hand(pool)
    q = np.array(seq[279:320], np.uint8)      # columns 280 .. 320
    q[20] = q[20] % 4 + 1
    h.add(280, q, [(20, "="), (1, "X"), (20, "=")], w=3)
    h.exact(300, 25, w=5)      # begins exactly at p
    h.exact(270, 31, w=7)      # ends exactly at p
    h.exact(270, 30, w=11)     # ends at p - 1
    h.exact(301, 25, w=13)     # begins at p + 1
    return h


def check_boundaries(rows):
    assert len(rows) == 1 and rows[0][1] == 800 and rows[0][3] == 3 + 5 + 7


def insertions(pool):
    seq = pool.seqs[0]
    ins = lambda a, at, sym: np.concatenate([a[:at], [sym], a[at:]]).astype(np.uint8)
    h = Hand(pool)
    # an interior run whose anchor column is itself an X: columns 400 .. 419, X at 409, the run behind it
    q = np.array(seq[399:419], np.uint8)
    q[9] = q[9] % 4 + 1
    h.add(400, ins(q, 10, 1), [(9, "="), (1, "X"), (1, "I"), (10, "=")], w=2)
    h.exact(395, 33, w=3)
    # a path that begins with I and one that ends with I: neither is counted
    h.add(600, ins(np.array(seq[599:630], np.uint8), 0, 2), [(1, "I"), (31, "=")])
    h.add(600, ins(np.array(seq[599:630], np.uint8), 31, 2), [(31, "="), (1, "I")])
    # a run behind a deletion
    h.add(700, ins(np.concatenate([seq[699:709], seq[710:730]]).astype(np.uint8), 10, 3), [(10, "="), (1, "D"), (1, "I"), (20, "=")], w=4)
    return h


def check_insertions(rows):
    by = {r[1]: r for r in rows}
    assert sorted(by) == [500 + 409, 500 + 710] and by[909][10] == 2 and by[909][3] == 5 and by[1210][10] == 4 and by[1210][8] == 4
