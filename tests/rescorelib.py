"""Constructed inputs for the re-scorer (k_rescore_classify, k_rescore_reg<0..3>, k_rescore<false / true>) and a plain
definition of the band a hit is re-scored in.  TEST INFRASTRUCTURE ONLY, no GPU code.

A raw hit goes to a re-scoring variant by ONE number, its band width Wd = min(e_last, L) - e_first + 2 * ed + 1, where
e_first / e_last are the first / last end column of the last row that attains the lane's edit distance ed.  last_row() states
that last row in numpy, bucket() the classification, expected_histogram() what the library's BHIP_DEBUG line
"re-scorer bands ..." must print for a set of oracle records, and build_cases() a small database with named reads that
aim at every width limit, matrix edge, register-window phase and tie of the re-scorer.  What a case actually is (its ed,
its band) is never taken from the builder's intention: the DP says."""
import numpy as np

SEED = 20261019
REG_LIMITS = (4, 6, 8, 12, 16, 24, 32, 40, 48)              # upper band widths of the nine register variants
WIDTHS = (3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49)
BUCKETS = tuple(str(w) for w in REG_LIMITS) + ("lds", "scratch")
RESCORE_WMAX = 48                                           # BHIP_RESCORE_WMAX
_BIG = 1 << 13                                              # "never" in the int16 matrix of last_rows (queries and lanes of < 8 192 symbols)


# ---------------------------------------------------------------------------------------------------------------------
# the band, in plain integers
# ---------------------------------------------------------------------------------------------------------------------
def last_rows(qs, lane, lut, L):
    """last_row() for several queries against one lane at once: int32[len(qs), L] (row y = len(q) of each query's matrix)"""
    lut2 = np.asarray(lut, np.uint8).reshape(16, 16)
    ref = np.zeros(L, np.uint8)
    ref[:len(lane)] = lane                                   # the lane, padded to the clump's length with code 0
    costs = np.where(lut2[:, ref] == 0, 0, 1).astype(np.int16)      # [query symbol, column]: 0 where the table says match, else 1
    costs[0] = _BIG                                          # (a query symbol of code 0 never takes the diagonal)
    lens = np.array([len(q) for q in qs])
    order = np.argsort(-lens, kind="stable")                 # longest first: the finished queries fall off the end
    R, M = len(qs), int(lens.max())
    Q = np.zeros((R, M), np.uint8)
    for i, k in enumerate(order):
        Q[i, :lens[k]] = qs[k]
    slen = lens[order]
    j = np.arange(L + 1, dtype=np.int16)
    prev = np.zeros((R, L + 1), np.int16)                    # row 0: a free start in every column
    out = np.zeros((R, L), np.int32)
    for y in range(1, M + 1):
        n = int(np.searchsorted(-slen, -y, side="right"))    # queries of at least y symbols
        prev = prev[:n]
        c = np.empty_like(prev)
        c[:, 0] = y                                          # column 0
        np.minimum(prev[:, :-1] + costs[Q[:n, y - 1]], prev[:, 1:] + 1, out=c[:, 1:])
        c -= j
        np.minimum.accumulate(c, axis=1, out=c)              # the left dependency: c[x] = min over x' <= x of c[x'] + (x - x')
        c += j
        done = slen[:n] == y
        if done.any():
            out[order[:n][done]] = c[done, 1:]
        prev = c
    return out


def last_row(q, lane, lut, L):
    """The unit-cost semi-global matrix of query q against one reference lane, as the SWEEP kernels see it: row 0 is zero,
    column 0 is i, a cell costs 0 where lut says match and 1 otherwise.  Returns (last row over columns 1..L, ed = its minimum,
    e_first, e_last = first / last 1-based column attaining it); L is the CLUMP's length, the lane is padded to it with code 0.

    Pad rule, from the sweeps (k_myers and the window kernels): a pad column has no bit in any query symbol's match mask, so it
    counts as an ordinary mismatch (cost 1) -- not the 255 of the score table that the re-scorer applies.  That cannot lower the
    minimum (a path through k pad columns costs at least the k insertions that end at the lane's last symbol instead), but the
    LAST best column may lie in the pads: BhipRawHit::e_last "may run into trailing pad columns", and the band then covers
    columns the re-scorer treats as invalid.  Columns beyond L (the filler of the last 32-symbol chunk) are cut by
    min(e_last, L).  A QUERY symbol of code 0 is not swept at all: the sweeps run on the query without it and add one edit, which
    equals a row that can only be entered from above (cost 1) -- the cost here is "never diagonal" for such a row."""
    row = last_rows([np.asarray(q, np.uint8)], lane, lut, L)[0]
    ed = int(row.min())
    at = np.flatnonzero(row == ed)
    return row, ed, int(at[0]) + 1, int(at[-1]) + 1


def band_width(ed, e_first, e_last, L):
    return min(e_last, L) - e_first + 2 * ed + 1


def band_rows_of(max_emac):
    """the LDS plan's band rows of a batch (plan_batch): min(48, 2 * maxE + 10)"""
    return min(RESCORE_WMAX, 2 * int(max_emac) + 10)


def bucket(Wd, band_rows, use_reg=True):
    """k_rescore_classify: the narrowest register variant that holds the band (option rescore_reg), else the LDS band while the
    band fits band_rows, else the global-scratch variant.  One of BUCKETS."""
    if use_reg:
        for lim in REG_LIMITS:
            if Wd <= lim:
                return str(lim)
    return "lds" if Wd <= band_rows else "scratch"


def rescore_cells(q, r, B, lut, rule="ref"):
    """The re-scorer's three planes cell by cell in plain Python (the reference's reScoreM, burst.c:713-886, as orc_rescore_lane restates
    it): a cell takes the predecessor with the lowest score, then the larger gapQ, then diagonal before up before left; row 1 takes the
    substitution cost alone.  Returns (ed, gapQ, gapR, finalPos).  rule = "uptie" ranks up and left equal, so that the lower gapR decides
    between them: where that changes the result, the up-before-left priority is what the record rests on.  Slow: for short reads."""
    lut = np.asarray(lut).reshape(16, 16).tolist()
    q, r = [int(x) for x in q], [int(x) for x in r]
    m, n, inf = len(q), len(r), 1 << 20
    pr = (0, 1, 2) if rule == "ref" else (0, 1, 1)
    prev = [(1, 0, 0, 1)]                                    # a cell: (score, -gapQ, priority of the move taken, gapR); column 0 of row 1
    for x in range(1, n + 1):
        s = lut[q[0]][r[x - 1]]
        prev.append((s if s <= B else inf, -1 if s == 1 and prev[x - 1][0] == 0 else 0, 0, 0))
    for y in range(2, m + 1):
        cur = [(y if y <= B else inf, 0, 0, y)]
        row = lut[q[y - 1]]
        for x in range(1, n + 1):
            d, u, l = prev[x - 1], prev[x], cur[x - 1]
            c = min((d[0] + row[r[x - 1]], d[1], pr[0], d[3]), (u[0] + 1, u[1], pr[1], u[3] + 1), (l[0] + 1, l[1] - 1, pr[2], l[3]))
            cur.append(c if c[0] <= B else (inf, 0, 0, 0))
        prev = cur
    keys = [(prev[x][0], prev[x][1]) for x in range(1, n + 1)]
    best = min(keys)
    at = [x for x in range(1, n + 1) if keys[x - 1] == best]
    return best[0], -best[1], prev[at[0]][3], at[-1]


class Batch:
    """a flat query batch with the attributes of burst_amd.capi.Queries (which the oracle and the device calls read)"""

    def __init__(self, seqs, emac, six=None):
        self.seqs = [np.asarray(s, np.uint8) for s in seqs]
        n = len(seqs)
        self.off = np.zeros(n + 1, np.uint64)
        np.cumsum([len(s) for s in seqs], out=self.off[1:])
        self.codes = np.concatenate(self.seqs)
        self.emac = np.ascontiguousarray(emac, np.uint16)
        self.six = np.ascontiguousarray(np.arange(n) if six is None else six, np.uint32)
        self.rc = np.zeros(n, np.uint8)
        self.flags = None
        self.n = n
        self.n_shared = int(self.six.max()) + 1


def record_bands(records, batch, db, lut):
    """per oracle record: (ed, e_first, e_last clamped to L, Wd, dlo) from the DP; asserts the DP's ed is the record's"""
    out = np.zeros(len(records), np.dtype([("ed", "i4"), ("e_first", "i4"), ("e_last", "i4"), ("Wd", "i4"), ("dlo", "i4")]))
    refs = np.asarray(records["refIx"])
    for r in np.unique(refs):
        idx = np.flatnonzero(refs == r)
        L = int(db.clump_len[r >> 4])
        rows = last_rows([batch.seqs[int(q)] for q in records["q"][idx]], db.seqs[int(r)], lut, L)
        ed = rows.min(axis=1)
        best = rows == ed[:, None]
        e1 = best.argmax(axis=1) + 1
        e2 = L - best[:, ::-1].argmax(axis=1)
        m = np.array([len(batch.seqs[int(q)]) for q in records["q"][idx]])
        assert np.array_equal(ed, records["ed"][idx]), ("DP and oracle disagree on ed", int(r))
        out["ed"][idx] = ed; out["e_first"][idx] = e1; out["e_last"][idx] = e2
        out["Wd"][idx] = e2 - e1 + 2 * ed + 1
        out["dlo"][idx] = e1 - m - ed
    return out


def expected_histogram(records, batch, db, lut, band_rows=None, use_reg=True):
    """hits per re-scoring variant for the oracle's records: one record is one raw hit that passed the filter; exact matches
    (ed 0) leave in the classifier and are not counted.  {bucket name: count} over BUCKETS."""
    if band_rows is None:
        band_rows = band_rows_of(batch.emac.max())
    hist = {b: 0 for b in BUCKETS}
    bands = record_bands(records, batch, db, lut)
    for w in bands["Wd"][bands["ed"] > 0]:
        hist[bucket(int(w), band_rows, use_reg)] += 1
    return hist


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, q, emac, target, want=None):
        self.name, self.family, self.q, self.emac, self.target, self.want = name, family, np.asarray(q, np.uint8), int(emac), int(target), want


class Lane:
    def __init__(self, seq, kind, stretch=None, codes=None):
        self.seq, self.kind, self.stretch, self.codes = seq, kind, stretch, codes      # stretch = (start, length, unit), codes = positions of IUPAC codes


CLUMP_LENS = (256, 257, 287, 340)       # a chunk boundary and one symbol either side of one; the last clump is the longest
_KINDS16 = ("longest", "rand", "short", "hp", "tr", "iupac1", "iupacrun", "hp_start", "tr_end", "rand", "hp_long", "short", "tr", "hp", "rand", "short")
_KINDS_LAST = ("longest", "len256", "len257", "len287", "hp", "tr", "iupacrun", "hp_long", "rand", "short")


def _other(s, rng):
    s = int(s)
    return (s + int(rng.integers(0, 3))) % 4 + 1 if 1 <= s <= 4 else int(rng.integers(1, 5))


def _rand(rng, n):
    return rng.integers(1, 5, size=n, dtype=np.uint8)


def _spread(m, n, rng, lo=3, hi=None):
    """n positions spread over [lo, hi) of a read, one per equal part with a jitter of one"""
    hi = m - 3 if hi is None else hi
    step = (hi - lo) / max(n, 1)
    return sorted({min(hi - 1, max(lo, int(lo + (k + 0.5) * step + rng.integers(-1, 2)))) for k in range(n)})


class CaseSet:
    def __init__(self, lut):
        import dbutil
        self.lut = lut
        self.rng = np.random.default_rng(SEED)
        self.lanes = []
        self._build_db()
        self.seqs = [ln.seq for ln in self.lanes]
        self.packed, self.clump_len, self.tot = dbutil.pack_clumps(self.seqs)
        assert tuple(int(x) for x in self.clump_len) == CLUMP_LENS
        self.cases = []
        self._ladders()
        self._edges()
        self._phase()
        self._ties()
        self._ties_early()
        self.long_read = _rand(self.rng, 452)               # plan_batch: (band_rows + 1 + qw + rw) * 256 > 40 KB with band_rows = 48

    # ---- database -------------------------------------------------------------------------------------------------
    def _build_db(self):
        rng = self.rng
        for c, CL in enumerate(CLUMP_LENS):
            kinds = _KINDS16 if c < 3 else _KINDS_LAST
            for z, kind in enumerate(kinds):
                n = CL if kind == "longest" else int(kind[3:]) if kind.startswith("len") else \
                    CL - int(rng.integers(40, min(90, CL - 200) + 1)) if kind == "short" else int(rng.integers(max(200, CL - 30), CL))
                s = _rand(rng, n)
                stretch = codes = None
                if kind in ("hp", "hp_start", "hp_long"):
                    k = 120 if kind == "hp_long" else int(rng.integers(20, 61))
                    a = 0 if kind == "hp_start" else int(rng.integers(30, n - k - 30))
                    sym = 1 + (c + z) % 4
                    s[a:a + k] = sym
                    stretch = (a, k, np.array([sym], np.uint8))
                elif kind in ("tr", "tr_end"):
                    ul = 2 + (c + z) % 4                      # units of 2 - 5 symbols
                    unit = _rand(rng, ul)
                    while len(set(unit.tolist())) == 1:
                        unit = _rand(rng, ul)
                    reps = int(rng.integers(5, 12))
                    a = n - ul * reps if kind == "tr_end" else int(rng.integers(30, n - ul * reps - 30))
                    s[a:a + ul * reps] = np.tile(unit, reps)
                    stretch = (a, ul * reps, unit)
                if stretch is not None:                      # the symbols beside a stretch do not continue it
                    a, k, unit = stretch
                    if a > 0:
                        s[a - 1] = _other(unit[-1], rng) if s[a - 1] == unit[-1] else s[a - 1]
                    if a + k < n:
                        s[a + k] = _other(unit[0], rng) if s[a + k] == unit[0] else s[a + k]
                if kind == "iupac1":
                    p = int(rng.integers(100, n - 100))
                    s[p] = 8                                 # R = A or G
                    codes = [p]
                elif kind == "iupacrun":
                    p = int(rng.integers(100, n - 100))
                    s[p:p + 6] = [5, 9, 12, 5, 7, 15]         # N Y B N M D
                    codes = list(range(p, p + 6))
                self.lanes.append(Lane(s, kind, stretch, codes))

    def L_of(self, r):
        return CLUMP_LENS[r >> 4]

    def of_kind(self, *kinds):
        return [r for r, ln in enumerate(self.lanes) if ln.kind in kinds]

    def measure(self, q, r):
        _, ed, e1, e2 = last_row(q, self.lanes[r].seq, self.lut, self.L_of(r))
        return ed, band_width(ed, e1, e2, self.L_of(r))

    def _aim(self, name, family, r, want, make, slack=0, tries=8, keep_exact=True):
        """make(t) -> read, tried until the DP gives the wanted band width on lane r; the closest attempt is kept"""
        best = None
        for t in range(tries):
            q = make(t)
            ed, Wd = self.measure(q, r)
            if best is None or (want is not None and abs(Wd - want) < abs(best[2] - want)):
                best = (q, ed, Wd)
            if want is None or Wd == want:
                break
        q, ed, Wd = best
        if ed == 0 and not keep_exact:
            return
        self.cases.append(Case(name, family, q, ed + slack, r, want))

    def _subs_read(self, r, start, m, n_sub, last_sub=False, fixed=()):
        """lane r's symbols [start, start + m) with n_sub substitutions: those at the read offsets `fixed`, one at the final symbol
        if last_sub, the rest spread over the read"""
        rng = self.rng
        q = self.lanes[r].seq[start:start + m].copy()
        pos = set(fixed)
        if last_sub and len(pos) < n_sub:
            pos.add(m - 1)
        free = n_sub - len(pos)
        if free > 0:
            pos |= set(_spread(m, free, rng, lo=4, hi=m - 4))
        for p in pos:
            q[p] = _other(q[p], rng)
        return q

    # ---- 1. width ladder --------------------------------------------------------------------------------------------
    def _ladders(self):
        rng = self.rng
        plain = self.of_kind("rand", "longest")
        for i, W in enumerate(WIDTHS):                       # by edits: (W - 1) // 2 substitutions, even widths end in one (span 1)
            ed, even = (W - 1) // 2, W % 2 == 0
            r = plain[i % len(plain)]
            n = len(self.lanes[r].seq)

            def make(t, r=r, n=n, ed=ed, even=even):
                m = min(160, 64 + 4 * ed + int(rng.integers(0, 9)))
                return self._subs_read(r, int(rng.integers(20, n - m - 20)), m, ed, last_sub=even)
            self._aim("ladder_edits/W%d" % W, "ladder_edits", r, W, make, slack=i & 1)
        longs = self.of_kind("hp_long")
        for i, W in enumerate(WIDTHS):                       # by span: one substitution in a homopolymer read against a longer homopolymer
            r = longs[i % len(longs)]
            a, H, unit = self.lanes[r].stretch

            def make(t, H=H, unit=unit, W=W):
                m = H - W + 4 + (0, 1, -1, 2, -2, 3, -3, 4)[t]
                q = np.full(m, unit[0], np.uint8)
                q[m // 2] = _other(unit[0], rng)
                return q
            self._aim("ladder_span/W%d" % W, "ladder_span", r, W, make, slack=i & 1)

    # ---- 2. matrix edges per width ------------------------------------------------------------------------------------
    def edge_lanes(self):
        """(lane, tag): every clump's longest lane (z = 0; clump lengths 256, 257, 287, 340), a short lane with pads behind it
        (z = 15 where the clump has one) and the lanes of 256 / 257 / 287 symbols inside the longest clump"""
        out = []
        for c in range(4):
            out.append((16 * c, "longest"))
            out.append((16 * c + (15 if c < 3 else 9), "short"))
        out += [(r, self.lanes[r].kind) for r in self.of_kind("len256", "len257", "len287")]
        return out

    def _edges(self):
        rng = self.rng
        for W in WIDTHS:
            ed, even = (W - 1) // 2, W % 2 == 0
            for r, tag in self.edge_lanes():
                n = len(self.lanes[r].seq)
                seq = self.lanes[r].seq
                base = "W%d/c%dz%d_%s" % (W, r >> 4, r & 15, tag)

                def m_of():
                    return min(160, 64 + 4 * ed + int(rng.integers(0, 9)))

                def start_sub(t):                            # the read starts at column 0, a substitution in its first two symbols
                    return self._subs_read(r, 0, m_of(), ed, last_sub=even, fixed=(t & 1,))

                def start_lead(t):                           # 1 - 2 extra leading query symbols (cells left of column 1)
                    k = min(ed, 1 + (t & 1))
                    body = self._subs_read(r, 0, m_of() - k, ed - k, last_sub=even and ed > k)
                    lead = np.array([_other(seq[0], rng) for _ in range(k)], np.uint8)
                    return np.concatenate([lead, body])

                def start_del(t):                            # the lane's first 1 - 2 symbols are missing from the read
                    return self._subs_read(r, 1 + (t & 1), m_of(), ed, last_sub=even, fixed=(t >> 1 & 1,))

                def end_sub(t):                              # the read ends flush with the lane's last symbol, an edit in its last two
                    m = m_of()
                    return self._subs_read(r, n - m, m, ed, fixed=(m - 1 if even else m - 2 + (t & 1),))

                def end_over(t):                             # the read runs 1 - 2 symbols past the lane's end (into pads, or past the clump)
                    k = min(ed, 1 + (t & 1))
                    m = m_of() - k
                    body = self._subs_read(r, n - m, m, ed - k)
                    return np.concatenate([body, _rand(rng, k)])
                for nm, fn in (("start_sub", start_sub), ("start_lead", start_lead), ("start_del", start_del), ("end_sub", end_sub), ("end_over", end_over)):
                    self._aim("edge_%s/%s" % (nm, base), "edge_" + nm, r, W, fn, tries=4)

    # ---- 3. phase of the register window and of the packed query ----------------------------------------------------------
    def _phase(self):
        rng = self.rng
        r = self.of_kind("rand")[-1]                         # in the longest clump
        r2 = self.of_kind("rand")[1]
        for s in list(range(0, 8)) + list(range(24, 57)):    # every start residue modulo 8, and modulo 32 across a chunk boundary
            for rr in (r, r2):
                self._aim("phase_start/s%d/r%d" % (s, rr), "phase", rr, None, lambda t, s=s, rr=rr: self._subs_read(rr, s, 80, 2))
        for m in range(57, 73):                              # every read length modulo 8
            self._aim("phase_len/m%d" % m, "phase", r, None, lambda t, m=m: self._subs_read(r, 101, m, 1 + (m & 1)))
        for rr in self.of_kind("iupac1", "iupacrun"):        # a code in the lane at every offset of the read: it enters and leaves the
            p = self.lanes[rr].codes[0]                      # register window at every row phase, a refill among them
            for t in range(0, 64):
                def make(_, rr=rr, t=t, p=p):
                    q = self._subs_read(rr, p - t, 64, 1 + (t & 1))
                    if t & 2:                                # the code resolved to a base instead of copied
                        for k in self.lanes[rr].codes:
                            if 0 <= k - (p - t) < 64:
                                q[k - (p - t)] = 1 + 2 * int(rng.integers(0, 2))
                    return q
                self._aim("phase_refcode/r%d/t%d" % (rr, t), "phase", rr, None, make)
        for t in range(8, 24):                               # the same with the code in the read
            def make(_, t=t):
                q = self._subs_read(r, 60 + t, 70, 1)
                q[t] = (8, 5, 12, 9)[t & 3]
                return q
            self._aim("phase_querycode/t%d" % t, "phase", r, None, make, slack=1)
        for i in range(8):                                   # N in the read (costs 1 everywhere under score table 1, 0 under table 0)
            def make(_, i=i):
                q = self._subs_read(r2, 40 + 3 * i, 64 + i, 1)
                q[20 + i] = 5
                if i & 1:
                    q[41] = 5
                return q
            self._aim("phase_N/%d" % i, "phase", r2, None, make, slack=2)
        for i in range(4):                                   # one symbol outside the alphabet in the middle of the read
            def make(_, i=i):
                q = self._subs_read(r, 120 + i, 66 + i, 1)
                return np.concatenate([q[:33], [0], q[33:]]).astype(np.uint8)
            self._aim("phase_code0/%d" % i, "phase", r, None, make)

    # ---- 4. ties ------------------------------------------------------------------------------------------------------
    def _ties(self):
        rng = self.rng
        lanes = [r for r in self.of_kind("hp", "tr", "hp_start", "tr_end") if (r >> 4) in (1, 3)]
        for r in lanes:
            seq = self.lanes[r].seq
            a, k, unit = self.lanes[r].stretch
            reps, ul = k // len(unit), len(unit)
            for d in (-3, -2, -1, 1, 2, 3):                  # the stretch 1 - 3 units shorter / longer in the read
                for mode, fl, fr in (("both", 18, 18), ("left", 18, 0), ("right", 0, 18), ("none", 0, 0), ("right1", 18, 1), ("right2", 18, 2)):
                    fl, fr = min(fl, a), min(fr, len(seq) - a - k)
                    for sub in ((0, 1, 2) if abs(d) == 1 else (0,)):     # 1: a substitution next to the stretch; 2: an extra symbol in a flank too
                        if sub and not (fl > 2 or fr > 2):
                            continue

                        def make(_, d=d, fl=fl, fr=fr, sub=sub):
                            left, right = seq[a - fl:a].copy(), seq[a + k:a + k + fr].copy()
                            if sub and fl > 2:
                                left[-1] = _other(left[-1], rng)
                            elif sub:
                                right[0] = _other(right[0], rng)
                            if sub == 2:
                                side = left if fl > 8 else right
                                ins = np.insert(side, len(side) // 2, _other(side[len(side) // 2], rng))
                                left, right = (ins, right) if fl > 8 else (left, ins)
                            return np.concatenate([left, np.tile(unit, reps + d), right]).astype(np.uint8)
                        self._aim("tie_%s/r%d/d%+d/s%d" % (mode, r, d, sub), "tie", r, None, make, slack=1, keep_exact=False)

    def _ties_early(self):
        """Two neighbouring symbols swapped at the read's second to fourth position.  Two substitutions, or a gap on either side; with row
        1 of the re-scorer taking the substitution cost alone, paths of equal score and equal gapQ but different gapR meet a few rows
        down, one from above and one from the left: about every third such read rests on the up-before-left priority (measured with
        rescore_cells; test_rescore_cases_cpu.py counts them).  Further substitutions spread the reads over the narrow variants."""
        rng = self.rng
        lanes = self.of_kind("rand", "longest", "short")
        for i in range(150):
            r = lanes[i % len(lanes)]
            n = len(self.lanes[r].seq)
            m, p, extra = 32 + i % 17, 1 + (i % 5 == 4) + (i % 10 == 9), i % 4

            def make(_, r=r, n=n, m=m, p=p, extra=extra):
                q = self._subs_read(r, int(rng.integers(0, n - m)), m, extra, fixed=tuple(_spread(m, extra, rng, lo=12, hi=m - 2)))
                k = p
                while k < 8 and q[k] == q[k + 1]:
                    k += 1
                q[k], q[k + 1] = q[k + 1], q[k]
                return q
            self._aim("tie_early/%d/p%d" % (i, p), "tie_early", r, None, make, slack=1, keep_exact=False)

    # ---- batches ------------------------------------------------------------------------------------------------------
    def select(self, *families):
        return [c for c in self.cases if not families or any(c.family.startswith(f) for f in families)]

    def batch(self, cases, rep=1, cap=None, long_read=False):
        """the cases as one batch (rep copies, every entry its own slot); cap: an upper limit for every budget"""
        seqs = [c.q for c in cases] * rep
        emac = [c.emac if cap is None else min(c.emac, cap) for c in cases] * rep
        if long_read:
            seqs.append(self.long_read); emac.append(max(emac) if cap is None else cap)
        return Batch(seqs, emac)


_set = None


def build_cases():
    """the case set (built once per process).  The builder aims under score table 1; the same database and reads serve both
    tables -- what a case is under a table comes from the DP and the oracle under that table."""
    global _set
    import oraclelib as ol
    if _set is None:
        _set = CaseSet(ol.score_lut(1))
    return _set
