"""Constructed inputs for the edit-distance sweeps -- k_myers_prefix<NWP> / k_myers_prefix_task<NWP>, k_myers_window<NW>,
k_myers_window_band<BW>, k_myers<NW>, k_myers_long -- and a plain model of the prefix stage.  TEST INFRASTRUCTURE ONLY, no GPU code.

A CELL is one batch whose entries all have m symbols, so that they sit in one length class (NW words) and the library picks exactly
one number of prefix words NWP for them (class_prefix_words, restated below as prefix_words()).  MATRIX is the table of cells: two
per admissible (NW, NWP), the one-stage cells and the cells of the long kernel.  Every length class has one small database shared by
its cells (class_db), every cell a list of reads planted at known places of known lanes (Cell.reads).  What a read actually is -- its
edit distance, the lanes it flags -- is never taken from the builder's intention: the oracle and the model say, and
test_sweep_cases_cpu.py holds the builder to what test_gpu_sweep_variants.py relies on."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261021
K_ACX = 12                                                  # word length of the accelerator of the `tasks` cells
CLASS_NW = (2, 4, 6, 8, 10, 16, 32)                         # kClasses without the class beyond 1 024 symbols
LOWER_EDGE = {2: 33, 4: 65, 6: 129, 8: 193, 10: 257, 16: 321, 32: 513}      # 32 * (previous NW) + 1; 33 for the first class
E_RANGE = {1: (1, 5), 2: (6, 10), 3: (11, 16), 4: (17, 21), 6: (22, 32)}    # budgets for which the library takes NWP prefix words
REPEAT_LENS = (160, 64, 104, 144, 48, 80, 120, 40, 152, 72, 96, 128)        # tandem repeat of the 12 lanes that carry one (lane 4 j: entry j)

# ---------------------------------------------------------------------------------------------------------------------
# The matrix.  (NW, NWP, m, Emax): for every NW and every NWP < NW the top of NWP's budget range at the class's lower edge
# (shift = 32 NW - m as large as it gets: the band starts many words up) and the bottom of the range at m = 32 NW (every Pv word all
# ones, no filler row).  Emax < m / 3 holds for every row as it stands (the tightest: 16 against 65), so no m had to move.
# (4, 3, 65, 16): the prefix is the whole query, P = m.
# ---------------------------------------------------------------------------------------------------------------------
TWO_STAGE = (
    (2, 1, 33, 5), (2, 1, 64, 1),
    (4, 1, 65, 5), (4, 1, 128, 1), (4, 2, 65, 10), (4, 2, 128, 6), (4, 3, 65, 16), (4, 3, 128, 11),
    (6, 1, 129, 5), (6, 1, 192, 1), (6, 2, 129, 10), (6, 2, 192, 6), (6, 3, 129, 16), (6, 3, 192, 11), (6, 4, 129, 21), (6, 4, 192, 17),
    (8, 1, 193, 5), (8, 1, 256, 1), (8, 2, 193, 10), (8, 2, 256, 6), (8, 3, 193, 16), (8, 3, 256, 11), (8, 4, 193, 21), (8, 4, 256, 17),
    (8, 6, 193, 32), (8, 6, 256, 22),
    (10, 1, 257, 5), (10, 1, 320, 1), (10, 2, 257, 10), (10, 2, 320, 6), (10, 3, 257, 16), (10, 3, 320, 11), (10, 4, 257, 21), (10, 4, 320, 17),
    (10, 6, 257, 32), (10, 6, 320, 22),
    (16, 1, 321, 5), (16, 1, 512, 1), (16, 2, 321, 10), (16, 2, 512, 6), (16, 3, 321, 16), (16, 3, 512, 11), (16, 4, 321, 21), (16, 4, 512, 17),
    (16, 6, 321, 32), (16, 6, 512, 22),
    (32, 1, 513, 5), (32, 1, 1024, 1), (32, 2, 513, 10), (32, 2, 1024, 6), (32, 3, 513, 16), (32, 3, 1024, 11), (32, 4, 513, 21), (32, 4, 1024, 17),
    (32, 6, 513, 32), (32, 6, 1024, 22),
)
# The rows of TWO_STAGE whose largest budget leaves no guaranteed seed word of K_ACX symbols (seed_need() < 1): their entries leave the
# prefilter route, so they are fed as `pairs` only.  The other 40 rows have a `tasks` twin.  (4, 3), (6, 4) and (8, 6) have no twin in
# either row: those widths never run through k_myers_prefix_task here on purpose, only through k_myers_prefix.
PAIRS_ONLY = (
    (2, 1, 33, 5), (4, 1, 65, 5), (4, 2, 65, 10), (4, 3, 65, 16), (4, 3, 128, 11), (6, 2, 129, 10), (6, 3, 129, 16), (6, 4, 129, 21),
    (6, 4, 192, 17), (8, 3, 193, 16), (8, 4, 193, 21), (8, 6, 193, 32), (8, 6, 256, 22), (10, 4, 257, 21), (10, 6, 257, 32), (16, 6, 321, 32),
)
# one stage: a budget beyond every prefix (33) at m = 32 NW -- not for NW = 2, where 33 >= 64 / 3 --, and the lower edge with option
# two_stage = 0; (NW, m, Emax, options)
ONE_STAGE = tuple((nw, 32 * nw, 33, {}) for nw in CLASS_NW if nw != 2) + tuple((nw, LOWER_EDGE[nw], 10, {"two_stage": 0}) for nw in CLASS_NW)
# k_myers_long: the first length beyond the register kernels, a full last word, one symbol more, BHIP_MAX_QLEN; (m, Emax)
LONG = ((1025, 10), (1056, 10), (1057, 10), (4095, 10))


def prefix_words(max_e, nw, two_stage=1):
    """class_prefix_words: about 6 prefix symbols per allowed edit, in whole words out of {1, 2, 3, 4, 6}, fewer than the query has"""
    if not two_stage or nw > 32:
        return 0
    want = (6 * max_e + 31) // 32
    nwp = 1 if want <= 1 else want if want <= 4 else 6 if want <= 6 else 0
    return nwp if nwp < nw else 0


def rule_matrix():
    """TWO_STAGE derived from the rule (the CPU module compares the table above with it)"""
    out = []
    for nw in CLASS_NW:
        for nwp in (1, 2, 3, 4, 6):
            if nwp >= nw:
                continue
            for emax, m in ((E_RANGE[nwp][1], LOWER_EDGE[nw]), (E_RANGE[nwp][0], 32 * nw)):
                while 3 * emax >= m:
                    m += 1
                out.append((nw, nwp, m, emax))
    return tuple(out)


def win_class(g_first, g_last, e):
    """bhip_win_class: a band of BW words holds 32 (BW - 1) - 6 diagonals; the flagged ones are 8 (g_last - g_first) + 8 + 2 E"""
    diags = 8 * (g_last - g_first) + 8 + 2 * e
    return 0 if diags <= 26 else 1 if diags <= 58 else 2 if diags <= 90 else 3


def seed_need(m, e, k=K_ACX):
    """The seed plan of a read of A/C/G/T only (make_seed_plan): sampled words at stride s guarantee need = W - E * ceil(K / s)
    survivors, W = (m - K) // s + 1.  The widest stride that leaves 3 is taken, else the stride with the most; below 1 the entry
    leaves the prefilter route and is aligned against every clump."""
    if m < k:
        return 0
    smin = (m - k) // 254 + 1

    def need(s):
        return (m - k) // s + 1 - e * ((k + s - 1) // s)
    for s in range(max(k, smin), smin - 1, -1):
        if need(s) >= 3:
            return need(s)
    return max(0, max(need(s) for s in range(smin, max(k, smin) + 1)))


# ---------------------------------------------------------------------------------------------------------------------
# the model of the prefix stage (tests/csrc/sweep_model.c)
# ---------------------------------------------------------------------------------------------------------------------
_model = None


def model_lib():
    global _model
    if _model is None:
        d = tempfile.mkdtemp(prefix="sweep_model_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "sweep_model.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-std=gnu11", "-Wall", os.path.join(HERE, "csrc", "sweep_model.c"), "-o", so])
        L = C.CDLL(so)
        L.sw_prefix_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.sw_prefix_rows.restype = C.c_int
        _model = L
    return _model


def prefix_rows(q, P, lanes, lut):
    """row P of the plain matrix of q[:P] against every row of `lanes` (uint8 [n, Lp]): int32 [n, Lp], column x at index x - 1"""
    q = np.ascontiguousarray(q, np.uint8)
    lanes = np.ascontiguousarray(lanes, np.uint8)
    lut = np.ascontiguousarray(lut, np.uint8)
    out = np.zeros(lanes.shape, np.int32)
    rc = model_lib().sw_prefix_rows(q.ctypes.data, int(P), lanes.ctypes.data, lanes.shape[0], lanes.shape[1], lut.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out


def prefix_model(db, batch, nwp, lut):
    """What the prefix stage must find for a batch: per (entry, live lane) the first and last group of 8 columns whose minimum of
    D[P][.] is <= the entry's budget, P = min(m, 32 NWP), over the lane padded with code 0 to 32 * ceil(ClumpLen / 32) columns.
    Returns (g_first int64 [n, tot] with -1 = not flagged, g_last, cls = win_class of the flagged ones, else -1)."""
    n, tot = batch.n, db.tot
    g_first = np.full((n, tot), -1, np.int64)
    g_last = np.full((n, tot), -1, np.int64)
    for c, lanes in enumerate(db.padded_clumps()):
        live = min(16, tot - 16 * c)
        for j in range(n):
            q = batch.seqs[j]
            P = min(len(q), 32 * nwp)
            rows = prefix_rows(q, P, lanes[:live], lut)
            fl = rows.reshape(live, -1, 8).min(axis=2) <= int(batch.emac[j])
            anyf = fl.any(axis=1)
            g_first[j, 16 * c:16 * c + live] = np.where(anyf, fl.argmax(axis=1), -1)
            g_last[j, 16 * c:16 * c + live] = np.where(anyf, fl.shape[1] - 1 - fl[:, ::-1].argmax(axis=1), -1)
    e = batch.emac.astype(np.int64)[:, None]
    diags = 8 * (g_last - g_first) + 8 + 2 * e
    cls = np.where(g_first < 0, -1, np.where(diags <= 26, 0, np.where(diags <= 58, 1, np.where(diags <= 90, 2, 3))))
    return g_first, g_last, cls


def window_columns(db, batch, nwp, g_first, g_last):
    """Columns the window stage sweeps for the model's windows, as both window kernels count them (n_window_columns): prefix ends in the
    1-based columns 8 g_first + 1 .. 8 g_last + 8 put the alignment's columns within [8 g_first + 2 - (P + E), 8 (g_last + 1) + (m - P) + E],
    cut to the lane's chunks and widened to whole groups of 8.
    This restates the window kernels' own column arithmetic from the model's flags, so it is not independent of them: it pins the
    counter (a change of the swept range shows up), it does not prove that the range is right.  That the range suffices is what the
    records' equality with the oracle shows."""
    total = 0
    for j in range(batch.n):
        m, e = len(batch.seqs[j]), int(batch.emac[j])
        P = min(m, 32 * nwp)
        for r in np.flatnonzero(g_first[j] >= 0):
            cols = 32 * ((int(db.clump_len[r >> 4]) + 31) // 32)
            c_lo = max(8 * int(g_first[j, r]) + 2 - (P + e) - 1, 0)
            c_hi = min(8 * (int(g_last[j, r]) + 1) + (m - P) + e - 1, cols - 1)
            total += 8 * ((c_hi >> 3) - (c_lo >> 3) + 1)
    return total


# ---------------------------------------------------------------------------------------------------------------------
# databases, one per length class
# ---------------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return rng.integers(1, 5, size=n, dtype=np.uint8)


def _other(s, rng):
    return np.uint8((int(s) - 1 + int(rng.integers(1, 4))) % 4 + 1)


def class_key(m):
    """the database a read length belongs to: the register classes by their words, the long kernel's lengths in two groups"""
    for nw in CLASS_NW:
        if m <= 32 * nw:
            return nw
    return "long" if m <= 1057 else "max"


_CLASS_MAX = {**{nw: 32 * nw for nw in CLASS_NW}, "long": 1057, "max": 4095}


def class_rate(key):
    """Edited fraction of a family's variants.  Two siblings differ in about 2 * rate * m places over a read: 8 over the class's
    longest read, so that a read which leaves half of a budget of 16 or more unspent meets them too, and 0.03 (about 4 over 64
    symbols) for the short classes.  test_sweep_cases_cpu.py counts the sibling records."""
    return min(0.03, 4.0 / _CLASS_MAX[key])


class ClassDB:
    """46 references in 3 clumps: 6 random bases x 8 variants without the last two (two dead lanes in the last clump), m_max + 150 .. 260
    symbols; every fifth lane cut short by 30 .. 80 symbols (pads trail it); every fourth lane with a tandem repeat of one unit of 3 .. 8
    symbols shared by the class, REPEAT_LENS long, starting 16 .. 100 symbols into the lane"""

    def __init__(self, key):
        from burst_amd import synth
        import dbutil
        self.key, self.max_m = key, _CLASS_MAX[key]
        rng = np.random.default_rng([SEED, self.max_m])
        seqs = []
        for _ in range(6):
            base = _rand(rng, self.max_m + int(rng.integers(150, 261)))
            seqs += [np.array(v, np.uint8) for v in synth.mutate_family(base, 8, class_rate(key), rng)]
        seqs = seqs[:46]
        self.unit = _rand(rng, int(rng.integers(3, 9)))
        while len(set(self.unit.tolist())) < 2:
            self.unit = _rand(rng, len(self.unit))
        self.repeat = {}                                     # lane -> (start, length)
        for i in range(len(seqs)):
            if i % 4 == 0:
                a, n = int(rng.integers(16, 101)), REPEAT_LENS[i // 4]
                seqs[i][a:a + n] = np.resize(self.unit, n)
                self.repeat[i] = (a, n)
            elif i % 5 == 2:
                seqs[i] = seqs[i][:len(seqs[i]) - int(rng.integers(30, 81))].copy()
        self.seqs = seqs
        self.packed, self.clump_len, self.tot = dbutil.pack_clumps(seqs)
        self.lens = np.array([len(s) for s in seqs])
        self._padded = None
        self._acx = None

    def padded_clumps(self):
        """per clump uint8 [16, 32 * ceil(ClumpLen / 32)]: the lanes as the sweeps read them, code 0 behind each"""
        if self._padded is None:
            self._padded = []
            for c, L in enumerate(self.clump_len):
                a = np.zeros((16, 32 * ((int(L) + 31) // 32)), np.uint8)
                for z, s in enumerate(self.seqs[16 * c:16 * c + 16]):
                    a[z, :len(s)] = s
                self._padded.append(a)
        return self._padded

    def full_lanes(self):
        """lanes as long as their clump"""
        return [i for i in range(self.tot) if self.lens[i] == self.clump_len[i >> 4]]

    def short_lanes(self):
        """the lanes that were cut short (pads of 30 symbols or more behind them)"""
        return [i for i in range(self.tot) if i % 5 == 2 and i % 4 and self.lens[i] + 30 <= self.clump_len[i >> 4]]

    def plain_lanes(self):
        return [i for i in range(self.tot) if i % 4 and not (i % 5 == 2)]

    def acx(self):
        import dbutil
        if self._acx is None:
            lens, entries, _ = dbutil.build_acx(self.seqs, K_ACX)
            self._acx = dict(acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=K_ACX)
        return self._acx


_dbs = {}


def class_db(key):
    if key not in _dbs:
        _dbs[key] = ClassDB(key)
    return _dbs[key]


# ---------------------------------------------------------------------------------------------------------------------
# cells
# ---------------------------------------------------------------------------------------------------------------------
class Read:
    def __init__(self, place, seq, e, lane, start, k, strict=True):
        """place: the placement's name; lane / start: where it was cut (0-based symbol of the lane); k: edits planted; strict: the edits lie
        where the name says (False where the query leaves no room, e.g. no suffix behind a prefix that is the whole query)"""
        self.place, self.seq, self.e, self.lane, self.start, self.k, self.strict = place, np.asarray(seq, np.uint8), int(e), int(lane), int(start), int(k), strict


class Batch:
    """a flat query batch with the attributes of burst_amd.capi.Queries: the reads' entries followed by their reverse complements"""

    def __init__(self, seqs, emac, flags=None):
        from burst_amd import synth
        n = len(seqs)
        self.seqs = [np.asarray(s, np.uint8) for s in seqs] + [synth.revcomp(s) for s in seqs]
        self.off = np.zeros(2 * n + 1, np.uint64)
        np.cumsum([len(s) for s in self.seqs], out=self.off[1:])
        self.codes = np.concatenate(self.seqs)
        self.emac = np.ascontiguousarray(list(emac) * 2, np.uint16)
        self.six = np.ascontiguousarray(list(range(n)) * 2, np.uint32)
        self.rc = np.ascontiguousarray([0] * n + [1] * n, np.uint8)
        self.flags = flags
        self.n = 2 * n
        self.n_shared = n


class Cell:
    def __init__(self, nw, nwp, m, emax, feeder="pairs", options=None):
        self.nw, self.nwp, self.m, self.emax, self.feeder = nw, nwp, m, emax, feeder
        self.options = dict(options or {})
        self.key = class_key(m)
        self.kind = "two_stage" if nwp else "long" if m > 1024 else "one_stage"
        self.name = "nw%d_p%d_m%d_e%d%s_%s" % (nw, nwp, m, emax, "_ts0" if self.options.get("two_stage") == 0 else "", feeder)
        self._reads = None
        self._batch = None

    @property
    def P(self):
        """the prefix's symbols; for the cells without a prefix stage the placements use half the query"""
        return min(self.m, 32 * self.nwp) if self.nwp else self.m // 2

    @property
    def budgets(self):
        return (self.emax, self.emax // 2, 1, 0)

    @property
    def band_classes(self):
        """The band classes the cell's windows must populate, from the formula alone: a window's flagged diagonals number 8 (g_last - g_first)
        + 8 + 2 E, so an entry of budget E reaches class win_class(0, 0, E) at best -- 8 + 2 E <= 26 for class 0 -- and every class above
        it up to 3 as its flagged run grows (budget slack; the shared tandem repeat for the small budgets).  The cell's budgets include 0,
        so that is every class.  With 2 words (NW = 2) no band kernel exists, and without a prefix stage there are no windows."""
        if not self.nwp or self.nw == 2:
            return ()
        return tuple(range(min(win_class(0, 0, b) for b in self.budgets), 4))

    def survives_prefilter(self):
        """every entry keeps a guaranteed seed word (the largest budget decides): the cell can be fed through lane tasks"""
        return seed_need(self.m, self.emax) >= 1

    # ---- the reads -------------------------------------------------------------------------------------------------
    def reads(self):
        if self._reads is None:
            self._reads = _plant(self)
        return self._reads

    def batch(self):
        """forward entries and their reverse complements; every second read is planted on the reverse strand (its forward entry is
        the reverse complement of what was cut, so the hit belongs to the second half of the batch)"""
        if self._batch is None:
            from burst_amd import synth
            rs = self.reads()
            seqs = [r.seq if i % 2 == 0 else synth.revcomp(r.seq) for i, r in enumerate(rs)]
            flags = np.zeros(2 * len(rs), np.uint8) if self.feeder == "tasks" else None
            self._batch = Batch(seqs, [r.e for r in rs], flags)
        return self._batch

    def entry_of(self, i):
        """the batch entry that carries read i as it was cut"""
        return i if i % 2 == 0 else len(self.reads()) + i


def _start_with_column(rng, lo, hi, mod, res):
    """a 0-based start in [lo, hi) whose 1-based column start + 1 is res modulo mod"""
    s = int(rng.integers(lo, max(lo + 1, hi - mod)))
    return s + (res - (s + 1)) % mod


def _plant(cell):
    db = class_db(cell.key)
    rng = np.random.default_rng([SEED, cell.nw, cell.nwp, cell.m, cell.emax])
    m, P, E, E2 = cell.m, cell.P, cell.emax, cell.emax // 2
    plain, full, short = db.plain_lanes(), db.full_lanes(), db.short_lanes()
    reps = sorted(db.repeat, key=lambda i: -db.repeat[i][1])            # longest repeat first
    out = []

    def lane_for(k):
        return plain[(k * 7 + cell.m) % len(plain)]

    def start_for(lane, col=None, need=m):
        hi = int(db.lens[lane]) - need - 2
        assert hi > 2, (cell.name, lane)
        return _start_with_column(rng, 1, hi, *col) if col else int(rng.integers(1, hi))

    def subs(seq, pos):
        for p in pos:
            seq[p] = _other(seq[p], rng)
        return seq

    def pick(lo, hi, k):
        """k distinct positions in [lo, hi); fewer where the range is smaller"""
        lo, hi = max(lo, 0), min(hi, m)
        k = min(k, max(hi - lo, 0))
        return sorted(rng.choice(np.arange(lo, hi), size=k, replace=False).tolist()) if k else []

    def mixed(lane, start, lo, hi, k):
        """a read of m symbols from `start` with k edits (substitutions, insertions and deletions 3 : 1 : 1) at read positions inside [lo, hi)"""
        src = db.seqs[lane]
        kinds = rng.choice(["s", "s", "s", "i", "d"], size=k).tolist()
        room = hi - lo - 2 * k - 2
        if room < k:                                         # too tight for coordinate shifts: substitutions only
            return subs(src[start:start + m].copy(), pick(lo, hi, k))
        pos = sorted(rng.choice(np.arange(lo + k, hi - k - 1), size=k, replace=False).tolist())     # positions in the lane's segment
        parts, last = [], 0
        seg = src[start:start + m + k + 2]
        for p, kd in zip(pos, kinds):
            parts.append(seg[last:p])
            if kd == "s":
                parts.append(np.array([_other(seg[p], rng)], np.uint8)); last = p + 1
            elif kd == "d":
                last = p + 1
            else:
                parts.append(np.array([_other(seg[p], rng)], np.uint8)); last = p
        parts.append(seg[last:])
        q = np.concatenate(parts)[:m]
        assert len(q) == m
        return q.astype(np.uint8)

    def add(place, seq, e, lane, start, k, strict=True):
        assert len(seq) == m, (cell.name, place, len(seq))
        out.append(Read(place, seq, e, lane, start, k, strict))

    def prefix(e, k, col, n):                                # all edits inside the first P symbols
        lane = lane_for(n); st = start_for(lane, col, m + k + 2)
        add("prefix", mixed(lane, st, 1, P, k), e, lane, st, k)

    def suffix(e, k, col, n, lane=None, st=None, place="suffix"):      # all edits inside the last m - P symbols
        lane = lane_for(n) if lane is None else lane
        st = start_for(lane, col, m + k + 2) if st is None else st
        strict = m - 1 - P >= k and k > 0 or k == 0
        lo = P if strict else max(1, m - 1 - 2 * k - 4)
        add(place, mixed(lane, st, lo, m - 1, k), e, lane, st, k, strict)

    def boundary_del(e, col, n):                             # e symbols of the lane missing directly before query symbol P
        lane = lane_for(n); st = start_for(lane, col, m + e + 2)
        src = db.seqs[lane]
        cut = min(P, m - 1)
        q = np.concatenate([src[st:st + cut], src[st + cut + e:st + m + e]])
        add("boundary_del", q, e, lane, st, e, strict=P < m)

    def boundary_ins(e, col, n):                             # e extra symbols directly behind query symbol P
        lane = lane_for(n); st = start_for(lane, col)
        src = db.seqs[lane]
        head = min(P + 1, m - 1)
        k = min(e, m - head - 1) if m - head - 1 > 0 else 0
        ins = np.array([_other(src[st + head], rng) for _ in range(k)], np.uint8)
        q = np.concatenate([src[st:st + head], ins, src[st + head:st + m - k]])
        add("boundary_ins", q, e, lane, st, k, strict=k == e and P < m)

    def whole(e, k, col, n, place="subs", lane=None, st=None):      # substitutions only, anywhere
        lane = lane_for(n) if lane is None else lane
        st = start_for(lane, col) if st is None else st
        add(place, subs(db.seqs[lane][st:st + m].copy(), pick(0, m, k)), e, lane, st, k)

    def col1(e, inserted):                                   # starts at column 1 of the lane, once with its first symbol inserted
        lane = lane_for(11 + inserted)
        src = db.seqs[lane]
        q = np.concatenate([[_other(src[0], rng)], src[:m - 1]]).astype(np.uint8) if inserted else src[:m].copy()
        add("col1_ins" if inserted else "col1", q, e, lane, 0, int(inserted))

    def at_end(e, k, lanes, place, n):                       # ends on the lane's last column
        lane = lanes[(n + cell.m) % len(lanes)]
        st = int(db.lens[lane]) - m
        add(place, subs(db.seqs[lane][st:st + m].copy(), pick(0, m - 1, k)), e, lane, st, k)

    def from_repeat(e, k, which, place="repeat"):            # cut from the start of a tandem repeat, its edits behind the prefix
        lane = reps[which % len(reps)]
        a = db.repeat[lane][0]
        suffix(e, k, None, 0, lane=lane, st=a, place=place)

    if m >= 513:
        n_reads = 2 if m == 4095 else 8
        prefix(E, E, (8, 0), 0)
        from_repeat(E, E, 0, place="suffix")                 # (the suffix placement, cut from the longest repeat)
        if n_reads > 2:
            boundary_ins(E, (64, 31), 2)
            at_end(E, E2, full, "end_full", 3)               # (half the budget left: the lane's siblings come within reach)
            boundary_del(E2, (8, 7), 4)
            at_end(E2, E2, short, "end_short", 5)
            col1(1, True)
            from_repeat(0, 1, 2, place="over")               # one edit for a budget of none
        return out
    prefix(E, E, (8, 0), 0)
    suffix(E, E, (8, 1), 1)
    boundary_del(E, (8, 7), 2)
    boundary_ins(E, (64, 31), 3)
    whole(E, E, (64, 32), 4)
    whole(E, 0, (64, 33), 5, place="exact")
    at_end(E, E, full, "end_full", 6)
    at_end(E, E, short, "end_short", 7)
    from_repeat(E, E2, 0)
    whole(E, E + 1, None, 9, place="over")                   # one edit more than the budget, substitutions: nothing on its own lane
    col1(0, False)
    col1(1, True)
    from_repeat(1, 1, 2)
    from_repeat(0, 0, 5)
    prefix(E2, E2, None, 14)
    suffix(E2, E2, None, 15)
    boundary_del(E2, None, 16)
    boundary_ins(E2, None, 17)
    whole(E2, E2 + 1, None, 18, place="over")
    at_end(1, 1, full, "end_full", 19)
    at_end(0, 0, short, "end_short", 20)
    whole(0, 0, None, 21, place="exact")
    prefix(E, E2, None, 22)                                  # half the budget spent in the prefix: a flagged run of about 2 (E - E / 2) + 1 columns
    whole(E, E, None, 23)
    return out


def _cells():
    cells = []
    for nw, nwp, m, emax in TWO_STAGE:
        c = Cell(nw, nwp, m, emax)
        cells.append(c)
        if c.survives_prefilter():
            cells.append(Cell(nw, nwp, m, emax, feeder="tasks"))
    for nw, m, emax, opts in ONE_STAGE:
        cells.append(Cell(nw, 0, m, emax, options=opts))
    for m, emax in LONG:
        cells.append(Cell((m + 31) // 32, 0, m, emax))
    return cells


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)


def twin_source(cell):
    """the `pairs` cell whose reads a `tasks` cell shares (same batch but for the route flags)"""
    return BY_NAME[cell.name.replace("_tasks", "_pairs")]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's side, computed once per cell and mode and shared
# ---------------------------------------------------------------------------------------------------------------------
_expected = {}
_models = {}


def lut():
    import oraclelib as ol
    return ol.score_lut(1)


def expected(cell, all_hits):
    """the oracle's records of a cell's batch (the `tasks` twin has the same batch)"""
    import oraclelib as ol
    src = twin_source(cell)
    k = (src.name, bool(all_hits))
    if k not in _expected:
        db, b = class_db(src.key), src.batch()
        _expected[k] = ol.search(db.packed, db.clump_len, db.tot, b.codes, b.off, b.emac.astype(np.uint32), b.six, b.rc, b.n_shared, lut(), bool(all_hits))
    return _expected[k]


def model(cell):
    """prefix_model of a two-stage cell's batch"""
    src = twin_source(cell)
    if src.name not in _models:
        _models[src.name] = prefix_model(class_db(src.key), src.batch(), src.nwp, lut())
    return _models[src.name]
