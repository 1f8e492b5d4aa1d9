"""The inputs the chimera tests share (tests/test_chimera_cpu.py against the model, tests/test_gpu_chimera.py against bh_chimera_host):
(weights, lens, lines, ops, parameters) with lines as rows (q, r, flags, n_ops, op_off), the smallest shapes at which each step of
bhip_chimera_run can go wrong."""
import functools

import numpy as np

import chimeralib as ml

WMAX = 2 ** 32 - 1


def xs(length, at, ins=(), dels=()):
    """the CIGAR of a read of `length` symbols with X at the read indices `at`, I at `ins`, and a D column in front of every index of `dels`
    (length itself: behind the last symbol)"""
    sym = ["="] * length
    for p in at:
        sym[p] = "X"
    for p in ins:
        sym[p] = "I"
    seq = []
    for j in range(length + 1):
        seq += ["D"] * list(dels).count(j)
        if j < length:
            seq.append(sym[j])
    out, k = "", 0
    while k < len(seq):
        e = k
        while e < len(seq) and seq[e] == seq[k]:
            e += 1
        out += "%d%s" % (e - k, seq[k])
        k = e
    return out


def mirror(cigar):
    """the path of the reverse-complement entry that shows the same edits"""
    return "".join(reversed(ml.re.findall(r"[0-9]+[=XID]", cigar)))


class Case:
    def __init__(self, weights, lens, **par):
        self.w, self.lens, self.lines, self.ops, self.par = list(weights), list(lens), [], [], par

    def add(self, q, r, cigar, rev=False):
        words = ml.ops_of(mirror(cigar) if rev else cigar)      # cigar is always given in READ orientation
        self.lines.append((q, r, 1 if rev else 0, len(words), len(self.ops)))
        self.ops += words
        return self

    def done(self):
        return self.w, self.lens, self.lines, self.ops, self.par


def two_parents(length, rev_a=False, rev_b=False, **par):
    """read 0 (weight 1) = parent 1 up to the middle, parent 2 from there: its line towards 1 has three X in the right quarter, the one
    towards 2 three X in the left quarter"""
    c = Case([1, 9, 9], [length] * 3, **par)
    q4 = max(length // 4, 1)
    c.add(0, 1, xs(length, [length - 1 - q4 + d for d in (0, 2, 4) if 0 <= length - 1 - q4 + d < length]), rev_a)
    c.add(0, 2, xs(length, [d for d in (q4 - 4, q4 - 2, q4) if 0 <= d < length]), rev_b)
    return c.done()


def d_at_the_cut(rev):
    """len = 2G: one cut, c = 16.  Towards 1 a D exactly at the cut (position 32 = 2c: LEFT, in both orientations), towards 2 an X on
    symbol 16 (position 33: right).  bestL = 0 from parent 2, bestR = 0 from parent 1"""
    return Case([1, 2, 2], [32] * 3, min_gain=1).add(0, 1, xs(32, [], dels=[16]), rev).add(0, 2, xs(32, [16]), rev).done()


def i_runs(rev):
    """a leading run of three I towards 1, a trailing one towards 2"""
    return Case([1, 2, 2], [40] * 3).add(0, 1, xs(40, [], ins=[0, 1, 2]), rev).add(0, 2, xs(40, [], ins=[37, 38, 39]), rev).done()


def many_lines(k, seed=5):
    """read 0 with a line towards each of k candidate parents (weights 2 .. 5: several share a priority class), 0 .. 6 X each"""
    rng = np.random.default_rng(seed + k)
    length = 120
    c = Case([1] + [int(x) for x in rng.integers(2, 6, size=k)], [length] * (k + 1))
    for r in range(1, k + 1):
        c.add(0, r, xs(length, sorted(set(rng.integers(0, length, size=int(rng.integers(0, 7))).tolist()))), bool(rng.integers(0, 2)))
    return c.done()


def edits254():
    """a line of 254 edits (the most a path has) towards 1, X on every symbol of the left 254; towards 2 the right 254 symbols"""
    length = 600
    return Case([1, 3, 3], [length] * 3).add(0, 1, xs(length, range(254))).add(0, 2, xs(length, range(length - 254, length)), True).done()


def equal_left_goes_to_priority():
    """both parents have L = 0 and R = 0 at every cut of the middle: the one of higher priority (weight 5, node 2) is A and B -- role N"""
    return Case([1, 4, 5], [40] * 3).add(0, 1, xs(40, [])).add(0, 2, xs(40, [])).done()


def five_times():
    """five lines of one (q, r) with other edits and equal edits: the smallest, then the first given (its X lie right; the later one's left)"""
    c = Case([1, 2, 2], [40] * 3)
    c.add(0, 1, xs(40, [1, 2, 3, 4, 5])).add(0, 1, xs(40, [30, 31, 32])).add(0, 1, xs(40, [1, 2, 3, 4])).add(0, 1, xs(40, [2, 3, 4])).add(0, 1, xs(40, [30, 31, 32, 33]))
    c.add(0, 2, xs(40, [5, 6, 7]))
    return c.done()


def skew_edge():
    """S = 3: read 0 weighs 2, parents weigh 6 (exactly S w: candidates) and 5 (one below: not); read 4 weighs 1 and has all of them"""
    c = Case([2, 6, 6, 5, 1], [40] * 5, skew=3)
    for q in (0, 4):
        c.add(q, 1, xs(40, [30, 32, 34])).add(q, 2, xs(40, [3, 5, 7])).add(q, 3, xs(40, []))
    return c.done()


def wide_product():
    """weights 2^32 - 1 with S = 2^31 - 1: S x 2 = 2^32 - 2 <= 2^32 - 1 (candidates of read 0), S x 3 is beyond (read 1 has none); a 32-bit
    product would wrap"""
    c = Case([2, 3, WMAX, WMAX], [40] * 4, skew=2 ** 31 - 1)
    for q in (0, 1):
        c.add(q, 2, xs(40, [30, 32, 34])).add(q, 3, xs(40, [3, 5, 7]))
    return c.done()


def gain(d):
    """Single 3, Model 0: a gain of 3 against min_gain d"""
    w, lens, lines, ops, _ = two_parents(40)
    return w, lens, lines, ops, {"min_gain": d}


@functools.lru_cache(maxsize=None)
def random_case(seed, n=2000, lines=20000):
    """reads of 40 .. 140 symbols, weights 1 .. 8, lines towards neighbours in number with random paths consistent with len (X, I and D, both
    strands), a tenth of them a repeated (q, r) with another path"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 9, size=n)
    lens = rng.integers(40, 141, size=n)
    base = lines * 9 // 10
    q = rng.integers(0, n, size=base)
    r = (q + rng.integers(-6, 7, size=base)) % n
    dup = rng.integers(0, base, size=lines - base)
    q, r = np.concatenate([q, q[dup]]), np.concatenate([r, r[dup]])
    rows, ops = [], []
    for i in range(lines):
        m = int(lens[q[i]])
        k = int(rng.integers(0, 9))
        code = np.full(m, 7, dtype=np.int64)
        at = rng.integers(0, m, size=k)
        code[at] = np.where(rng.random(k) < 0.7, 8, 1)
        nd = int(rng.integers(0, 3)) if rng.random() < 0.3 else 0
        seq = np.insert(code, np.sort(rng.integers(0, m + 1, size=nd)), 2) if nd else code
        edge = np.flatnonzero(np.diff(seq)) + 1
        start = np.concatenate([[0], edge])
        run = np.diff(np.concatenate([start, [len(seq)]]))
        words = (run << 4 | seq[start]).tolist()
        rows.append((int(q[i]), int(r[i]), int(rng.integers(0, 2)), len(words), len(ops)))
        ops += words
    return [int(x) for x in w], [int(x) for x in lens], rows, ops, {}


RANDOM_SEEDS = (1, 2, 3)

CASES = {
    "baseline": two_parents(40),
    "baseline_reverse": two_parents(40, True, True),
    "baseline_mixed_strands": two_parents(40, False, True),
    "d_at_the_cut": d_at_the_cut(False),
    "d_at_the_cut_reverse": d_at_the_cut(True),
    "i_runs": i_runs(False),
    "i_runs_reverse": i_runs(True),
    "len_2g_one_cut": two_parents(32),
    "len_2g_minus_1": two_parents(31),
    "len_1": two_parents(1),
    "edits254": edits254(),
    "equal_left_goes_to_priority": equal_left_goes_to_priority(),
    "five_times": five_times(),
    "skew_edge": skew_edge(),
    "wide_product": wide_product(),
    "self_lines_only": Case([1, 2], [40, 40]).add(0, 0, xs(40, [])).add(1, 1, xs(40, [3])).done(),
    "one_candidate_only": Case([1, 2, 1], [40] * 3).add(0, 1, xs(40, [3, 4, 5])).add(0, 2, xs(40, [30])).done(),
    "no_lines": ([1, 2, 3], [40, 50, 60], [], [], {}),
    "gain_exactly_d": gain(3),
    "gain_d_minus_1": gain(4),
    "min_seg_1": two_parents(40, min_seg=1),
}
for _len in (63, 64, 65, 129, 4095):
    CASES["len_%d" % _len] = two_parents(_len, _len % 2 == 1, False)
for _k in (1, 2, 64, 65, 1500):
    CASES["lines_%d" % _k] = many_lines(_k)
