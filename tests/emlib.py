"""The abundance definition (--abundance) as a plain Python model: Python integers for every sum, numpy.float64 for
the one division per (class, candidate).  Written from the definition, not from the C or the HIP: bh_em_host and bhip_em_run are both
compared against it.

  em(n_headers, group_w, lines, max_iters, tol) -> (counts, info)
      group_w[g] = reads of group g, lines = iterable of (group, header); counts in units of 2^-30 read;
      info = [iterations, distinct pairs of participating groups, classes, last delta, 1 if it stopped on tol]
  b6_groups(text)      -> (headers ascending, group_w, lines, read names): read = column 1, header = column 2 of a .b6 text
  table_text(headers, names, columns) -> what PREFIXabundance.txt holds for per-sample count columns"""
import numpy as np

ONE = 1 << 30
SCALE = np.float64(1073741824.0)


def candidate_sets(n_headers, group_w, lines):
    """{group: sorted tuple of distinct headers} of the participating groups (a line at all, weight > 0)"""
    sets = {}
    for g, h in lines:
        g, h = int(g), int(h)
        assert 0 <= g < len(group_w) and 0 <= h < n_headers
        if int(group_w[g]) > 0:
            sets.setdefault(g, set()).add(h)
    return {g: tuple(sorted(s)) for g, s in sets.items()}


def classes_of(n_headers, group_w, lines):
    """{candidate set: summed weight} and the number of distinct (group, header) pairs"""
    sets = candidate_sets(n_headers, group_w, lines)
    cls = {}
    for g, s in sets.items():
        cls[s] = cls.get(s, 0) + int(group_w[g])
    return cls, sum(len(s) for s in sets.values())


def step(n_headers, cls, c):
    """one iteration: the counts after it (the divisions of one class in one numpy.float64 array operation: the same IEEE division)"""
    new = [0] * n_headers
    for s, w in cls.items():
        if len(s) == 1:
            new[s[0]] += w * ONE
            continue
        cs = [c[h] for h in s]
        d = sum(cs)
        q = np.floor((np.array(cs, dtype=np.float64) / np.float64(d)) * SCALE)
        tot = 0
        for h, x in zip(s, q):
            x = int(x)
            tot += x
            new[h] += w * x
        r = ONE - tot
        assert r >= 0, (s, r)
        top = min(s, key=lambda h: (-c[h], h))
        new[top] += w * r
    return new


def em(n_headers, group_w, lines, max_iters=1000, tol=1024, trace=None):
    assert max_iters >= 1
    cls, pairs = classes_of(n_headers, group_w, lines)
    if not cls:
        return [0] * n_headers, [0, 0, 0, 0, 0]
    total = sum(cls.values())
    assert total <= (1 << 31) - 1
    c = [ONE] * n_headers
    t, delta, conv = 0, 0, 0
    while t < max_iters:
        new = step(n_headers, cls, c)
        assert sum(new) == ONE * total
        delta = max(abs(a - b) for a, b in zip(new, c))
        c = new
        t += 1
        if trace is not None:
            trace.append((t, list(c), delta))
        if delta <= tol:
            conv = 1
            break
    return c, [t, pairs, len(cls), delta, conv]


def b6_groups(text):
    """the lines of a .b6 text as the abundance sees them: one group per distinct read name (column 1) of weight 1, headers numbered in
    strcmp (byte) order of column 2"""
    rows = [ln.split("\t") for ln in text.splitlines() if ln]
    headers = sorted({r[1] for r in rows}, key=lambda s: s.encode())
    hix = {h: i for i, h in enumerate(headers)}
    reads = {}
    lines = []
    for r in rows:
        g = reads.setdefault(r[0], len(reads))
        lines.append((g, hix[r[1]]))
    return headers, [1] * len(reads), lines, list(reads)


def table_text(headers, names, columns):
    """headers: names of the header numbers; names: sample names; columns: per sample a list of counts.  Dataset = the integer sum of the
    sample columns; rows with Dataset 0 are skipped; rows in byte order of the header"""
    out = ["#OTU ID\tDataset" + "".join("\t" + n for n in names)]
    for h in sorted(range(len(headers)), key=lambda i: headers[i].encode()):
        ds = sum(int(col[h]) for col in columns)
        if not ds:
            continue
        out.append(headers[h] + "".join("\t%.4f" % (np.float64(v) / SCALE) for v in [ds] + [int(col[h]) for col in columns]))
    return "\n".join(out) + "\n"


def random_case(seed, n_groups=600, n_used=60, n_headers=64):
    """600 groups on 60 of 64 headers (the last four are on no line): set sizes drawn from {1, 1, 2, 3, 5, 58}, one group on all 60, weights
    0 .. 3, header 7 in every set of more than one candidate (every class hits one cell), a tenth of the lines twice, the lines shuffled"""
    rng = np.random.default_rng(seed)
    hot = 7
    group_w = [int(x) for x in rng.integers(0, 4, size=n_groups)]
    lines = []
    for g in range(n_groups):
        size = n_used if g == 17 else int(rng.choice([1, 1, 2, 3, 5, 58]))
        s = set(int(x) for x in rng.choice(n_used, size=size, replace=False))
        if size > 1 and hot not in s:
            s.remove(next(iter(s)))
            s.add(hot)
        lines += [(g, h) for h in s]
    group_w[17] = 2
    dup = [lines[int(i)] for i in rng.choice(len(lines), size=len(lines) // 10, replace=False)]
    lines += dup
    order = rng.permutation(len(lines))
    return n_headers, group_w, [lines[int(i)] for i in order]


# the hand cases of the definition: (n_headers, group_w, lines)
# case 1: headers A, B, C; three reads on {A}, one on {B}, four on {A, B}, the last of them with its A line twice
CASE1 = (3, [1] * 8, [(0, 0), (1, 0), (2, 0), (3, 1), (4, 0), (4, 1), (5, 1), (5, 0), (6, 0), (6, 1), (7, 0), (7, 1), (7, 0)])
CASE2 = (3, [1], [(0, 0), (0, 1), (0, 2)])
CASE3 = (4, [5], [(0, 1), (0, 2), (0, 3)])
CASE4 = (2, [1, 1], [(0, 0), (1, 1)])
