"""The definition of burst_hip --mates, restated (README "Paired-end reads").  Shares nothing with the product.

A placement is one .b6 line of a single-end run: read (column 1), header (column 2), st / ed (columns 9 and 10, signed 32-bit), edits
(column 11), its bytes and its position in the output.  It is reverse when st > ed.  A combination is a line a of mate 1 and a line b of
its mate 2 with byte-equal column 2; join() decides which are concordant by brute force (every a against every b of its pair) and
paired_text() turns two .b6 texts into the paired output."""
from collections import namedtuple

ORIENTATIONS = ("fr", "rf", "ff")
REPORTS = ("all", "best")

Line = namedtuple("Line", "pair ref st ed edits")


def _lo_hi(l):
    return (l.st, l.ed) if l.st <= l.ed else (l.ed, l.st)


def fragment(a, b, orientation):
    """(leftmost position, fragment length) of the combination if its orientation and order are acceptable, else None; the insert
    bounds are not looked at here"""
    ra, rb = a.st > a.ed, b.st > b.ed
    if orientation == "ff":
        if ra != rb:
            return None
        up, down = (a, b) if not ra else (b, a)
    else:
        if ra == rb:
            return None
        fwd, rev = (a, b) if rb else (b, a)
        up, down = (fwd, rev) if orientation == "fr" else (rev, fwd)
    ulo, uhi = _lo_hi(up)
    dlo, dhi = _lo_hi(down)
    if not (ulo <= dlo and uhi <= dhi):
        return None
    return ulo, dhi - ulo + 1


def concordant(a, b, orientation, ins_min, ins_max):
    f = fragment(a, b, orientation)
    return f is not None and ins_min <= f[1] <= ins_max


def join(a, b, orientation="fr", ins_min=0, ins_max=1000, report="all"):
    """a, b: sequences of Line (or 5-tuples pair, ref, st, ed, edits).  Returns the reported combinations as a list of (index in a,
    index in b), ascending"""
    assert orientation in ORIENTATIONS and report in REPORTS and ins_min <= ins_max
    a = [Line(*(int(v) for v in x)) for x in a]
    b = [Line(*(int(v) for v in x)) for x in b]
    by_pair = {}
    for j, lb in enumerate(b):
        by_pair.setdefault(lb.pair, []).append(j)
    combos = []
    for i, la in enumerate(a):
        for j in by_pair.get(la.pair, ()):
            if b[j].ref == la.ref and concordant(la, b[j], orientation, ins_min, ins_max):
                combos.append((i, j))
    if report == "all":
        return combos
    best = {}
    for i, j in combos:
        k = (min(a[i].edits + b[j].edits, 0xFFFFFFFF), i, j)
        if a[i].pair not in best or k < best[a[i].pair]:
            best[a[i].pair] = k
    return sorted((i, j) for _, i, j in best.values())


def examined(a, b):
    """combinations looked at: pairs of lines with equal (pair, ref)"""
    n = {}
    for x in b:
        n[(int(x[0]), int(x[1]))] = n.get((int(x[0]), int(x[1])), 0) + 1
    return sum(n.get((int(x[0]), int(x[1])), 0) for x in a)


# ---- .b6 text ----

def pair_name(read):
    return read[:-2] if read.endswith(b"/1") or read.endswith(b"/2") else read


def _s32(text):
    v = int(text) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def parse_b6(text):
    """[(read, header, st, ed, edits, line bytes without the newline)] in output order"""
    out = []
    for ln in text.split(b"\n"):
        if not ln:
            continue
        c = ln.split(b"\t")
        out.append((c[0], c[1], _s32(c[8]), _s32(c[9]), int(c[10]), ln))
    return out


def number_lines(p1, p2):
    """the two parsed outputs as Line arrays with dense pair and header numbers"""
    pairs, refs = {}, {}
    def conv(p):
        return [Line(pairs.setdefault(pair_name(r), len(pairs)), refs.setdefault(h, len(refs)), st, ed, e) for r, h, st, ed, e, _ in p]
    return conv(p1), conv(p2)


def paired_text(b6_1, b6_2, orientation="fr", ins_min=0, ins_max=1000, report="all", joiner=join):
    """the output of --mates for the single-end outputs b6_1 (mate 1) and b6_2 (mate 2): per reported combination a's line and b's line,
    each followed by the fragment's leftmost position and its length"""
    p1, p2 = parse_b6(b6_1), parse_b6(b6_2)
    a, b = number_lines(p1, p2)
    out = []
    for i, j in joiner(a, b, orientation, ins_min, ins_max, report):
        left, length = fragment(a[i], b[j], orientation)
        tail = b"\t%d\t%d\n" % (left, length)
        out.append(p1[i][5] + tail)
        out.append(p2[j][5] + tail)
    return b"".join(out)


def counts(b6_1, b6_2, names1, names2, orientation="fr", ins_min=0, ins_max=1000, report="all"):
    """the figures of the `Mates:` line.  names1 / names2: the read names of the two query files as column 1 would print them"""
    p1, p2 = parse_b6(b6_1), parse_b6(b6_2)
    a, b = number_lines(p1, p2)
    n1, n2 = {pair_name(n) for n in names1}, {pair_name(n) for n in names2}
    placed1, placed2 = {pair_name(x[0]) for x in p1}, {pair_name(x[0]) for x in p2}
    return dict(reads1=len(names1), reads2=len(names2), named=len(n1 & n2), placed=len(placed1 & placed2 & n1 & n2),
                examined=examined(a, b), written=len(join(a, b, orientation, ins_min, ins_max, report)))
