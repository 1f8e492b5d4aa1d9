"""An independent model of the consensus pairs (include/burst_hip.h "Consensus pairs"): dictionaries position -> byte per
(sample, header) and set intersections.  It shares no code with the C: nothing here sorts segments, builds an axis or counts bits.

rows: {(sample, header): {pos: byte}} -- every position a segment covers, N and ambiguity letters included."""
import numpy as np

COMPARABLE = frozenset(b"ACGT-")


def rows_of_segs(segs, letters):
    """segs: (sample, header, pos, len, off) tuples or a structured array with those fields; letters: bytes"""
    letters = bytes(letters)
    rows = {}
    for g in segs:
        sample, header, pos, ln, off = (int(g[k]) for k in ("sample", "header", "pos", "len", "off")) if not isinstance(g, tuple) else g
        row = rows.setdefault((sample, header), {})
        for t in range(ln):
            row[pos + t] = letters[off + t]
    return rows


def pairs(rows, min_compared=1):
    """[(header, a, b, compared, same)] ascending, the pairs with compared >= min_compared"""
    called = {k: {p: c for p, c in row.items() if c in COMPARABLE} for k, row in rows.items()}
    out = []
    for header in sorted({h for _, h in rows}):
        samples = sorted(s for s, h in rows if h == header)
        for i, a in enumerate(samples):
            for b in samples[i + 1:]:
                ra, rb = called[(a, header)], called[(b, header)]
                both = set(ra) & set(rb)
                same = sum(1 for p in both if ra[p] == rb[p])
                if len(both) >= min_compared:
                    out.append((header, a, b, len(both), same))
    return out


def info(rows, n_segs, n_pairs):
    """segments, headers with two samples or more, union positions of those headers, pairs examined, pairs returned"""
    headers, union, examined = 0, 0, 0
    for header in {h for _, h in rows}:
        samples = [s for s, h in rows if h == header]
        if len(samples) < 2:
            continue
        headers += 1
        examined += len(samples) * (len(samples) - 1) // 2
        union += len(set().union(*(set(rows[(s, header)]) for s in samples)))
    return (n_segs, headers, union, examined, n_pairs)


def pairs_array(ps):
    from burst_amd import capi
    a = np.zeros(len(ps), capi.PAIR_DTYPE)
    for i, (h, x, y, c, s) in enumerate(ps):
        a[i] = (h, x, y, 0, c, s)
    return a


def files(fa, names, failed=(), min_compared=1):
    """fa: the bytes of PREFIXconsensus.fa; names: the samples in study order; failed: the names of samples that failed alone ->
    (pairs.txt, identity.txt, compared.txt) as bytes"""
    index = {n: i for i, n in enumerate(names)}
    rows, length = {}, {}
    lines = fa.decode().split("\n")
    for k in range(0, len(lines) - 1, 2):
        assert lines[k].startswith(">")
        sample, header = lines[k][1:].split("|", 1)
        rows[(index[sample], header.encode())] = {p + 1: c for p, c in enumerate(lines[k + 1].encode())}
        assert length.setdefault(header.encode(), len(lines[k + 1])) == len(lines[k + 1])
    ps = pairs(rows, min_compared)      # (bytes sort as strcmp does)
    text = ["#Reference\tSampleA\tSampleB\tLength\tCompared\tSame\tDiffer\tIdentity\n"]
    n = len(names)
    sum_c, sum_s = [[0] * n for _ in range(n)], [[0] * n for _ in range(n)]
    for h, a, b, c, s in ps:
        text.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%.6f\n" % (h.decode(), names[a], names[b], length[h], c, s, c - s, s / c))
        for x, y in ((a, b), (b, a)):
            sum_c[x][y] += c
            sum_s[x][y] += s
    own = [sum(1 for (s, _), row in rows.items() if s == i for c in row.values() if c in COMPARABLE) for i in range(n)]
    ident, comp = ["#Identity" + "".join("\t" + x for x in names) + "\n"], ["#Compared" + "".join("\t" + x for x in names) + "\n"]
    for a in range(n):
        ci, cc = [names[a]], [names[a]]
        for b in range(n):
            if names[a] in failed or names[b] in failed:
                ci.append("NA"); cc.append("NA")
            elif a == b:
                ci.append("1.000000"); cc.append("%d" % own[a])
            elif sum_c[a][b]:
                ci.append("%.6f" % (sum_s[a][b] / sum_c[a][b])); cc.append("%d" % sum_c[a][b])
            else:
                ci.append("NA"); cc.append("0")
        ident.append("\t".join(ci) + "\n"); comp.append("\t".join(cc) + "\n")
    return "".join(text).encode(), "".join(ident).encode(), "".join(comp).encode()
