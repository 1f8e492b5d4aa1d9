"""numpy restatement of the coverage definitions (README, --coverage) for the coverage tests: dense depth arrays per reference, the
integer statistics, and the five tables as text.  Independent of the product code: nothing here goes through burst_amd."""
import math
import os

import numpy as np

KINDS = ("shared.txt", "unique.txt", "shared_binary.txt", "unique_binary.txt", "counts.txt")


def read_lengths(path):
    """{header: length} of a `name<TAB>length` table"""
    out = {}
    for ln in open(path, "rb").read().splitlines():
        if ln:
            n, l = ln.rsplit(b"\t", 1)
            out[n.decode()] = int(l)
    return out


def parse_b6(path):
    """[(query name, header, column 9, column 10, unique)] of a .b6; unique: the query name is on exactly one line of the file"""
    rows = [ln.split(b"\t") for ln in open(path, "rb").read().splitlines() if ln]
    cnt = {}
    for r in rows:
        cnt[r[0]] = cnt.get(r[0], 0) + 1
    return [(r[0].decode(), r[1].decode(), int(r[8]), int(r[9]), cnt[r[0]] == 1) for r in rows]


def interval(st, ed, L, pad):
    lo, hi = min(st, ed), max(st, ed)
    return max(lo - 1 - pad, 0), min(hi - 1 + pad, L)


def dense_stats(ref, st, ed, w, uniq, lengths, pad=0):
    """(shared, unique) uint64 [headers][4] = tot, cov, sq, lines from per-position depth arrays (python integers: exact)"""
    nH = len(lengths)
    out = []
    for sel in (np.ones(len(ref), bool), np.asarray(uniq, bool)):
        res = np.zeros((nH, 4), np.uint64)
        for h in range(nH):
            L = int(lengths[h])
            d = np.zeros(L + 1, np.int64)
            m = sel & (np.asarray(ref) == h)
            for s, e, ww in zip(np.asarray(st)[m], np.asarray(ed)[m], np.asarray(w)[m]):
                b, t = interval(int(s), int(e), L, pad)
                if b < t:
                    d[b] += int(ww)
                    d[t] -= int(ww)
            depth = np.cumsum(d[:L])
            res[h] = (int(depth.sum()), int((depth != 0).sum()), int((depth.astype(object) ** 2).sum()) if L else 0, int(np.asarray(w)[m].sum()))
        out.append(res)
    return out[0], out[1]


def signed_mean(tot, sq, L):
    mean = tot / L
    if L == 1 or not tot:
        return mean
    return mean if mean > math.sqrt((sq - tot * tot / L) / (L - 1)) else -mean


def tables(headers, lengths, col_names, shared, unique):
    """{kind: bytes} of the five tables; shared / unique: [columns][headers][4], column 0 = Dataset; col_names: the samples'"""
    rows = sorted((h for h in range(len(headers)) if int(shared[0][h][0]) > 0), key=lambda h: headers[h].encode())
    out = {}
    for kind in KINDS:
        t = ["\t".join(["#OTU ID" if kind == "counts.txt" else "#Coverage", "Dataset"] + list(col_names))]
        for h in rows:
            L = int(lengths[h])
            cells = []
            for c in range(len(shared)):
                a, b = [int(x) for x in shared[c][h]], [int(x) for x in unique[c][h]]
                if kind == "shared.txt":
                    cells.append("%.4f" % signed_mean(a[0], a[2], L))
                elif kind == "unique.txt":
                    cells.append("%.4f" % signed_mean(b[0], b[2], L))
                elif kind == "shared_binary.txt":
                    cells.append("%.4f" % (a[1] / L))
                elif kind == "unique_binary.txt":
                    cells.append("%.4f" % (b[1] / L))
                else:
                    cells.append("%d" % a[3])
            t.append("\t".join([headers[h]] + cells))
        out[kind] = ("\n".join(t) + "\n").encode()
    return out


def b6_columns(b6_paths, headers, lengths, pad=0):
    """the statistics of a study from its .b6 files: (shared, unique) [1 + samples][headers][4], Dataset = all files' lines together"""
    ix = {h: i for i, h in enumerate(headers)}
    per = []
    for p in b6_paths:
        rows = parse_b6(p) if p and os.path.exists(p) else []
        per.append((np.array([ix[r[1]] for r in rows], np.int64), np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64),
                    np.ones(len(rows), np.int64), np.array([r[4] for r in rows], bool)))
    cat = tuple(np.concatenate([x[k] for x in per]) for k in range(5))
    cols = [dense_stats(*cat, lengths, pad)] + [dense_stats(*x, lengths, pad) for x in per]
    return np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
