"""The chimera check of burst_hip --chimeras (include/burst_hip.h) as a model.  Works from (weights, lens, lines, ops) and
from .b6 TEXT with the --cigar columns; writes the table's text."""
import re

import numpy as np

OP = {"I": 1, "D": 2, "=": 7, "X": 8}
OP_CHAR = {v: k for k, v in OP.items()}


def ops_of(cigar):
    """CIGAR text in =XID -> op words length << 4 | code"""
    out = [int(n) << 4 | OP[c] for n, c in re.findall(r"([0-9]+)([=XID])", cigar)]
    assert "".join("%d%s" % (w >> 4, OP_CHAR[w & 15]) for w in out) == cigar, cigar
    return out


def positions(words, length, reverse):
    """the doubled edit positions of a path in read orientation, ascending"""
    pos, j = [], 0
    for w in words:
        run, code = int(w) >> 4, int(w) & 15
        if code == OP["D"]:
            pos += [2 * j] * run
        elif code == OP["="]:
            j += run
        else:
            pos += [2 * (j + t) + 1 for t in range(run)]
            j += run
    assert j == length, (j, length)
    if reverse:
        pos = [2 * length - p for p in reversed(pos)]
    assert pos == sorted(pos)
    return pos


def chimera(weights, lens, lines, ops, skew=2, min_seg=16, min_gain=3):
    """lines: rows (q, r, flags, n_ops, op_off), raw -> (rows [(role, single, model, cut, a, ea, b, eb)] per node, pairs kept)"""
    n = len(weights)
    order = sorted(range(n), key=lambda i: (-int(weights[i]), i))
    rank = {node: p for p, node in enumerate(order)}
    best = {}                                            # (q, r) -> (edits, input index)
    for i, (q, r, flags, n_ops, off) in enumerate(lines):
        q, r = int(q), int(r)
        if q == r or int(weights[r]) < int(skew) * int(weights[q]):
            continue
        words = ops[int(off):int(off) + int(n_ops)]
        e = sum(int(w) >> 4 for w in words if int(w) & 15 != OP["="])
        if (q, r) not in best or (e, i) < best[(q, r)]:
            best[(q, r)] = (e, i)
    per = {}
    for (q, r), (e, i) in best.items():
        per.setdefault(q, []).append((r, e, i))
    rows = [(0,) * 8] * n
    for q, lst in per.items():
        m = int(lens[q])
        if len(lst) < 2 or m < 2 * min_seg:
            continue
        cuts = np.arange(min_seg, m - min_seg + 1, dtype=np.int64)
        big = np.int64(1) << 62
        bl, br = np.full(len(cuts), big), np.full(len(cuts), big)
        for r, e, i in lst:
            _, _, flags, n_ops, off = lines[i]
            pos = np.array(positions(ops[int(off):int(off) + int(n_ops)], m, int(flags) & 1), dtype=np.int64)
            assert len(pos) == e
            left = np.searchsorted(pos, 2 * cuts, side="right").astype(np.int64)
            bl = np.minimum(bl, left << 32 | rank[r])
            br = np.minimum(br, (e - left) << 32 | rank[r])
        model = (bl >> 32) + (br >> 32)
        k = int(np.argmin(model))                        # (the first of the smallest: the smallest cut)
        single = min(e for _, e, _ in lst)
        a, ea, b, eb = order[int(bl[k]) & 0xFFFFFFFF], int(bl[k]) >> 32, order[int(br[k]) & 0xFFFFFFFF], int(br[k]) >> 32
        role = 2 if single - int(model[k]) >= min_gain else 1
        assert role != 2 or a != b
        rows[q] = (role, single, int(model[k]), int(cuts[k]), a, ea, b, eb)
    return rows, len(best)


def weight_of(name, sizes):
    m = re.search(r";size=([0-9]+);?$", name) if sizes else None
    return int(m.group(1)) if m else 1


def from_b6(names, text, sizes=False):
    """reads' names in file order, .b6 text with the --cigar columns -> (weights, lens, lines, ops, printed lines, foreign lines); the
    length of a read is column 8 of its lines (a read without lines is never evaluated: 0)"""
    node = {nm: i for i, nm in enumerate(names)}
    assert len(node) == len(names)
    lens, lines, ops, printed, foreign = [0] * len(names), [], [], 0, 0
    for ln in text.splitlines():
        if not ln:
            continue
        col = ln.split("\t")
        assert len(col) >= 14, "the --cigar columns are missing"
        printed += 1
        q = node[col[0]]
        lens[q] = int(col[7])
        if col[1] not in node:
            foreign += 1
            continue
        words = ops_of(col[-1])
        assert sum(w >> 4 for w in words if w & 15 != OP["="]) == int(col[10])      # E equals column 11
        lines.append((q, node[col[1]], 1 if int(col[8]) > int(col[9]) else 0, len(words), len(ops)))
        ops += words
    return [weight_of(nm, sizes) for nm in names], lens, lines, ops, printed, foreign


def table(names, weights, rows):
    """the text of PREFIXchimeras.txt"""
    t = "#Read\tRole\tSingle\tModel\tCut\tParentA\tEditsA\tParentB\tEditsB\tWeight\n"
    for nm, w, (role, single, model, cut, a, ea, b, eb) in zip(names, weights, rows):
        if not role:
            t += "%s\t-\t0\t0\t0\t*\t0\t*\t0\t%d\n" % (nm, w)
        else:
            t += "%s\t%s\t%d\t%d\t%d\t%s\t%d\t%s\t%d\t%d\n" % (nm, "-NY"[role], single, model, cut, names[a], ea, names[b], eb, w)
    return t


def table_from_b6(names, text, sizes=False, **par):
    w, lens, lines, ops, _, _ = from_b6(names, text, sizes)
    rows, _ = chimera(w, lens, lines, ops, **par)
    return table(names, w, rows)


def rows_of(arr):
    """a capi.CHIMERA_DTYPE array as the model's list of tuples"""
    return [tuple(int(x) for x in r) for r in arr.tolist()]


def read_fasta_names(path):
    return [ln[1:].split()[0] for ln in open(path) if ln.startswith(">")]
