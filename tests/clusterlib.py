"""The clustering definition of burst_hip --cluster (include/burst_hip.h) as a model: sort by priority, walk.  Works from
(weights, edges) and from .b6 text."""
import re


def cluster(weights, edges):
    """weights[node], edges (q, r, edits) raw -> (centroid[node], edits[node]); a centroid names itself with 0 edits"""
    n = len(weights)
    order = sorted(range(n), key=lambda i: (-int(weights[i]), i))
    rank = {node: p for p, node in enumerate(order)}
    best = {}                                            # (q, r) -> smallest edits
    for q, r, e in edges:
        q, r, e = int(q), int(r), int(e)
        if q != r:
            best[(q, r)] = min(e, best.get((q, r), e))
    out = {}
    for (q, r), e in best.items():
        out.setdefault(q, []).append((e, rank[r], r))
    centroid, edits, is_centroid = [0] * n, [0] * n, [False] * n
    for q in order:
        cands = [c for c in out.get(q, []) if c[1] < rank[q] and is_centroid[c[2]]]
        if cands:
            e, _, r = min(cands)                         # fewest edits, then the centroid that came first
            centroid[q], edits[q] = r, e
        else:
            centroid[q], is_centroid[q] = q, True
    return centroid, edits


def weight_of(name, sizes):
    m = re.search(r";size=([0-9]+);?$", name) if sizes else None
    return int(m.group(1)) if m else 1


def from_b6(names, text, sizes=False):
    """reads' names in file order, .b6 text -> (weights, edges, lines, foreign)"""
    node = {nm: i for i, nm in enumerate(names)}
    assert len(node) == len(names)
    edges, lines, foreign = [], 0, 0
    for ln in text.splitlines():
        if not ln:
            continue
        col = ln.split("\t")
        lines += 1
        if col[1] not in node:
            foreign += 1
        elif node[col[1]] != node[col[0]]:
            edges.append((node[col[0]], node[col[1]], int(col[10])))
    return [weight_of(nm, sizes) for nm in names], edges, lines, foreign


def tables(names, weights, centroid, edits):
    """the text of PREFIXclusters.txt and PREFIXcluster_sizes.txt"""
    a = "#Read\tCentroid\tRole\tEdits\tWeight\n"
    reads, wsum = {}, {}
    for i, nm in enumerate(names):
        c = centroid[i]
        a += "%s\t%s\t%s\t%d\t%d\n" % (nm, names[c], "C" if c == i else "M", edits[i], weights[i])
        reads[c] = reads.get(c, 0) + 1
        wsum[c] = wsum.get(c, 0) + int(weights[i])
    b = "#OTU ID\tReads\tWeight\n"
    for c in sorted(reads, key=lambda i: (-int(weights[i]), i)):
        b += "%s\t%d\t%d\n" % (names[c], reads[c], wsum[c])
    return a, b


def tables_from_b6(names, text, sizes=False):
    w, e, _, _ = from_b6(names, text, sizes)
    c, d = cluster(w, e)
    return tables(names, w, c, d)


def read_fasta_names(path):
    return [ln[1:].split()[0] for ln in open(path) if ln.startswith(">")]
