"""The taxon tables' definition (include/burst_hip.h, bhip_taxa_run) once more, in plain Python integers: the tree of a list of
taxonomy strings, a group's taxon by counting its candidates below every ancestor, own and clade counts, the roll-up of counts per header,
and the text of the tables.  Groups come from .b6 text and a taxonomy map's text directly.  Nothing here touches the project's libraries."""
import numpy as np

NONE = 0xFFFFFFFF
MASK = (1 << 64) - 1


def levels_of(s):
    """the levels of a taxonomy string, None = no taxonomy"""
    s = s.rstrip(";")
    if s == "" or s == "Unassigned":
        return None
    return tuple(s.split(";"))


def tree_of(strings, reverse=False):
    """names, parent, depth in preorder and the node of every string; siblings in byte order of their level, or the reverse of it"""
    kids = {(): set()}
    for s in strings:
        lv = levels_of(s)
        for k in range(1, len(lv or ()) + 1):
            kids.setdefault(lv[:k - 1], set()).add(lv[:k])
            kids.setdefault(lv[:k], set())
    names, parent, depth, num = ["Unassigned"], [0], [0], {(): 0}
    stack = [iter(sorted(kids[()], key=lambda t: t[-1].encode(), reverse=reverse))]
    path = [0]
    while stack:
        nxt = next(stack[-1], None)
        if nxt is None:
            stack.pop()
            path.pop()
            continue
        num[nxt] = len(names)
        names.append(";".join(nxt))
        parent.append(path[-1])
        depth.append(len(nxt))
        path.append(num[nxt])
        stack.append(iter(sorted(kids[nxt], key=lambda t: t[-1].encode(), reverse=reverse)))
    return names, parent, depth, [num[levels_of(s) or ()] for s in strings]


def depths(parent):
    d = [0] * len(parent)
    for v in range(1, len(parent)):
        d[v] = d[parent[v]] + 1
    return d


def is_preorder(parent):
    if parent[0] != 0:
        return False
    for v in range(1, len(parent)):
        p, x = parent[v], v - 1
        if p >= v:
            return False
        while x > p:
            x = parent[x]
        if x != p:
            return False
    return True


def taxon(parent, depth, nodes, agree):
    """the deepest node whose subtree holds at least t of the candidates' nodes, counted ancestor by ancestor"""
    n = len(nodes)
    t = (agree * n + 999) // 1000
    cnt = {}
    for v in nodes:
        while True:
            cnt[v] = cnt.get(v, 0) + 1
            if v == 0:
                break
            v = parent[v]
    ok = [v for v, c in cnt.items() if c >= t]
    top = max(depth[v] for v in ok)
    best = [v for v in ok if depth[v] == top]
    assert len(best) == 1
    return best[0]


def clade_of(parent, own):
    clade = list(own)
    for v in range(len(parent) - 1, 0, -1):
        clade[parent[v]] = (clade[parent[v]] + clade[v]) & MASK
    return clade


def taxa(parent, header_node, group_w, lines, agree=1000):
    """(group_node, own, clade, info[0..4]) of the definition"""
    depth = depths(parent)
    cand = {}
    for g, h in lines:
        cand.setdefault(int(g), set()).add(int(h))
    group_node, own = [NONE] * len(group_w), [0] * len(parent)
    info = [sum(len(s) for s in cand.values()), len(cand), 0, 0, 0]
    for g, hs in cand.items():
        v = taxon(parent, depth, [int(header_node[h]) for h in hs], agree)
        group_node[g] = v
        own[v] += int(group_w[g])
        info[2] += int(group_w[g])
        info[4] = max(info[4], depth[v])
    info[3] = own[0]
    return group_node, own, clade_of(parent, own), info


def rollup(parent, header_node, counts):
    own = [0] * len(parent)
    for h, c in enumerate(counts):
        own[int(header_node[h])] = (own[int(header_node[h])] + int(c)) & MASK
    return own, clade_of(parent, own)


def read_map(text):
    """a taxonomy map's text as header -> string (the string ends at a further tab or a carriage return)"""
    m = {}
    for ln in text.split("\n"):
        if ln:
            head, tax = ln.split("\t", 1)
            m[head] = tax.split("\t")[0].split("\r")[0]
    return m


def b6_groups(text, tax_map):
    """the lines of a .b6 text as the tables see them: one group per distinct read name (column 1) of weight 1, the headers of column 2 in
    byte order, each with the map's string (absent: none): (headers, strings, group_w, lines, read names)"""
    rows = [ln.split("\t") for ln in text.splitlines() if ln]
    headers = sorted({r[1] for r in rows}, key=lambda s: s.encode())
    hix = {h: i for i, h in enumerate(headers)}
    reads, lines = {}, []
    for r in rows:
        lines.append((reads.setdefault(r[0], len(reads)), hix[r[1]]))
    return headers, [tax_map.get(h, "") for h in headers], [1] * len(reads), lines, list(reads)


def table_text(names, rows, sample_names, columns, em=False, keep_zero=False):
    """rows: node numbers; columns: per sample a list of counts per node.  Dataset = the integer sum of the sample columns, rows with
    Dataset 0 are skipped, rows in byte order of the name"""
    out = ["#OTU ID\tDataset" + "".join("\t" + n for n in sample_names)]
    for v in sorted(rows, key=lambda i: names[i].encode()):
        cells = [int(col[v]) for col in columns]
        cells = [sum(cells)] + cells
        if cells[0] or keep_zero:
            out.append(names[v] + "".join(("\t%.4f" % (np.float64(c) / np.float64(1 << 30))) if em else ("\t%d" % c) for c in cells))
    return "\n".join(out) + "\n"


def tables(names, depth, sample_names, own_cols, clade_cols, clade_em_cols=None):
    """suffix -> text of every file the writer leaves for these columns"""
    nodes = range(len(names))
    out = {"taxa.txt": table_text(names, nodes, sample_names, own_cols)}
    live = [v for v in nodes if sum(int(c[v]) for c in clade_cols)]      # the rows of the level files: a Dataset clade count
    for k in range(1, max([depth[v] for v in live] + [0]) + 1):
        rows = [v for v in live if depth[v] == k]
        out["taxa_L%d.txt" % k] = table_text(names, rows, sample_names, clade_cols)
        if clade_em_cols is not None:      # the same rows from the rolled-up abundance counts, a zero Dataset cell included
            out["taxa_abundance_L%d.txt" % k] = table_text(names, rows, sample_names, clade_em_cols, True, keep_zero=True)
    return out


# ---- random cases: a tree in two sibling orders ----
def random_parents(rng, n):
    """parent[v] < v, any shape, at most 64 levels (not a preorder numbering)"""
    par, dep = [0], [0]
    for v in range(1, n):
        p = int(rng.integers(0, v))
        while dep[p] >= 64:
            p = par[p]
        par.append(p)
        dep.append(dep[p] + 1)
    return par


def preorder(raw_parent, reverse=False):
    """(parent in preorder numbers, new number of every raw node); children in ascending raw number or the reverse"""
    n = len(raw_parent)
    kids = [[] for _ in range(n)]
    for v in range(1, n):
        kids[raw_parent[v]].append(v)
    new, order, stack = [0] * n, [], [0]
    while stack:
        v = stack.pop()
        new[v] = len(order)
        order.append(v)
        stack.extend(kids[v] if reverse else kids[v][::-1])      # (popped last first)
    return [new[raw_parent[v]] for v in order], new


def random_case(seed, n_nodes=200, n_headers=300, n_groups=250, max_cand=12):
    """a raw tree, raw nodes of the headers (a tenth at the root), groups of 1 .. max_cand candidates with a fifth of the lines twice,
    weights 0 .. 3, a few groups without lines, the lines shuffled"""
    rng = np.random.default_rng(seed)
    raw = random_parents(rng, n_nodes)
    hraw = [0 if rng.integers(0, 10) == 0 else int(rng.integers(0, n_nodes)) for _ in range(n_headers)]
    dfs = preorder(raw)[1]
    hraw.sort(key=lambda v: dfs[v])      # (neighbouring headers are relatives, as the references of one family are)
    gw = [int(x) for x in rng.integers(0, 4, size=n_groups)]
    lines = []
    for g in range(n_groups):
        if g % 37 == 5:
            continue
        # candidates drawn from a narrow window of headers half of the time, so that deep taxa occur
        lo = int(rng.integers(0, n_headers - 8))
        pool = np.arange(lo, lo + 8) if rng.integers(0, 2) else np.arange(n_headers)
        k = int(rng.integers(1, min(max_cand, len(pool)) + 1))
        lines += [(g, int(h)) for h in rng.choice(pool, size=k, replace=False)]
    lines += [lines[int(i)] for i in rng.choice(len(lines), size=len(lines) // 5, replace=False)]
    return raw, hraw, gw, [lines[int(i)] for i in rng.permutation(len(lines))]
