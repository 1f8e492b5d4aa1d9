"""The model of the variants tests: the definition of a variant site (README "Variant sites", include/burst_hip.h) as a dictionary count
over every observed base.  It shares no code with the project: a line is plain Python data, the counts live in a dict keyed by
(header, position).  TEST INFRASTRUCTURE ONLY.

A line = dict(header=..., pos=int (1-based), ops=[(length, one of "=XID")], query=sequence of symbol codes, ref=callable position -> code
(the reference code at a 1-based position of the header, as the line's own lane holds it), w=int reads).  Symbol codes are
.ACGTNKMRYSWBVHD = 0..15."""
import re

LETTERS = ".ACGTNKMRYSWBVHD"
CODE = {c: i for i, c in enumerate(LETTERS)}
CODE.update({c.lower(): i for i, c in enumerate(LETTERS) if c != "."})
CODE["U"] = CODE["u"] = 4
A, C, G, T, DEL, OTHER = range(6)
HEADER_LINE = "#Reference\tPosition\tRef\tSample\tDepth\tA\tC\tG\tT\tDel\tOther\tIns\n"


def klass(code):
    return code - 1 if 1 <= code <= 4 else OTHER


def pile(lines):
    """every site any line observes: {(header, pos): dict(n=[A, C, G, T, Del, Other], ins=..., ref=smallest code seen, events=observations
    that are not plain plus insertion marks)}"""
    sites = {}

    def at(key, ref):
        s = sites.get(key)
        if s is None:
            s = sites[key] = dict(n=[0] * 6, ins=0, ref=ref, events=0)
        s["ref"] = min(s["ref"], ref)
        return s

    for ln in lines:
        p, j, w, ops = ln["pos"], 0, ln["w"], ln["ops"]
        assert p >= 1 and w >= 1
        for k, (n, op) in enumerate(ops):
            assert n >= 1
            if op == "I":
                j += n
                if 0 < k < len(ops) - 1:      # a run at an end of the path is what a local aligner would clip
                    s = sites[(ln["header"], p - 1)]      # (the column before an interior run was observed by this line)
                    s["ins"] += w
                    s["events"] += 1
            elif op == "D":
                for _ in range(n):
                    s = at((ln["header"], p), ln["ref"](p))
                    s["n"][DEL] += w
                    s["events"] += 1
                    p += 1
            else:
                assert op in "=X"
                for _ in range(n):
                    q = int(ln["query"][j])
                    s = at((ln["header"], p), ln["ref"](p))
                    s["n"][klass(q)] += w
                    if not (op == "=" and 1 <= q <= 4):
                        s["events"] += 1
                    p += 1
                    j += 1
        assert j == len(ln["query"]), "the ops do not consume the query"
    return sites


def reported(sites, min_depth, min_alt):
    """the rows (header, pos, ref, depth, A, C, G, T, Del, Other, ins) of the sites that are reported, ascending (header, pos)"""
    rows = []
    for (h, p) in sorted(sites):
        s = sites[(h, p)]
        depth = sum(s["n"])
        if not 1 <= s["ref"] <= 4 or depth < min_depth:
            continue
        if depth - s["n"][s["ref"] - 1] >= min_alt or s["ins"] >= min_alt:
            rows.append((h, p, s["ref"], depth) + tuple(s["n"]) + (s["ins"],))
    return rows


def figures(sites):
    """(events, candidate sites): what a count that skips plain observations has to sort, and the sites it has to look at"""
    return sum(s["events"] for s in sites.values()), sum(1 for s in sites.values() if s["events"])


def table(blocks):
    """the bytes of PREFIXvariants.txt: blocks = [(sample name, rows of reported() with the header as its NAME)] in study order; inside a
    block rows go by the bytes of the whole header, then by position"""
    out = [HEADER_LINE]
    for name, rows in blocks:
        for r in sorted(rows, key=lambda r: (r[0].encode(), r[1])):
            out.append("%s\t%d\t%s\t%s\t%s\n" % (r[0], r[1], LETTERS[r[2]], name, "\t".join(str(int(x)) for x in r[3:])))
    return "".join(out).encode()


def parse_cigar(text):
    items = re.findall(r"(\d+)([=XID])", text)
    assert items and "".join(a + b for a, b in items) == text, text
    return [(int(a), b) for a, b in items]


def read_fasta(path):
    """[(header line without '>', sequence)] of a FASTA file whose records may span lines"""
    recs, name, seq = [], None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(seq)))
                name, seq = line[1:], []
            elif name is not None:
                seq.append(line)
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs


def revcomp_codes(codes):
    comp = {0: 0, 1: 4, 2: 3, 3: 2, 4: 1, 5: 5, 6: 7, 7: 6, 8: 9, 9: 8, 10: 10, 11: 11, 12: 15, 13: 14, 14: 13, 15: 12}      # K<->M, R<->Y, B<->V, H<->D
    return [comp[c] for c in reversed(codes)]


def lines_of_b6(b6_text, refs, queries, unique_only=False):
    """the lines of one sample from its printed output with the two --cigar columns (position, CIGAR) at the end of every line.
    refs = {header: sequence}, queries = {read name: sequence}.  A reverse line (column 9 > column 10) shows the reverse complement of its
    read.  unique_only: only the lines whose read is on exactly one line of the output"""
    rows = [ln.split("\t") for ln in b6_text.split("\n") if ln]
    per_read = {}
    for r in rows:
        per_read[r[0]] = per_read.get(r[0], 0) + 1
    out = []
    for r in rows:
        if unique_only and per_read[r[0]] != 1:
            continue
        codes = [CODE.get(c, 0) for c in queries[r[0]]]
        if int(r[8]) > int(r[9]):
            codes = revcomp_codes(codes)
        seq = refs[r[1]]
        out.append(dict(header=r[1], pos=int(r[-2]), ops=parse_cigar(r[-1]), query=codes, w=1,
                        ref=lambda p, seq=seq: CODE.get(seq[p - 1], 0)))
    return out
