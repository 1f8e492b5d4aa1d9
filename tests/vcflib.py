"""The model of the VCF tests: the definition of an indel allele (README "VCF output", include/burst_hip.h "Indel alleles") as a dictionary
count of allele runs over pilelib-style lines, and the bytes of OUT.vcf rendered from pilelib.pile's sites plus those alleles.  It shares
no code with the project.  TEST INFRASTRUCTURE ONLY.

A line is pilelib's: dict(header, pos, ops=[(length, one of "=XID")], query=codes, ref=callable position -> code, w=reads)."""
import pilelib

DEL, INS = 0, 1
MAX_INS = 15
VCF_LETTER = "NACGT" + "N" * 11      # A C G T for the codes 1 .. 4, N for every other code
HEAD = ('##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads observing the position">\n'
        '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads observing the position">\n'
        '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads per allele, reference first">\n')


def alleles(lines):
    """({(header, anchor, kind, n, codes): dict(count, ref=code of the anchor, deleted=reference codes of a Del)}, dict(events, end, adjacent,
    long)).  kind DEL: codes = (); kind INS: codes = the inserted query codes.  Python's tuple order of the keys is the defined order."""
    table, fig = {}, dict(events=0, end=0, adjacent=0, long=0)
    for ln in lines:
        p, j, ops = ln["pos"], 0, ln["ops"]
        for k, (n, op) in enumerate(ops):
            if op in "ID":
                if k == 0 or k == len(ops) - 1:
                    fig["end"] += 1
                elif ops[k - 1][1] in "ID":
                    fig["adjacent"] += 1
                elif op == "I" and n > MAX_INS:
                    fig["long"] += 1
                else:
                    fig["events"] += 1
                    codes = tuple(int(c) for c in ln["query"][j:j + n]) if op == "I" else ()
                    key = (ln["header"], p - 1, INS if op == "I" else DEL, n, codes)
                    ref, deleted = ln["ref"](p - 1), tuple(ln["ref"](p + t) for t in range(n)) if op == "D" else ()
                    a = table.get(key)
                    if a is None:
                        a = table[key] = dict(count=0, ref=ref, deleted=deleted)
                    assert (a["ref"], a["deleted"]) == (ref, deleted), "lanes that share header positions must agree where an allele lies"
                    a["count"] += ln["w"]
            if op != "I":
                p += n
            if op != "D":
                j += n
    return table, fig


def returned(table, sites, min_depth, min_alt):
    """the rows (header, anchor, ref, depth, count, kind, n, codes, deleted) of the alleles that are returned, in the defined order; sites =
    pilelib.pile(lines) of the same lines"""
    rows = []
    for key in sorted(table):
        h, p, kind, n, codes = key
        a, depth = table[key], sum(sites[(h, p)]["n"])      # (every carrying line observes the anchor)
        assert a["count"] <= depth
        if depth >= min_depth and a["count"] >= min_alt:
            rows.append((h, p, a["ref"], depth, a["count"], kind, n, codes, a["deleted"]))
    return rows


def word(kind, n, codes):
    """the 64-bit allele word: Del(n) = n; Ins = n << 60 | c1 << 56 | c2 << 52 ..."""
    if kind == DEL:
        return n
    w = n << 60
    for t, c in enumerate(codes):
        w |= c << (56 - 4 * t)
    return w


def snvs(sites, min_depth, min_alt):
    """the rows (header, pos, ref, depth, n[ref], [(base 0..3, n)]) of the SNV records, ascending (header, pos)"""
    rows = []
    for (h, p) in sorted(sites):
        s = sites[(h, p)]
        depth = sum(s["n"])
        if not 1 <= s["ref"] <= 4 or depth < min_depth:
            continue
        alts = [(b, s["n"][b]) for b in range(4) if b != s["ref"] - 1 and s["n"][b] >= min_alt]
        if alts:
            rows.append((h, p, s["ref"], depth, s["n"][s["ref"] - 1], alts))
    return rows


def render(contigs, sample, lines, min_depth, min_alt, number=None):
    """the bytes of OUT.vcf.  contigs = [(SN, length)] in header-number order; number: header of a line -> its header number (default: the
    header IS the number).  Returns (bytes, dict(snv, del, ins))"""
    number = number or (lambda h: h)
    sites = pilelib.pile(lines)
    table, _ = alleles(lines)
    recs = []
    for h, p, ref, depth, nref, alts in snvs(sites, min_depth, min_alt):
        recs.append(((number(h), p, 0), "%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d\tDP:AD\t%d:%s" % (
            contigs[number(h)][0], p, VCF_LETTER[ref], ",".join("ACGT"[b] for b, _ in alts), depth, depth, ",".join(str(x) for x in [nref] + [n for _, n in alts]))))
    count = dict(snv=len(recs), ins=0)
    count["del"] = 0
    for k, (h, p, ref, depth, cnt, kind, n, codes, deleted) in enumerate(returned(table, sites, min_depth, min_alt)):
        a = VCF_LETTER[ref]
        if kind == DEL:
            REF, ALT = a + "".join(VCF_LETTER[c] for c in deleted), a
            count["del"] += 1
        else:
            REF, ALT = a, a + "".join(VCF_LETTER[c] for c in codes)
            count["ins"] += 1
        recs.append(((number(h), p, 1 + k), "%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d\tDP:AD\t%d:%d,%d" % (contigs[number(h)][0], p, REF, ALT, depth, depth, depth - cnt, cnt)))
    out = ["##fileformat=VCFv4.2\n##source=burst_hip\n"]
    out += ["##contig=<ID=%s,length=%d>\n" % c for c in contigs]
    out.append(HEAD)
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % sample)
    out += [text + "\n" for _, text in sorted(recs, key=lambda r: r[0])]
    return "".join(out).encode(), count
