"""The model of the study-VCF tests: the definition of PREFIXstudy.vcf (README "Study VCF", include/burst_hip.h "Site counts") as dictionary
counts over pilelib-style lines per sample -- pilelib.pile's sites, vcflib's alleles -- and the bytes of the file rendered from them.  It
shares no code with the project.  TEST INFRASTRUCTURE ONLY.

A sample is a list of pilelib lines (dict(header, pos, ops, query, ref, w)), or None for a sample that failed alone."""
import pilelib
import vcflib

NS_LINE = '##INFO=<ID=NS,Number=1,Type=Integer,Description="Samples with a read observing the position">\n'


class Counts:
    """one sample's dictionary counts: Depth, n[b] and count(word) anywhere, 0 where the sample observes nothing"""
    def __init__(self, lines):
        self.sites = pilelib.pile(lines)
        self.table, _ = vcflib.alleles(lines)

    def depth(self, h, p):
        s = self.sites.get((h, p))
        return sum(s["n"]) if s else 0

    def n(self, h, p, b):
        s = self.sites.get((h, p))
        return s["n"][b] if s else 0

    def count(self, key):
        a = self.table.get(key)
        return a["count"] if a else 0


def records(counts, min_depth, min_alt):
    """{(header, pos, 0): dict(ref, alts=set of bases)} and {(header, pos, kind, n, codes): dict(ref, deleted)} of the records at least one
    sample reports; counts: a Counts per sample that did not fail"""
    snv, indel = {}, {}
    for c in counts:
        for h, p, ref, depth, nref, alts in vcflib.snvs(c.sites, min_depth, min_alt):
            r = snv.setdefault((h, p), dict(ref=ref, alts=set()))
            assert r["ref"] == ref
            r["alts"] |= {b for b, _ in alts}
        for h, p, ref, depth, cnt, kind, n, codes, deleted in vcflib.returned(c.table, c.sites, min_depth, min_alt):
            r = indel.setdefault((h, p, kind, n, codes), dict(ref=ref, deleted=deleted))
            assert (r["ref"], r["deleted"]) == (ref, deleted), "all reporting samples agree: the database is the same"
    return snv, indel


def render(contigs, names, samples, min_depth, min_alt, number=None):
    """the bytes of PREFIXstudy.vcf.  contigs = [(SN, length)] in header-number order; names: the column names in study order; samples: per
    name the sample's lines or None; number: header of a line -> its header number.  Returns (bytes, dict(snv, del, ins))"""
    number = number or (lambda h: h)
    counts = [None if s is None else Counts(s) for s in samples]
    live = [c for c in counts if c is not None]
    snv, indel = records(live, min_depth, min_alt)
    recs = []
    for (h, p), r in snv.items():
        alts = sorted(r["alts"])
        cols, dp, ns = [], 0, 0
        for c in counts:
            if c is None:
                cols.append(".")
                continue
            d = c.depth(h, p)
            dp, ns = dp + d, ns + (d >= 1)
            cols.append("%d:%s" % (d, ",".join(str(c.n(h, p, b)) for b in [r["ref"] - 1] + alts)))
        recs.append(((number(h), p, 0, 0), "%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;NS=%d\tDP:AD\t%s" % (
            contigs[number(h)][0], p, vcflib.VCF_LETTER[r["ref"]], ",".join("ACGT"[b] for b in alts), dp, ns, "\t".join(cols))))
    count = dict(snv=len(recs), ins=0)
    count["del"] = 0
    for key, r in indel.items():
        h, p, kind, n, codes = key
        a = vcflib.VCF_LETTER[r["ref"]]
        if kind == vcflib.DEL:
            REF, ALT = a + "".join(vcflib.VCF_LETTER[c] for c in r["deleted"]), a
            count["del"] += 1
        else:
            REF, ALT = a, a + "".join(vcflib.VCF_LETTER[c] for c in codes)
            count["ins"] += 1
        cols, dp, ns = [], 0, 0
        for c in counts:
            if c is None:
                cols.append(".")
                continue
            d, k = c.depth(h, p), c.count(key)
            assert k <= d
            dp, ns = dp + d, ns + (d >= 1)
            cols.append("%d:%d,%d" % (d, d - k, k))
        recs.append(((number(h), p, 1, vcflib.word(kind, n, codes)), "%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;NS=%d\tDP:AD\t%s" % (contigs[number(h)][0], p, REF, ALT, dp, ns, "\t".join(cols))))
    head = vcflib.HEAD.split("\n")
    out = ["##fileformat=VCFv4.2\n##source=burst_hip\n"]
    out += ["##contig=<ID=%s,length=%d>\n" % c for c in contigs]
    out += [head[0] + "\n", NS_LINE, head[1] + "\n", head[2] + "\n"]
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % "\t".join(names))
    out += [text + "\n" for _, text in sorted(recs, key=lambda r: r[0])]
    return "".join(out).encode(), count


def project(study_bytes, column, min_depth, min_alt):
    """the body lines of the single-sample file that sample `column` (0-based) of a study file would have: the records it reports itself, ALT
    and AD cut down to its own alternatives, INFO DP its own depth"""
    out = []
    for ln in study_bytes.decode().split("\n"):
        if not ln or ln.startswith("#"):
            continue
        f = ln.split("\t")
        cell = f[9 + column]
        if cell == ".":
            continue
        dp, ad = cell.split(":")
        dp, ad, alts = int(dp), [int(x) for x in ad.split(",")], f[4].split(",")
        if dp < min_depth:
            continue
        if len(f[3]) == 1 and all(len(a) == 1 for a in alts):      # an SNV record
            keep = [k for k in range(len(alts)) if ad[1 + k] >= min_alt]
            if not keep:
                continue
            f[4], ad = ",".join(alts[k] for k in keep), [ad[0]] + [ad[1 + k] for k in keep]
        elif ad[1] < min_alt:
            continue
        out.append("\t".join(f[:7] + ["DP=%d" % dp, "DP:AD", "%d:%s" % (dp, ",".join(str(x) for x in ad))]))
    return out


# ---- the primitive: one sample's arrays for bhip_site_counts / bh_site_counts_host, and the cells the dictionaries give ------------------
def arrays(lines):
    """(ranges, sites, alleles) of one sample as plain tuples: ranges (header, pos, span, w); sites the pile_run(1, 1) rows (header, pos, ref,
    depth, n[6], ins); alleles the alleles_run(1, 1) rows (header, pos, word, ref, depth, count)"""
    c = Counts(lines)
    ranges = [(ln["header"], ln["pos"], sum(n for n, op in ln["ops"] if op != "I"), ln["w"]) for ln in lines]
    sites = [(r[0], r[1], r[2], r[3], tuple(r[4:10]), r[10]) for r in pilelib.reported(c.sites, 1, 1)]
    alleles = [(h, p, vcflib.word(kind, n, codes), ref, depth, cnt) for h, p, ref, depth, cnt, kind, n, codes, _ in vcflib.returned(c.table, c.sites, 1, 1)]
    return c, ranges, sites, alleles


def cell(c, record):
    """(depth, (nA, nC, nG, nT), count) of a record (header, pos, word, ref) from the dictionaries: a site record's plain observations are
    counted where they were made, never derived from the depth"""
    h, p, word, ref = record
    d = c.depth(h, p)
    if word == 0:
        return d, tuple(c.n(h, p, b) for b in range(4)), 0
    cnt = sum(a["count"] for (kh, kp, kind, n, codes), a in c.table.items() if (kh, kp) == (h, p) and vcflib.word(kind, n, codes) == word)
    return d, (0, 0, 0, 0), cnt
