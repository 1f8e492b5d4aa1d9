"""The model of the consensus tests: the definition of README "Consensus" / include/burst_hip.h as a dictionary per (header, position),
built on pilelib.pile's sites -- which walk every observation, plain ones included, so the depth needs no trick.  Segments, letters,
figures and the bytes of both files.  It shares no code with the project.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import pilelib

REF_LETTERS = "NACGTNKMRYSWBVHD"
SEG_DTYPE = np.dtype([("header", "<u4"), ("pos", "<u4"), ("len", "<u4"), ("called", "<u4"), ("same", "<u4"), ("subst", "<u4"), ("del", "<u4"),
                      ("ambig", "<u4"), ("ins_major", "<u4"), ("pad", "<u4"), ("off", "<u8")])
FIGURES = ("called", "same", "subst", "del", "ambig", "ins_major")
TABLE_HEADER = "#Reference\tSample\tLength\tCovered\tCalled\tSame\tSubst\tDel\tAmbig\tInsMajor\tRecord\n"


def call(site, min_depth):
    """(letter, kind) of a covered position: kind is None (not called), "same", "subst", "del" or "ambig" """
    depth = sum(site["n"])
    assert depth >= 1
    if depth < min_depth:
        return "N", None
    ref = site["ref"]
    if not 1 <= ref <= 4:
        return REF_LETTERS[ref], "ambig"
    five = site["n"][:5]
    top = max(five)
    win = ref - 1 if five[ref - 1] == top else five.index(top)
    if win == ref - 1:
        return "ACGT"[win], "same"
    return ("ACGT-"[win], "del" if win == 4 else "subst")


def consensus(lines, min_depth, sites=None):
    """(segments, letters): segments = dicts of SEG_DTYPE's fields in ascending (header, pos) order, letters = one str; segment s owns
    letters[off : off + len]"""
    sites = pilelib.pile(lines) if sites is None else sites
    segs, letters = [], []
    cur = None
    for (h, p) in sorted(sites):
        s = sites[(h, p)]
        if cur is None or cur["header"] != h or cur["pos"] + cur["len"] != p:
            cur = dict(header=h, pos=p, len=0, called=0, same=0, subst=0, ambig=0, ins_major=0, pad=0, off=len(letters))
            cur["del"] = 0
            segs.append(cur)
        letter, kind = call(s, min_depth)
        letters.append(letter)
        cur["len"] += 1
        if kind:
            cur["called"] += 1
            cur[kind] += 1
            if 2 * s["ins"] > sum(s["n"]):
                cur["ins_major"] += 1
    for g in segs:
        assert g["called"] == g["same"] + g["subst"] + g["del"] + g["ambig"]
    return segs, "".join(letters)


def seg_bytes(segs):
    a = np.zeros(len(segs), SEG_DTYPE)
    for k, g in enumerate(segs):
        for name in SEG_DTYPE.names:
            a[name][k] = g[name]
    return a.tobytes()


def info(lines, segs, sites=None):
    """(events, candidate sites, segments, covered positions)"""
    sites = pilelib.pile(lines) if sites is None else sites
    return pilelib.figures(sites) + (len(segs), sum(g["len"] for g in segs))


class TooShort(Exception):
    """a segment ends beyond the length of its header (a usage error that names the header)"""


def files(samples, lengths, min_depth=4, min_breadth=0):
    """(bytes of PREFIXconsensus.fa, bytes of PREFIXconsensus.txt, rows): samples = [(sample name, lines whose header is the header's NAME,
    or None for a sample that failed alone)] in study order, lengths = {header name: L}.  rows = (header, sample, L, covered, called, same,
    subst, del, ambig, ins_major, record)"""
    fa, txt, rows = [], [TABLE_HEADER], []
    for name, lines in samples:
        if lines is None:
            continue
        segs, letters = consensus(lines, min_depth)
        by = {}
        for g in segs:
            by.setdefault(g["header"], []).append(g)
        for h in sorted(by, key=lambda h: h.encode()):
            L = lengths[h]
            fig = {f: sum(g[f] for g in by[h]) for f in FIGURES}
            covered = sum(g["len"] for g in by[h])
            rec = ["N"] * L
            for g in by[h]:
                if g["pos"] - 1 + g["len"] > L:
                    raise TooShort(h)
                rec[g["pos"] - 1:g["pos"] - 1 + g["len"]] = letters[g["off"]:g["off"] + g["len"]]
            record = int(fig["called"] >= 1 and 1000 * fig["called"] >= min_breadth * L)
            if record:
                fa.append(">%s|%s\n%s\n" % (name, h, "".join(rec)))
            row = (h, name, L, covered) + tuple(fig[f] for f in FIGURES) + (record,)
            rows.append(row)
            txt.append("\t".join(str(x) for x in row) + "\n")
    return "".join(fa).encode(), "".join(txt).encode(), rows
