"""The pair files of the --mates tests, generated from tests/golden/refs.fa (the references behind tests/golden/dna.edx): fragments of
250-700 bases from the references of at least 800, mate 1 = the first 100 bases, mate 2 = the reverse complement of the last 100, 0-3
substitutions per mate, half the fragments from the reverse strand -- plus the cases that must NOT pair (other family, fragment beyond
the insert bound the tests pass, wrong orientation, no partner) and pairs that repeat another pair's sequences under new names."""
import os

import numpy as np

import goldenlib as gl

INSERT_MAX = 600      # what the tests pass as --insert-max: the `long` pairs below lie beyond it
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP.get(c, "N") for c in reversed(s))


def read_refs():
    names, seqs = [], []
    for ln in open(os.path.join(gl.G, "refs.fa")):
        if ln.startswith(">"):
            names.append(ln[1:].strip())
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return names, ["".join(s) for s in seqs]


def mutate(s, k, rng):
    s = list(s)
    for p in rng.choice(len(s), size=k, replace=False):
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] if s[p] in "ACGT" else "A"
    return "".join(s)


def make_pairs(seed=20):
    """[(kind, name, mate 1 or None, mate 2 or None)]"""
    rng = np.random.default_rng(seed)
    names, seqs = read_refs()
    big = [i for i, s in enumerate(seqs) if len(s) >= 800]
    fam = lambda i: names[i].split("_")[0]

    def frag(lo, hi, ref=None):
        i = int(rng.choice(big)) if ref is None else ref
        n = int(rng.integers(lo, min(hi, len(seqs[i])) + 1))
        p = int(rng.integers(0, len(seqs[i]) - n + 1))
        f = seqs[i][p:p + n]
        return i, (revcomp(f) if rng.integers(0, 2) else f)

    ends = lambda f: (mutate(f[:100], int(rng.integers(0, 4)), rng), mutate(revcomp(f[-100:]), int(rng.integers(0, 4)), rng))
    out = []
    for k in range(300):
        out.append(("proper", "p%03d" % k) + ends(frag(250, 700)[1]))
    for k in range(30):      # mates from different families
        i, f = frag(250, 700)
        j = int(rng.choice([x for x in big if fam(x) != fam(i)]))
        out.append(("families", "x%03d" % k, ends(f)[0], ends(frag(250, 700, j)[1])[1]))
    for k in range(30):      # a fragment longer than the insert bound
        out.append(("long", "l%03d" % k) + ends(frag(INSERT_MAX + 50, 780)[1]))
    for k in range(20):      # mate 2 not reverse-complemented
        m1, m2 = ends(frag(250, 700)[1])
        out.append(("orientation", "o%03d" % k, m1, revcomp(m2)))
    for k in range(20):      # no partner in file 2
        out.append(("alone", "s%03d" % k, ends(frag(250, 700)[1])[0], None))
    for k in range(20):      # another pair's sequences under a new name
        src = out[int(rng.integers(0, 300))]
        out.append(("repeat", "d%03d" % k, src[2], src[3]))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def write_files(d, seed=20):
    """writes m1.fa and m2.fa into directory d; half the pairs carry /1 and /2.  Returns (path 1, path 2, pairs)"""
    pairs = make_pairs(seed)
    p1, p2 = os.path.join(str(d), "m1.fa"), os.path.join(str(d), "m2.fa")
    with open(p1, "w") as f1, open(p2, "w") as f2:
        for k, (_, name, m1, m2) in enumerate(pairs):
            s1, s2 = ("/1", "/2") if k % 2 else ("", "")
            if m1 is not None:
                f1.write(">%s%s\n%s\n" % (name, s1, m1))
            if m2 is not None:
                f2.write(">%s%s\n%s\n" % (name, s2, m2))
    return p1, p2, pairs


def names_of(path):
    """read names as column 1 prints them (up to the first blank)"""
    return [ln[1:].split()[0].encode() for ln in open(path) if ln.startswith(">")]
