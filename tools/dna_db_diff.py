#!/usr/bin/env python3
"""Differential runner of the compressive build (-d DNA) against the compiled reference (oracle/_ref/burst12, -t 1):
a seeded strain-family FASTA, one reference run and one burst_hip run with the same arguments, the .edx compared byte for byte
and the .acx by sha256.  Exit status 0 = identical.

  python tools/dna_db_diff.py --seed 3 --families 6 --variants 5 --length 1500 --rate 0.004 -- -d DNA 120 -s 200 -i 0.97 [-dp 2]
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from burst_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "burst12")
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")


def make_fasta(path, seed, families, variants, length, rate, repeats):
    rng = np.random.default_rng(seed)
    seqs, names = [], []
    for f in range(families):
        base = rng.integers(1, 5, size=int(rng.integers(length // 2, length * 3 // 2)), dtype=np.uint8)
        if repeats and f % 3 == 0:      # a tandem repeat inside the family's base: chains of equal windows
            at = int(rng.integers(0, len(base) // 2))
            unit = rng.integers(1, 5, size=int(rng.integers(1, 8)), dtype=np.uint8)
            base = np.concatenate([base[:at], np.tile(unit, length // len(unit)), base[at:]])
        for v, s in enumerate(synth.mutate_family(base, variants, rate, rng)):
            seqs.append(s)
            names.append("f%d_v%d" % (f, v))
    synth.write_fasta(path, seqs, names)


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--families", type=int, default=6)
    ap.add_argument("--variants", type=int, default=5)
    ap.add_argument("--length", type=int, default=1500)
    ap.add_argument("--rate", type=float, default=0.004)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--fasta", help="use this FASTA instead of a synthetic one")
    ap.add_argument("--no-acx", action="store_true")
    ap.add_argument("args", nargs=argparse.REMAINDER)
    a = ap.parse_args()
    args = [x for x in a.args if x != "--"] or ["-d", "DNA", "120", "-s", "200", "-i", "0.97"]
    if not os.path.exists(REF):
        sys.exit("no compiled reference at %s" % REF)
    with tempfile.TemporaryDirectory() as d:
        fa = a.fasta or os.path.join(d, "in.fa")
        if not a.fasta:
            make_fasta(fa, a.seed, a.families, a.variants, a.length, a.rate, a.repeats)
        outs = {}
        for tag, exe in (("ref", [REF, "-t", "1"]), ("hip", [CLI])):
            edx, acx = os.path.join(d, tag + ".edx"), os.path.join(d, tag + ".acx")
            cmd = exe + ["-r", fa, "-o", edx] + ([] if a.no_acx else ["-a", acx]) + args
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode:
                print(r.stdout[-3000:])
                sys.exit("%s failed (%d): %s" % (tag, r.returncode, " ".join(cmd)))
            marks = [ln.strip() for ln in r.stdout.splitlines() if "duplicate marks computed" in ln]
            outs[tag] = (open(edx, "rb").read(), None if a.no_acx else sha(acx), marks)
        same_edx = outs["ref"][0] == outs["hip"][0]
        same_acx = outs["ref"][1] == outs["hip"][1]
        print("dna_db_diff: %s; edx %s (%d bytes), acx %s; %s" % (" ".join(args), "identical" if same_edx else "DIFFERENT", len(outs["ref"][0]),
              "identical" if same_acx else "DIFFERENT", "; ".join(outs["hip"][2])))
        sys.exit(0 if same_edx and same_acx else 1)


if __name__ == "__main__":
    main()
