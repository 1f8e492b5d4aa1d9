#!/usr/bin/env python3
"""QUICK against the compressive build (-d DNA) on a database of bench.py's `strains` profile, scaled down: 70 % of the content as
base sequences with --n-variants variants at --variant-rate, 30 % in families of 60 / 200 / 500 strains at 1 / 0.5 / 0.1 % divergence.
Prints one JSON line: unique fragments (totR / origTotR), clumps and .edx bytes of both layouts.

  python tools/dna_redundancy.py --n-base 20000 [--workdir /tmp/dna_red]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from burst_amd import host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-base", type=int, default=20000)
ap.add_argument("--n-variants", type=int, default=2)
ap.add_argument("--ref-len", type=int, default=1400)
ap.add_argument("--variant-rate", type=float, default=0.05)
ap.add_argument("--workdir", default="/tmp/dna_redundancy")
ap.add_argument("--cmd", default="-d {mode} 110 -s 500 -i 0.98")
a = ap.parse_args()
os.makedirs(a.workdir, exist_ok=True)
parts = []
seqs = a.n_base * a.n_variants
pairs = int(a.n_base * 0.7)
parts.append((0, pairs, a.n_variants, a.variant_rate, 7))
first = a.n_base
for nv, rate, seed in ((60, 0.01, 11), (200, 0.005, 12), (500, 0.001, 13)):
    n = max(1, int(seqs * 0.1 / nv))
    parts.append((first, n, nv, rate, seed))
    first += n + 8
fa = os.path.join(a.workdir, "strains.fa")
with open(fa, "wb") as out:
    for i, (b0, nb, nv, rate, seed) in enumerate(parts):
        p = fa + ".%d" % i
        host.synth_refs(p, nb, nv, a.ref_len, rate, seed, first_base=b0)
        out.write(open(p, "rb").read())
        os.remove(p)
res = {"fasta_bytes": os.path.getsize(fa), "parts": parts}
for mode in ("QUICK", "DNA"):
    edx = os.path.join(a.workdir, mode + ".edx")
    t = time.time()
    r = subprocess.run([os.path.join(ROOT, "burst_amd", "burst_hip"), "-r", fa, "-o", edx] + a.cmd.format(mode=mode).split(),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.exit(r.stdout[-2000:])
    m = re.search(r"Database written: (\d+) refs \[(\d+) orig\], (\d+) clumps", r.stdout)
    res[mode] = {"totR": int(m.group(1)), "origTotR": int(m.group(2)), "clumps": int(m.group(3)), "edx_bytes": os.path.getsize(edx),
                 "wall_s": round(time.time() - t, 2), "marks": [ln.strip() for ln in r.stdout.splitlines() if "duplicate marks" in ln]}
print(json.dumps(res))
