#!/usr/bin/env python3
"""Golden fixtures of the compressive build (-d DNA) from the COMPILED REFERENCE (oracle/_ref/burst12, built by oracle/Makefile).
Run where the reference is compiled:  python tests/golden/make_golden_dna.py

Writes, for small seeded inputs:
  dna_cases/<name>.fa        the input
  dna_cases/<name>.edx       the .edx the reference wrote with -t 1 (its sha256 in dna_cases.json instead when larger than 256 KiB)
  dna_cases.json             per case: the arguments, the .edx file or sha256, and the sha256 of the .acx (64 MiB, not committed)
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from burst_amd import synth  # noqa: E402

BURST12 = os.path.join(ROOT, "oracle", "_ref", "burst12")
OUT = os.path.join(HERE, "dna_cases")
TMP = "/tmp/burst_golden_dna"
LETTERS = synth.CODE2CHAR


def fasta(path, seqs, names, wrap=0, crlf=False, lower=False):
    nl = "\r\n" if crlf else "\n"
    with open(path, "w", newline="") as f:
        for s, n in zip(seqs, names):
            t = LETTERS[np.asarray(s, np.uint8)].tobytes().decode()
            if lower:
                t = t.lower()
            f.write(">" + n + nl)
            step = wrap or len(t) or 1
            for i in range(0, len(t), step):
                f.write(t[i:i + step] + nl)


def families(rng, n_fam, n_var, lo, hi, rate):
    seqs = []
    for _ in range(n_fam):
        base = rng.integers(1, 5, size=int(rng.integers(lo, hi)), dtype=np.uint8)
        seqs += synth.mutate_family(base, n_var, rate, rng)
    return seqs


def make_inputs():
    rng = np.random.default_rng(20261016)
    cases = {}
    fam = families(rng, 8, 4, 1500, 3000, 0.01)
    cases["fam"] = (fam, ["fam%02d strain" % i for i in range(len(fam))], {})
    # a homopolymer and a tandem repeat long enough for maxChain > 2048, beside families whose chains are short (t == 0)
    hp = np.concatenate([rng.integers(1, 5, 300, dtype=np.uint8), np.full(3200, 1, np.uint8), rng.integers(1, 5, 300, dtype=np.uint8)])
    tr = np.concatenate([rng.integers(1, 5, 200, dtype=np.uint8), np.tile(np.array([1, 2, 3, 4, 4, 2, 1], np.uint8), 500), rng.integers(1, 5, 200, dtype=np.uint8)])
    short = families(rng, 3, 4, 900, 1400, 0.01)
    cases["chain_t0"] = ([hp, tr] + short, ["homopolymer", "tandem"] + ["s%d" % i for i in range(len(short))], {})
    iu = families(rng, 4, 4, 1200, 2200, 0.01)
    for s in iu:
        m = np.flatnonzero(rng.random(len(s)) < 0.03)
        s[m] = rng.integers(5, 16, size=len(m))
        at = int(rng.integers(0, len(s) - 60))
        s[at:at + int(rng.integers(5, 60))] = 5
    cases["iupac"] = (iu, ["iu%d" % i for i in range(len(iu))], {})
    # W = 206 for `-d DNA 100 -s 30 -i 0.97`: lengths around it and below five symbols
    base = rng.integers(1, 5, 900, dtype=np.uint8)
    lens = [3, 4, 1, 205, 206, 207, 150, 206, 207, 900]
    ls = [base[:n].copy() for n in lens] + [base.copy(), base[:3].copy()]
    cases["lengths"] = (ls, ["len%d_%d" % (i, len(s)) for i, s in enumerate(ls)], {})
    cr = families(rng, 3, 3, 800, 1500, 0.02)
    cases["crlf"] = (cr, ["crlf%d" % i for i in range(len(cr))], {"wrap": 61, "crlf": True, "lower": True})
    return cases


# name -> (input, arguments after -r IN -o OUT [-a ACX])
RUNS = {
    "readme": ("fam", ["-d", "DNA", "320", "-s", "1", "-i", "0.97"]),
    "dp2": ("fam", ["-d", "DNA", "320", "-s", "500", "-i", "0.95", "-dp", "2"]),
    "dp3": ("fam", ["-d", "DNA", "320", "-s", "500", "-i", "0.95", "-dp", "3"]),
    "chain_t0": ("chain_t0", ["-d", "DNA", "100", "-s", "30", "-i", "0.97"]),
    "iupac": ("iupac", ["-d", "DNA", "150", "-s", "200", "-i", "0.97"]),
    "lengths": ("lengths", ["-d", "DNA", "100", "-s", "30", "-i", "0.97"]),
    "l0": ("fam", ["-d", "DNA", "200", "-s", "300", "-i", "0.97", "-l", "0"]),
    "y": ("iupac", ["-d", "DNA", "150", "-s", "200", "-i", "0.97", "-y"]),
    "crlf": ("crlf", ["-d", "DNA", "100", "-s", "100", "-i", "0.95"]),
}


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    if not os.path.exists(BURST12):
        raise SystemExit("build the reference first (oracle/Makefile)")
    os.makedirs(OUT, exist_ok=True)
    os.makedirs(TMP, exist_ok=True)
    for name, (seqs, names, fmt) in make_inputs().items():
        fasta(os.path.join(OUT, name + ".fa"), seqs, names, **fmt)
    meta = {}
    for name, (inp, args) in RUNS.items():
        edx, acx = os.path.join(TMP, name + ".edx"), os.path.join(TMP, name + ".acx")
        cmd = [BURST12, "-r", os.path.join(OUT, inp + ".fa"), "-o", edx, "-a", acx, "-t", "1"] + args
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:])
            raise SystemExit("reference failed: %s" % " ".join(cmd))
        m = {"input": inp + ".fa", "args": args, "acx_sha256": sha(acx)}
        if os.path.getsize(edx) <= 256 << 10:
            shutil.copy(edx, os.path.join(OUT, name + ".edx"))
            m["edx"] = name + ".edx"
        else:
            m["edx_sha256"] = sha(edx)
        for line in r.stdout.splitlines():
            if "Max chain" in line:
                m["reference_tally"] = line.strip()
        meta[name] = m
        print(name, m.get("reference_tally", ""), os.path.getsize(edx))
    with open(os.path.join(HERE, "dna_cases.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
