#!/usr/bin/env python3
"""The fixtures of the coverage tests (tests/test_coverage_cpu.py, tests/test_gpu_coverage.py), produced once in the build container:
    python tests/golden/cov/make_cov_golden.py
  len.txt                                 `name<TAB>length` of every sequence of tests/golden/refs.fa (bcov's length table)
  dna_q100_best_shared.txt, _shared_binary.txt   what the reference's embalmlets/bcov.c writes for tests/golden/dna_q100_best.b6
bcov is compiled from the reference (REF, default /root/reference) into a scratch directory; only its output files are committed.
That .b6 holds forward lines only, so bcov's tables are the tables of this project's definition there (README, --coverage); bcov's
unique tables depend on its neighbour comparison of query names, which is not reproduced, and are not kept."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.dirname(HERE)
REF = os.environ.get("REF", "/root/reference")


def main():
    names, lens = [], []
    for ln in open(os.path.join(G, "refs.fa")):
        ln = ln.rstrip("\r\n")
        if ln.startswith(">"):
            names.append(ln[1:])
            lens.append(0)
        else:
            lens[-1] += len(ln)
    with open(os.path.join(HERE, "len.txt"), "w") as f:
        for n, l in zip(names, lens):
            f.write("%s\t%d\n" % (n, l))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bcov")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-w", os.path.join(REF, "embalmlets", "bcov.c"), "-o", exe, "-lm"])
        b6 = os.path.join(G, "dna_q100_best.b6")
        assert all(int(ln.split(b"\t")[8]) <= int(ln.split(b"\t")[9]) for ln in open(b6, "rb").read().splitlines()), "forward lines only"
        subprocess.check_call([exe, b6, os.path.join(HERE, "len.txt"), os.path.join(tmp, "o_")], stdout=subprocess.DEVNULL)
        for kind in ("shared", "shared_binary"):
            open(os.path.join(HERE, "dna_q100_best_%s.txt" % kind), "wb").write(open(os.path.join(tmp, "o_%s.txt" % kind), "rb").read())


if __name__ == "__main__":
    main()
