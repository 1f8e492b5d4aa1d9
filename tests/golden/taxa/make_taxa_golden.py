#!/usr/bin/env python3
"""The fixture of the taxon-table tests (tests/test_taxa_cpu.py, tests/test_gpu_taxa_cli.py), produced once in the build container:
    REF=<the reference's source tree> python tests/golden/taxa/make_taxa_golden.py
  dna_q100_best_tax_fr_taxa.txt   the taxa table the reference's embalmlets/embalmulate.c writes for tests/golden/dna_q100_best_tax_fr.b6
embalmulate is compiled from the reference (the directory REF names) into a scratch directory; only its output table is committed.
As written the tool names an undeclared variable (`GGtrim` for its `ggtrim`), hence -DGGtrim=ggtrim.  It takes a line's sample from the text
of the read name before '_' and writes no count column for a name without one, so every read name is given the prefix `s1_`.  The table then
has one row per distinct string of column 13 (the empty string included: the reads of a reference the map does not know) with the number of
reads that carry it."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.dirname(HERE)
REF = os.environ["REF"]


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "embalmulate")
        subprocess.check_call(["gcc", "-O2", "-w", "-DGGtrim=ggtrim", os.path.join(REF, "embalmlets", "embalmulate.c"), "-o", exe, "-lm"])
        b6 = os.path.join(tmp, "in.b6")
        with open(b6, "wb") as f:
            for ln in open(os.path.join(G, "dna_q100_best_tax_fr.b6"), "rb").read().splitlines():
                f.write(b"s1_" + ln + b"\n")
        subprocess.check_call([exe, b6, os.path.join(tmp, "otu.tsv"), os.path.join(tmp, "taxa.tsv")], stdout=subprocess.DEVNULL)
        open(os.path.join(HERE, "dna_q100_best_tax_fr_taxa.txt"), "wb").write(open(os.path.join(tmp, "taxa.tsv"), "rb").read())


if __name__ == "__main__":
    main()
