#!/usr/bin/env python3
"""What --vcf adds to a study: wall seconds per further sample of `burst_hip --samples LIST -m BEST` without and with the flag, on the
set-up of tools/variants_e2e.py (bench.py's database, synthetic reads) with ONE DEEP SAMPLE, first and once more last: reads drawn from a few hundred
windows of the first references, most of them from a haplotype that carries one substitution, one insertion and one deletion per window,
so that records of all three kinds are written.  Alternated repetitions; --parent-cli names the burst_hip of the parent commit: the same
run without the flag, in the same alternation -- the time with the flag off must not move.  The `Vcf:` lines give the lines, allele
events, distinct alleles, records and the device milliseconds: the deep sample as the first call of a process, which pays for the scratch
buffers, and the same sample again as the last, warm call.  The .b6 outputs of all legs must be byte-identical.  One JSON document on standard output and in --out."""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")
VCF_LINE = re.compile(r"^Vcf: (\d+) lines, (\d+) allele events, (\d+) distinct alleles, records written (\d+) SNV / (\d+) Del / (\d+) Ins, "
                      r"skipped runs (\d+) end / (\d+) adjacent / (\d+) long, device ([0-9.]+) ms$", re.M)


def first_records(path, n):
    """the first n (header, sequence) records of a FASTA file, read no further"""
    recs, name, seq = [], None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(seq)))
                    if len(recs) == n:
                        return recs
                name, seq = line[1:], []
            else:
                seq.append(line)
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs


def deep_sample(refs, path, windows, depth, seed=5):
    """`depth` reads of 100 symbols over one window of each of the first `windows` references; four in five come from a haplotype with a
    substitution at 250, one inserted base behind 300 and two deleted ones behind 350 (a read of 100 symbols holds at most two of the three)"""
    rng = np.random.default_rng(seed)
    n = 0
    with open(path, "w") as f:
        for w, (_, seq) in enumerate(first_records(refs, windows)):
            if len(seq) < 600:
                continue
            hap = seq[:250] + "CGTA"["ACGT".find(seq[250].upper())] + seq[251:300] + "G" + seq[300:350] + seq[352:]
            for k in range(depth):
                src = hap if k % 5 else seq
                s = int(rng.integers(160, 340))
                f.write(">deep_w%d_r%d\n%s\n" % (w, k, src[s:s + 100]))
                n += 1
    return n


def main():
    import bench
    import samples_e2e as se
    from burst_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--windows", type=int, default=300)
    ap.add_argument("--depth", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--db-scale", type=float, default=1.0)
    ap.add_argument("--profiles", default="pairs")
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--id", type=float, default=0.98)
    ap.add_argument("--parent-cli", default="", help="burst_hip of the parent commit (optional)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_e2e.json"))
    a = ap.parse_args()
    res = {"what": "wall seconds of burst_hip --samples (a deep sample of %d windows x %d reads, %d samples of %d reads, the deep sample again; -ad -k %d -m BEST -i %s) without and "
                   "with --vcf%s; marginal = median seconds of the samples between the two deep ones, from the run's own phase lines" % (
                       a.windows, a.depth, a.samples - 2, a.reads, a.K, a.id, ", and the parent commit's binary without it" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "profiles": {}}
    for profile in a.profiles.split(","):
        wd = os.path.join(a.workdir, profile)
        b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile=profile,
                               reads=a.reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
        refs, edx, acx, done = bench.build_db(wd, b)
        if not os.path.exists(refs):
            host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
        deep = os.path.join(wd, "deep_w%d_d%d.fa" % (a.windows, a.depth))
        n_deep = deep_sample(refs, deep, a.windows, a.depth)
        files = [deep]
        for k in range(1, a.samples - 1):
            fa = os.path.join(wd, "sample_%d_of_%d_r%d.fa" % (k, a.samples, a.reads))
            if not os.path.exists(fa + ".done"):
                host.synth_reads(refs, fa, a.reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * a.reads)
                open(fa + ".done", "w").write("ok")
            files.append(fa)
        files.append(deep)
        flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", "BEST", "-i", str(a.id)]
        legs = {"off": (CLI, []), "on": (CLI, ["--vcf"])}
        if a.parent_cli:
            legs["parent_off"] = (a.parent_cli, [])
        outs = {leg: [os.path.join(wd, "v_%s_%d.b6" % (leg, k)) for k in range(a.samples)] for leg in legs}
        lists = {}
        for leg in legs:
            lists[leg] = os.path.join(wd, "vlist_%s.txt" % leg)
            open(lists[leg], "w").write("".join("%s\t%s\n" % p for p in zip(files, outs[leg])))
        se.run([CLI] + flags + ["--samples", lists["off"]])      # (the files into the page cache)
        wall = {leg: [] for leg in legs}
        marginal = {leg: [] for leg in legs}
        first, warm, further = [], [], []      # the Vcf: lines of the deep sample as the first call of a process and as the last, and of the samples between
        for rep in range(a.reps):
            for leg, (cli, extra) in legs.items():
                t, text = se.run([cli] + flags + ["--samples", lists[leg]] + extra)
                wall[leg].append(t)
                blocks = se.phases(text)[1]
                marginal[leg].append(statistics.median(blocks[1:-1]) if len(blocks) > 2 else blocks[0])
                if leg == "on":
                    found = VCF_LINE.findall(text)
                    if len(found) != a.samples:
                        raise SystemExit("%d Vcf: lines for %d samples" % (len(found), a.samples))
                    first.append(found[0])
                    warm.append(found[-1])
                    further += found[1:-1]
            same = all(len({open(outs[leg][k], "rb").read() for leg in legs}) == 1 for k in range(a.samples))
            sys.stderr.write("[vcf_e2e] %s rep %d: %s, outputs identical: %s\n" % (profile, rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
            if not same:
                raise SystemExit("the outputs of the legs differ")
        figures = lambda rows: {name: se.spread([(float if name == "device_ms" else int)(x[k]) for x in rows]) for k, name in enumerate(
            ("lines", "allele_events", "distinct_alleles", "snv_records", "del_records", "ins_records", "skipped_end", "skipped_adjacent", "skipped_long", "device_ms"))}
        res["profiles"][profile] = {
            "edx_bytes": os.path.getsize(edx), "reads_of_the_deep_sample": n_deep, "reads_per_further_sample": a.reads,
            "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs}, "marginal_seconds_per_sample": {leg: se.spread(marginal[leg]) for leg in legs},
            "vcf_line_deep_sample_first_call": figures(first), "vcf_line_deep_sample_warm_call": figures(warm), "vcf_lines_samples_between": figures(further) if further else {},
            "vcf_bytes": [os.path.getsize(o + ".vcf") for o in outs["on"]],
            "outputs_identical": True}
        for leg in legs:
            for o in outs[leg]:
                os.remove(o)
                if os.path.exists(o + ".vcf"):
                    os.remove(o + ".vcf")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
