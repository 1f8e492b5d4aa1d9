#!/usr/bin/env python3
"""What --vcf-study adds to a study: wall seconds of `burst_hip --samples LIST -m BEST --vcf` without and with the flag, on the set-up of
tools/vcf_e2e.py (bench.py's database, synthetic reads, ONE DEEP SAMPLE first and once more last, whose haplotype carries a substitution,
an insertion and a deletion per window).  Three alternated repetitions of: flag off, flag on, and -- with --parent-cli, the burst_hip of
the parent commit -- the parent's binary with the flag off: the time with the flag off must be the parent's within the spread of the
repetitions.  Per sample the flag adds the (1, 1) lists coming back in place of the filtered ones (the marginal seconds per sample, and
the `Vcf:` device milliseconds of both legs); at the end of the run it adds one bhip_site_counts call per sample and the file (the
`study VCF` phase line, the `VcfStudy:` line: records, cells, host bytes kept, device milliseconds).  The .b6 and OUT.vcf outputs of all
legs must be byte-identical.  One JSON document on standard output and in --out."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")
STUDY_LINE = re.compile(r"^VcfStudy: (\d+) samples done, (\d+) failed, records (\d+) SNV / (\d+) Del / (\d+) Ins, (\d+) cells, (\d+) host bytes kept, device ([0-9.]+) ms$", re.M)
STUDY_PHASE = re.compile(r"^ \[study VCF\s+([0-9.]+) s\]$", re.M)


def main():
    import bench
    import samples_e2e as se
    import vcf_e2e as ve
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcfstudy_e2e.json"))
    a = ap.parse_args()
    res = {"what": "wall seconds of burst_hip --samples --vcf (a deep sample of %d windows x %d reads, %d samples of %d reads, the deep sample again under another name; "
                   "-ad -k %d -m BEST -i %s) without and with --vcf-study%s; marginal = median seconds of the samples between the two deep ones, from the run's own "
                   "phase lines" % (a.windows, a.depth, a.samples - 2, a.reads, a.K, a.id, ", and the parent commit's binary without it" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "profiles": {}}
    for profile in a.profiles.split(","):
        wd = os.path.join(a.workdir, profile)
        b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile=profile,
                               reads=a.reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
        refs, edx, acx, done = bench.build_db(wd, b)
        if not os.path.exists(refs):
            host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
        deep = os.path.join(wd, "deep_w%d_d%d.fa" % (a.windows, a.depth))
        n_deep = ve.deep_sample(refs, deep, a.windows, a.depth)
        files = [deep]
        for k in range(1, a.samples - 1):
            fa = os.path.join(wd, "sample_%d_of_%d_r%d.fa" % (k, a.samples, a.reads))
            if not os.path.exists(fa + ".done"):
                host.synth_reads(refs, fa, a.reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * a.reads)
                open(fa + ".done", "w").write("ok")
            files.append(fa)
        files.append(deep)
        flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", "BEST", "-i", str(a.id), "--vcf"]
        legs = {"off": (CLI, []), "on": (CLI, ["--vcf-study", os.path.join(wd, "vs_on_")])}
        if a.parent_cli:
            legs["parent_off"] = (a.parent_cli, [])
        outs = {leg: [os.path.join(wd, "vs_%s" % leg, "s%d.b6" % k) for k in range(a.samples)] for leg in legs}      # (the same sample names in every leg)
        lists = {}
        for leg in legs:
            os.makedirs(os.path.join(wd, "vs_%s" % leg), exist_ok=True)
            lists[leg] = os.path.join(wd, "vslist_%s.txt" % leg)
            open(lists[leg], "w").write("".join("%s\t%s\n" % p for p in zip(files, outs[leg])))
        se.run([CLI] + flags + ["--samples", lists["off"]])      # (the files into the page cache)
        wall = {leg: [] for leg in legs}
        marginal = {leg: [] for leg in legs}
        vcf_ms = {leg: [] for leg in legs}
        study, study_phase = [], []
        for rep in range(a.reps):
            for leg, (cli, extra) in legs.items():
                t, text = se.run([cli] + flags + ["--samples", lists[leg]] + extra)
                wall[leg].append(t)
                blocks = se.phases(text)[1]
                marginal[leg].append(statistics.median(blocks[1:-1]) if len(blocks) > 2 else blocks[0])
                vcf_ms[leg] += [float(x[9]) for x in ve.VCF_LINE.findall(text)]
                if leg == "on":
                    found, phase = STUDY_LINE.findall(text), STUDY_PHASE.findall(text)
                    if len(found) != 1 or len(phase) != 1:
                        raise SystemExit("%d VcfStudy: lines and %d phase lines in one run" % (len(found), len(phase)))
                    study.append(found[0])
                    study_phase.append(float(phase[0]))
            same = all(len({open(outs[leg][k] + ext, "rb").read() for leg in legs}) == 1 for k in range(a.samples) for ext in ("", ".vcf"))
            sys.stderr.write("[vcfstudy_e2e] %s rep %d: %s, outputs identical: %s\n" % (profile, rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
            if not same:
                raise SystemExit("the outputs of the legs differ")
        names = ("samples_done", "samples_failed", "snv_records", "del_records", "ins_records", "cells", "host_bytes_kept", "device_ms")
        res["profiles"][profile] = {
            "edx_bytes": os.path.getsize(edx), "reads_of_the_deep_sample": n_deep, "reads_per_further_sample": a.reads,
            "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs}, "marginal_seconds_per_sample": {leg: se.spread(marginal[leg]) for leg in legs},
            "vcf_line_device_ms": {leg: se.spread(vcf_ms[leg]) for leg in legs if vcf_ms[leg]},
            "study_phase_seconds": se.spread(study_phase),
            "study_line": {name: se.spread([(float if name == "device_ms" else int)(x[k]) for x in study]) for k, name in enumerate(names)},
            "study_vcf_bytes": os.path.getsize(os.path.join(wd, "vs_on_study.vcf")),
            "outputs_identical": True}
        os.remove(os.path.join(wd, "vs_on_study.vcf"))
        for leg in legs:
            for o in outs[leg]:
                os.remove(o)
                os.remove(o + ".vcf")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
