#!/usr/bin/env python3
"""What --sam adds to a study: wall seconds per further sample of `burst_hip --samples LIST -m BEST` without and with the flag, on
the set-up of tools/samples_e2e.py (bench.py's database, synthetic reads), in alternated repetitions.  --parent-cli names the burst_hip
of the parent commit: the same run without the flag, in the same alternation -- the time with the flag off must not move.  The
`Sam:` lines give the records, the MD bytes and the device milliseconds of the MD calls (the re-upload of the ops is inside the wall
time, not inside the device time).  The .b6 outputs of all legs must be byte-identical.  One JSON document on standard output and in --out."""
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


def main():
    import bench
    import samples_e2e as se
    from burst_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--db-scale", type=float, default=1.0)
    ap.add_argument("--profiles", default="pairs")
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--id", type=float, default=0.98)
    ap.add_argument("--parent-cli", default="", help="burst_hip of the parent commit (optional)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_e2e.json"))
    a = ap.parse_args()
    res = {"what": "wall seconds of burst_hip --samples (%d samples of %d reads, -ad -k %d -m BEST -i %s) without and with --sam%s; marginal = median "
                   "seconds of samples 2 .. n from the run's own phase lines" % (a.samples, a.reads, a.K, a.id, ", and the parent commit's binary without it" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "profiles": {}}
    for profile in a.profiles.split(","):
        wd = os.path.join(a.workdir, profile)
        n_reads = a.reads
        b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile=profile,
                               reads=n_reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
        refs, edx, acx, done = bench.build_db(wd, b)
        if not os.path.exists(refs):
            host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
        files = []
        for k in range(a.samples):
            fa = os.path.join(wd, "sample_%d_of_%d_r%d.fa" % (k, a.samples, n_reads))
            if not os.path.exists(fa + ".done"):
                host.synth_reads(refs, fa, n_reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * n_reads)
                open(fa + ".done", "w").write("ok")
            files.append(fa)
        flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", "BEST", "-i", str(a.id)]
        legs = {"off": (CLI, []), "on": (CLI, ["--sam"])}
        if a.parent_cli:
            legs["parent_off"] = (a.parent_cli, [])
        outs = {leg: [os.path.join(wd, "s_%s_%d.b6" % (leg, k)) for k in range(a.samples)] for leg in legs}
        lists = {}
        for leg in legs:
            lists[leg] = os.path.join(wd, "list_%s.txt" % leg)
            open(lists[leg], "w").write("".join("%s\t%s\n" % p for p in zip(files, outs[leg])))
        se.run([CLI] + flags + ["--samples", lists["off"]])      # (the files into the page cache)
        wall = {leg: [] for leg in legs}
        marginal = {leg: [] for leg in legs}
        sam_lines = []
        for rep in range(a.reps):
            for leg, (cli, extra) in legs.items():
                t, text = se.run([cli] + flags + ["--samples", lists[leg]] + extra)
                wall[leg].append(t)
                blocks = se.phases(text)[1]
                marginal[leg].append(statistics.median(blocks[1:]) if len(blocks) > 1 else blocks[0])
                if leg == "on":
                    sam_lines += re.findall(r"^Sam: (\d+) records, (\d+) unmapped records, (\d+) MD bytes, device ([0-9.]+) ms$", text, re.M)
            same = all(len({open(outs[leg][k], "rb").read() for leg in legs}) == 1 for k in range(a.samples))
            sys.stderr.write("[sam_e2e] %s rep %d: %s, outputs identical: %s\n" % (profile, rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
            if not same:
                raise SystemExit("the outputs of the legs differ")
        lines_per_sample = sum(1 for _ in open(outs["off"][0], "rb"))
        res["profiles"][profile] = {
            "edx_bytes": os.path.getsize(edx), "reads_per_sample": n_reads, "lines_of_sample_1": lines_per_sample,
            "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs}, "marginal_seconds_per_sample": {leg: se.spread(marginal[leg]) for leg in legs},
            "sam_lines": {"device_ms": se.spread([float(x[3]) for x in sam_lines]), "records": se.spread([int(x[0]) for x in sam_lines]),
                          "md_bytes": se.spread([int(x[2]) for x in sam_lines])},
            "sam_bytes_of_sample_1": os.path.getsize(outs["on"][0] + ".sam"),
            "outputs_identical": True}
        for leg in legs:
            for o in outs[leg]:
                os.remove(o)
                if os.path.exists(o + ".sam"):
                    os.remove(o + ".sam")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
