#!/usr/bin/env python3
"""What --taxa adds to a study: wall seconds per further sample of `burst_hip --samples LIST -m ALLPATHS -b MAP` without and with the flag,
on the set-up of tools/abundance_e2e.py (bench.py's database, synthetic reads), for the low-redundancy database (`pairs`) and for the
`strains` profile, in alternated repetitions.  The taxonomy map is synthetic and follows the generator's families: base sequence b is a
genus, its variants are its species, and b // 100, // 1000, // 10000, // 100000 are family, order, class and phylum.  --parent-cli names the
burst_hip of the parent commit: the same run without the flag, in the same alternation -- the time with the flag off must not move.  The
`Taxa:` lines give the device milliseconds of a sample's call, the first of a run (buffers allocated) apart from the later ones.  The
outputs of all legs must be byte-identical.  One JSON document on standard output and in --out."""
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


def write_map(path, parts):
    """`ref_b<b>_v<v><TAB>taxonomy` for every sequence the generator names (bench.db_parts: first base, bases, variants per base, ...)"""
    with open(path + ".tmp", "w") as f:
        for first, n, nv, _, _ in parts:
            for b in range(first, first + n):
                up = "k__Synth;p__P%d;c__C%d;o__O%d;f__F%d;g__G%d;s__S%d_" % (b // 100000, b // 10000, b // 1000, b // 100, b, b)
                f.write("".join("ref_b%d_v%d\t%s%d\n" % (b, v, up, v) for v in range(nv)))
    os.rename(path + ".tmp", path)


def main():
    import bench
    import samples_e2e as se
    from burst_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reads-strains", type=int, default=250000, help="reads per sample on the strains profile (a read ties on about 28 lanes there: 28 lines per read)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--db-scale", type=float, default=1.0)
    ap.add_argument("--profiles", default="pairs,strains")
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--id", type=float, default=0.98)
    ap.add_argument("--agree", type=int, default=1000)
    ap.add_argument("--parent-cli", default="", help="burst_hip of the parent commit (optional)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taxa_e2e.json"))
    a = ap.parse_args()
    res = {"what": "wall seconds of burst_hip --samples (%d samples of %d reads -- %d on the strains profile --, -ad -k %d -m ALLPATHS -i %s -b MAP) without and with --taxa%s; marginal = "
                   "median seconds of samples 2 .. n from the run's own phase lines; the map is synthetic (7 levels, a genus per base sequence)"
                   % (a.samples, a.reads, a.reads_strains, a.K, a.id, ", and the parent commit's binary without it" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "db_scale": a.db_scale, "profiles": {}}
    for profile in a.profiles.split(","):
        wd = os.path.join(a.workdir, profile)
        n_reads = a.reads_strains if profile == "strains" else a.reads
        b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile=profile,
                               reads=n_reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
        refs, edx, acx, done = bench.build_db(wd, b)
        if not os.path.exists(refs):
            host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
        tax = os.path.join(wd, "taxa_map_%s_b%d.txt" % (profile, b.n_base))
        if not os.path.exists(tax):
            write_map(tax, bench.db_parts(b))
        files = []
        for k in range(a.samples):
            fa = os.path.join(wd, "sample_%d_of_%d_r%d.fa" % (k, a.samples, n_reads))
            if not os.path.exists(fa + ".done"):
                host.synth_reads(refs, fa, n_reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * n_reads)
                open(fa + ".done", "w").write("ok")
            files.append(fa)
        flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", "ALLPATHS", "-i", str(a.id), "-b", tax]
        prefix = os.path.join(wd, "tx_")
        legs = {"off": (CLI, []), "on": (CLI, ["--taxa", prefix, "--taxa-agree", str(a.agree)])}
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
        first_ms, warm_ms, tx_lines, table_s = [], [], [], []
        for rep in range(a.reps):
            for leg, (cli, extra) in legs.items():
                t, text = se.run([cli] + flags + ["--samples", lists[leg]] + extra)
                wall[leg].append(t)
                blocks = se.phases(text)[1]
                marginal[leg].append(statistics.median(blocks[1:]) if len(blocks) > 1 else blocks[0])
                if leg == "on":
                    m = re.findall(r"^Taxa: (\d+) reads, (\d+) groups, (\d+) pairs, (\d+) reads at the root, deepest level (\d+), device ([0-9.]+) ms$", text, re.M)
                    if len(m) != a.samples:
                        raise SystemExit("%d `Taxa:` lines for %d samples" % (len(m), a.samples))
                    first_ms.append(float(m[0][5]))
                    warm_ms += [float(x[5]) for x in m[1:]]
                    tx_lines += m
                    table_s += [float(x) for x in re.findall(r"^ \[taxon tables +([0-9.]+) s", text, re.M)]
            same = all(len({open(outs[leg][k], "rb").read() for leg in legs}) == 1 for k in range(a.samples))
            sys.stderr.write("[taxa_e2e] %s rep %d: %s, outputs identical: %s\n" % (profile, rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
            if not same:
                raise SystemExit("the outputs of the legs differ")
        lines_per_sample = sum(1 for _ in open(outs["off"][0], "rb"))
        levels = sorted(f for f in os.listdir(wd) if f.startswith("tx_taxa"))
        res["profiles"][profile] = {
            "edx_bytes": os.path.getsize(edx), "map_bytes": os.path.getsize(tax), "reads_per_sample": n_reads, "lines_of_sample_1": lines_per_sample,
            "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs}, "marginal_seconds_per_sample": {leg: se.spread(marginal[leg]) for leg in legs},
            "taxa_lines": {"device_ms_first_call": se.spread(first_ms), "device_ms_warm_call": se.spread(warm_ms) if warm_ms else None,
                           "groups": se.spread([int(x[1]) for x in tx_lines]), "pairs": se.spread([int(x[2]) for x in tx_lines]),
                           "reads_at_the_root": se.spread([int(x[3]) for x in tx_lines]), "deepest_level": max(int(x[4]) for x in tx_lines)},
            "taxon_tables_seconds": se.spread(table_s) if table_s else None, "files": levels, "outputs_identical": True}
        for leg in legs:
            for o in outs[leg]:
                os.remove(o)
        for f in levels:
            os.remove(os.path.join(wd, f))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")      # (after every profile: a run that is cut short keeps what it has)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
