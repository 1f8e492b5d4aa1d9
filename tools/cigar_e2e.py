#!/usr/bin/env python3
"""What --cigar adds to a study: tools/samples_e2e.py's set-up (bench.py's database, --samples files of --reads synthetic 100-bp reads,
-ad -k 15 -m BEST -i 0.98), one `burst_hip --samples LIST` without the flag and one with it, alternated --reps times.

Recorded: wall seconds of both legs, seconds per further sample (samples 2 .. n, from the phase lines) of both and their difference, and the
device milliseconds, requests and ops of the `Paths:` lines.  With its last two columns removed every output of the --cigar leg must be
the other leg's, byte for byte.  One JSON document on standard output and in --out."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import bench
    import samples_e2e as se
    from burst_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--mode", default="BEST")
    ap.add_argument("--id", type=float, default=0.98)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cigar_e2e.json"))
    a = ap.parse_args()
    b = argparse.Namespace(read_len=100, n_base=1600000, n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile="pairs",
                           reads=a.reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
    refs, edx, acx, done = bench.build_db(a.workdir, b)
    if not os.path.exists(refs):
        host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
    files = []
    for k in range(a.samples):
        fa = os.path.join(a.workdir, "sample_%d_of_%d_r%d.fa" % (k, a.samples, a.reads))
        if not os.path.exists(fa + ".done"):
            host.synth_reads(refs, fa, a.reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * a.reads)
            open(fa + ".done", "w").write("ok")
        files.append(fa)
    flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", a.mode, "-i", str(a.id)]
    outs = {leg: [os.path.join(a.workdir, "cigar_%s_%d.b6" % (leg, k)) for k in range(a.samples)] for leg in ("plain", "cigar")}
    lists = {}
    for leg in outs:
        lists[leg] = os.path.join(a.workdir, "cigar_%s.txt" % leg)
        open(lists[leg], "w").write("".join("%s\t%s\n" % p for p in zip(files, outs[leg])))
    se.run([se.CLI] + flags + ["--samples", lists["plain"]])      # (the files into the page cache)
    wall = {"plain": [], "cigar": []}
    marginal = {"plain": [], "cigar": []}
    paths_ms, requests, ops = [], 0, 0
    for rep in range(a.reps):
        for leg in ("plain", "cigar"):
            t, text = se.run([se.CLI] + flags + ["--samples", lists[leg]] + (["--cigar"] if leg == "cigar" else []))
            wall[leg].append(t)
            blocks = se.phases(text)[1]
            marginal[leg].append(statistics.median(blocks[1:] or blocks))
            if leg == "cigar":
                found = re.findall(r"^Paths: (\d+) requests, (\d+) ops for \d+ lines so far, ([0-9.]+) ms on the device$", text, flags=re.M)
                if len(found) != a.samples:
                    raise SystemExit("%d Paths: lines for %d samples" % (len(found), a.samples))
                paths_ms.append([float(x[2]) for x in found])
                requests, ops = sum(int(x[0]) for x in found), sum(int(x[1]) for x in found)
        for x, y in zip(outs["plain"], outs["cigar"]):
            stripped = b"".join(ln.rsplit(b"\t", 2)[0] + b"\n" for ln in open(y, "rb").read().split(b"\n")[:-1])
            if stripped != open(x, "rb").read():
                raise SystemExit("%s without its last two columns is not %s" % (y, x))
        sys.stderr.write("[cigar_e2e] rep %d: plain %.2f s, --cigar %.2f s\n" % (rep, wall["plain"][-1], wall["cigar"][-1]))
    added = [c - p for p, c in zip(marginal["plain"], marginal["cigar"])]
    res = {"what": "%d samples of %d reads through one burst_hip --samples, without and with --cigar" % (a.samples, a.reads),
           "command": " ".join(["burst_hip"] + flags + ["--samples LIST [--cigar]"]), "commit": a.commit, "edx_bytes": os.path.getsize(edx),
           "samples": a.samples, "reads_per_sample": a.reads, "reps": a.reps,
           "plain_seconds": se.spread(wall["plain"]), "cigar_seconds": se.spread(wall["cigar"]),
           "plain_seconds_per_sample_2_to_n": se.spread(marginal["plain"]), "cigar_seconds_per_sample_2_to_n": se.spread(marginal["cigar"]),
           "added_seconds_per_sample": se.spread(added),
           "paths_device_ms_per_sample": se.spread([statistics.median(x) for x in paths_ms]), "paths_requests_per_run": requests, "paths_ops_per_run": ops,
           "outputs_identical_without_the_two_columns": True}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    for leg in outs:
        for o in outs[leg]:
            os.remove(o)


if __name__ == "__main__":
    main()
