#!/usr/bin/env python3
"""Wall time per sample of burst_hip --samples against the way without it (one process per query file), on the bench database.

  A   one `burst_hip -q ... -o ...` per sample, one after the other (sum of the wall times)
  B   one `burst_hip --samples LIST`
  C   B with BURST_HOST_SERIAL_INGEST=1 (no ingest thread: what parsing sample i+1 beside sample i is worth)

The legs alternate, each --reps times.  The database is bench.py's (generated from its seed, --db-scale as there), the samples are
--samples files of --reads synthetic reads each (bh_synth_reads_ex, distinct first_read), as FASTA.  All outputs of B (and C) must be
byte-identical to A's.  One JSON document on standard output and in --out."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")


def run(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if r.returncode:
        sys.stderr.write(r.stdout[-4000:])
        raise SystemExit("failed (%d): %s" % (r.returncode, " ".join(cmd)))
    return time.time() - t, r.stdout


def phases(text):
    """(database seconds, [seconds of each sample block]) from the phase lines of a --samples run"""
    t_db, blocks, cur = 0.0, [], None
    for ln in text.splitlines():
        if ln.startswith("Sample ") and ": " in ln and " -> " in ln:
            cur = len(blocks)
            blocks.append(0.0)
            continue
        m = re.match(r"^ \[(.{28}) +([0-9.]+) s(.*)\]$", ln)
        if not m:
            continue
        if cur is None:
            t_db += float(m.group(2))
        else:
            w = re.search(r"waited for ([0-9.]+) s", m.group(3))      # (an ingest that ran ahead costs the sample what it waited for)
            blocks[cur] += float(w.group(1)) if w else float(m.group(2))
    return t_db, blocks


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def main():
    import bench
    from burst_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--db-scale", type=float, default=1.0, help="as bench.py: 1 = the 2.77 GB .edx, 11.37 = the 31.5 GB one")
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--mode", default="BEST")
    ap.add_argument("--id", type=float, default=0.98)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samples_e2e.json"))
    a = ap.parse_args()
    b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile="pairs",
                           reads=a.reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
    if len(bench.db_parts(b)) > 1:
        raise SystemExit("a database built in parts keeps no reference FASTA to draw the samples from: --db-scale <= 2.5")
    t = time.time()
    refs, edx, acx, done = bench.build_db(a.workdir, b)
    if not os.path.exists(refs):                       # (a database another run left without its FASTA)
        host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
    files = []
    for k in range(a.samples):
        fa = os.path.join(a.workdir, "sample_%d_of_%d_r%d.fa" % (k, a.samples, a.reads))
        if not os.path.exists(fa + ".done"):
            host.synth_reads(refs, fa, a.reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * a.reads)
            open(fa + ".done", "w").write("ok")
        files.append(fa)
    sys.stderr.write("[samples_e2e] inputs ready in %.1f s (%s, %.2f GB)\n" % (time.time() - t, edx, os.path.getsize(edx) / 1e9))
    flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", a.mode, "-i", str(a.id)]
    outs = {leg: [os.path.join(a.workdir, "sample_%s_%d.b6" % (leg, k)) for k in range(a.samples)] for leg in "ABC"}
    lists = {}
    for leg in "BC":
        lists[leg] = os.path.join(a.workdir, "samples_%s.txt" % leg)
        open(lists[leg], "w").write("".join("%s\t%s\n" % p for p in zip(files, outs[leg])))
    serial = dict(os.environ, BURST_HOST_SERIAL_INGEST="1")
    A, B, C, A_each, B_db, B_marginal, C_marginal = [], [], [], [], [], [], []
    run([CLI] + flags + ["-q", files[0], "-o", outs["A"][0]])      # (the files into the page cache, the binary's first start)
    for rep in range(a.reps):
        each = [run([CLI] + flags + ["-q", q, "-o", o])[0] for q, o in zip(files, outs["A"])]
        A.append(sum(each)); A_each.append(each)
        tb, text = run([CLI] + flags + ["--samples", lists["B"]])
        B.append(tb)
        t_db, blocks = phases(text)
        B_db.append(t_db); B_marginal.append(statistics.median(blocks[1:]) if len(blocks) > 1 else blocks[0])
        tc, text = run([CLI] + flags + ["--samples", lists["C"]], env=serial)
        C.append(tc)
        C_marginal.append(statistics.median(phases(text)[1][1:] or phases(text)[1]))
        same = all(open(x, "rb").read() == open(y, "rb").read() == open(z, "rb").read() for x, y, z in zip(outs["A"], outs["B"], outs["C"]))
        sys.stderr.write("[samples_e2e] rep %d: A %.2f s, B %.2f s, C %.2f s, outputs identical: %s\n" % (rep, A[-1], B[-1], C[-1], same))
        if not same:
            raise SystemExit("the outputs of --samples differ from the separate invocations'")
    res = {"what": "wall time of %d samples of %d reads: A = one burst_hip process per sample, B = one burst_hip --samples, C = B without the ingest thread" % (a.samples, a.reads),
           "command": " ".join(["burst_hip"] + flags + ["--samples LIST | -q sample_k.fa -o sample_k.b6"]), "commit": a.commit, "edx_bytes": os.path.getsize(edx),
           "samples": a.samples, "reads_per_sample": a.reads, "reps": a.reps,
           "A_seconds": spread(A), "B_seconds": spread(B), "C_seconds": spread(C), "A_per_invocation_seconds": spread([x for e in A_each for x in e]),
           "B_database_phases_seconds": spread(B_db), "B_marginal_seconds_per_sample_2_to_n": spread(B_marginal), "C_marginal_seconds_per_sample_2_to_n": spread(C_marginal),
           "A_over_B": statistics.median(A) / statistics.median(B), "B_below_A_in_every_rep": all(y < x for x, y in zip(A, B)), "outputs_identical": True}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    for leg in "ABC":
        for o in outs[leg]:
            os.remove(o)


if __name__ == "__main__":
    main()
