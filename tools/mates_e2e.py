#!/usr/bin/env python3
"""Wall time of burst_hip --mates against the way without it (two single-end invocations), on the bench database.

  A   `burst_hip -q R1 -o o1.b6 -fr` and `burst_hip -q R2 -o o2.b6 -fr`, one after the other (sum of the wall times; the user's own
      join script is not counted)
  B   one `burst_hip -q R1 --mates R2 -o paired.b6`

The legs alternate, each --reps times.  The database is bench.py's (generated from its seed, --db-scale as there).  The pairs are --pairs
synthetic fragments of --fragment bases drawn from its references with 0-2 edits (bh_synth_reads_ex), mate 1 = the first 100 bases, mate 2
= the reverse complement of the last 100.  B's output must be tests/mateslib.py applied to A's two outputs (checked once, on the first
repetition, when --check is given: the brute force in Python takes minutes at a million pairs).  One JSON document on standard output and in
--out, with the figures of B's `Mates:` line."""
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
COMP = bytes.maketrans(b"ACGTRYKMBVDHacgtrykmbvdh", b"TGCAYRMKVBHDtgcayrmkvbhd")      # (S, W and N are their own complements)


def run(cmd):
    t = time.time()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout[-4000:])
        raise SystemExit("failed (%d): %s" % (r.returncode, " ".join(cmd)))
    return time.time() - t, r.stdout


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def split_fragments(frag_fa, m1, m2, n=100):
    with open(frag_fa, "rb") as f, open(m1, "wb") as o1, open(m2, "wb") as o2:
        name = None
        for ln in f:
            if ln.startswith(b">"):
                name = ln[1:].split()[0]
                continue
            s = ln.strip()
            if name is None or len(s) < n:
                continue
            o1.write(b">" + name + b"/1\n" + s[:n] + b"\n")
            o2.write(b">" + name + b"/2\n" + s[-n:].translate(COMP)[::-1] + b"\n")
            name = None


def main():
    import bench
    from burst_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--fragment", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--db-scale", type=float, default=1.0, help="as bench.py: 1 = the 2.77 GB .edx")
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--mode", default="ALLPATHS")
    ap.add_argument("--id", type=float, default=0.98)
    ap.add_argument("--check", action="store_true", help="compare B's output with tests/mateslib.py over A's outputs (slow in Python)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mates_e2e.json"))
    a = ap.parse_args()
    b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile="pairs",
                           reads=a.pairs, pool=1, edits="0,1,2", fr=True, iupac=0.0, drop_refs=False)
    if len(bench.db_parts(b)) > 1:
        raise SystemExit("a database built in parts keeps no reference FASTA to draw the fragments from: --db-scale <= 2.5")
    t = time.time()
    refs, edx, acx, done = bench.build_db(a.workdir, b)
    if not os.path.exists(refs):
        host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
    tag = "p%d_f%d" % (a.pairs, a.fragment)
    frag, m1, m2 = (os.path.join(a.workdir, "mates_%s_%s.fa" % (tag, x)) for x in ("frag", "1", "2"))
    if not os.path.exists(m2 + ".done"):
        host.synth_reads(refs, frag, a.pairs, a.fragment, [0, 1, 2], rc=True, seed=43)
        split_fragments(frag, m1, m2)
        os.remove(frag)
        open(m2 + ".done", "w").write("ok")
    sys.stderr.write("[mates_e2e] inputs ready in %.1f s (%s, %.2f GB)\n" % (time.time() - t, edx, os.path.getsize(edx) / 1e9))
    flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", a.mode, "-i", str(a.id)]
    o1, o2, op = (os.path.join(a.workdir, "mates_%s.b6" % x) for x in ("A1", "A2", "B"))
    run([CLI] + flags + ["-q", m1, "-o", o1, "-fr"])      # (the files into the page cache, the binary's first start)
    A, B, mates, checked = [], [], None, None
    for rep in range(a.reps):
        ta = run([CLI] + flags + ["-q", m1, "-o", o1, "-fr"])[0] + run([CLI] + flags + ["-q", m2, "-o", o2, "-fr"])[0]
        tb, text = run([CLI] + flags + ["-q", m1, "--mates", m2, "-o", op])
        A.append(ta); B.append(tb)
        m = re.search(r"^Mates: (\d+) \+ (\d+) reads, (\d+) pairs named in both files, (\d+) placed on both sides; (\d+) \+ (\d+) lines, (\d+) combinations examined, (\d+) written; ([0-9.]+) ms on the device$", text, re.M)
        if not m:
            raise SystemExit("no Mates: line in the output of --mates")
        mates = dict(zip(("reads1", "reads2", "pairs_named", "pairs_placed", "lines1", "lines2", "examined", "written"), (int(x) for x in m.groups()[:8])), device_ms=float(m.group(9)))
        if a.check and rep == 0:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import mateslib
            checked = open(op, "rb").read() == mateslib.paired_text(open(o1, "rb").read(), open(o2, "rb").read())
            if not checked:
                raise SystemExit("the output of --mates differs from the definition over the two single-end outputs")
        sys.stderr.write("[mates_e2e] rep %d: A %.2f s, B %.2f s, %s\n" % (rep, ta, tb, mates))
    res = {"what": "wall time of %d pairs of 100-base mates: A = two single-end burst_hip invocations (join not counted), B = one burst_hip --mates" % a.pairs,
           "command": " ".join(["burst_hip"] + flags + ["-q R1 --mates R2 -o paired.b6 | -q Rk -o ok.b6 -fr"]), "commit": a.commit, "edx_bytes": os.path.getsize(edx),
           "pairs": a.pairs, "fragment": a.fragment, "reps": a.reps, "A_seconds": spread(A), "B_seconds": spread(B), "A_over_B": statistics.median(A) / statistics.median(B),
           "B_below_A_in_every_rep": all(y < x for x, y in zip(A, B)), "mates_line": mates, "lines_joined": mates["lines1"] + mates["lines2"], "output_is_the_definition": checked}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    for o in (o1, o2, op):
        os.remove(o)


if __name__ == "__main__":
    main()
