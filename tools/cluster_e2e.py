#!/usr/bin/env python3
"""What --cluster adds to a self-alignment: wall seconds of `burst_hip -r reads.fa -q reads.fa -m FORAGE -fr` without and with the flag on
synthetic amplicon families (a base sequence per family, every read a few substitutions away from it, a share of exact copies), in
alternated repetitions.  --parent-cli names the burst_hip of the parent commit: the same run without the flag, in the same alternation --
the time with the flag off must not move.  The `Clusters:` line gives the device milliseconds and the rounds.  The .b6 of all legs must be
byte-identical.  One JSON document on standard output and in --out."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")


def write_families(path, families, per_family, length, max_subs, copies, seed):
    """families x per_family reads of `length` bases, 0 .. max_subs substitutions from the family's base; `copies` of them exact copies of
    the read before; names carry `;size=N`"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        n = 0
        for _ in range(families):
            base = rng.integers(0, 4, size=length)
            prev = base
            for _ in range(per_family):
                if rng.random() < copies:
                    s = prev
                else:
                    s = base.copy()
                    pos = rng.choice(length, size=int(rng.integers(0, max_subs + 1)), replace=False)
                    s[pos] = (s[pos] + rng.integers(1, 4, size=len(pos))) % 4
                prev = s
                f.write(b">amp%07d;size=%d\n" % (n, int(rng.integers(1, 50))) + acgt[s].tobytes() + b"\n")
                n += 1
    return n


def main():
    import samples_e2e as se
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=400)
    ap.add_argument("--per-family", type=int, default=25)
    ap.add_argument("--length", type=int, default=250)
    ap.add_argument("--max-subs", type=int, default=3)
    ap.add_argument("--copies", type=float, default=0.2)
    ap.add_argument("--id", type=float, default=0.97)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--parent-cli", default="", help="burst_hip of the parent commit (optional)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_e2e.json"))
    a = ap.parse_args()
    wd = os.path.join(a.workdir, "cluster")
    os.makedirs(wd, exist_ok=True)
    fa = os.path.join(wd, "amplicons_%d_%d_%d.fa" % (a.families, a.per_family, a.length))
    n_reads = write_families(fa, a.families, a.per_family, a.length, a.max_subs, a.copies, 7)
    flags = ["-r", fa, "-q", fa, "-m", "FORAGE", "-i", str(a.id), "-fr"]
    legs = {"off": (CLI, []), "on": (CLI, ["--cluster", os.path.join(wd, "cl_"), "--cluster-sizes"])}
    if a.parent_cli:
        legs["parent_off"] = (a.parent_cli, [])
    outs = {leg: os.path.join(wd, "self_%s.b6" % leg) for leg in legs}
    se.run([CLI] + flags + ["-o", outs["off"]])      # (the file into the page cache)
    wall, lines = {leg: [] for leg in legs}, []
    for rep in range(a.reps):
        for leg, (cli, extra) in legs.items():
            t, text = se.run([cli] + flags + ["-o", outs[leg]] + extra)
            wall[leg].append(t)
            if leg == "on":
                lines += re.findall(r"^Clusters: (\d+) reads, (\d+) lines, (\d+) foreign lines, (\d+) edges kept, (\d+) centroids, (\d+) rounds, device ([0-9.]+) ms$", text, re.M)
        same = len({open(outs[leg], "rb").read() for leg in legs}) == 1
        sys.stderr.write("[cluster_e2e] rep %d: %s, outputs identical: %s\n" % (rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
        if not same:
            raise SystemExit("the outputs of the legs differ")
    res = {"what": "wall seconds of burst_hip -r reads.fa -q reads.fa -m FORAGE -i %s -fr (%d families of %d reads of %d bases, up to %d substitutions, %.0f %% exact copies) "
                   "without and with --cluster --cluster-sizes%s" % (a.id, a.families, a.per_family, a.length, a.max_subs, 100 * a.copies,
                                                                    ", and the parent commit's binary without it" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "reads": n_reads, "b6_lines": int(lines[0][1]) if lines else 0,
           "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs},
           "clusters_lines": {"device_ms": se.spread([float(x[6]) for x in lines]), "rounds": se.spread([int(x[5]) for x in lines]),
                              "edges_kept": int(lines[0][3]) if lines else 0, "centroids": int(lines[0][4]) if lines else 0},
           "outputs_identical": True}
    for o in outs.values():
        os.remove(o)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
