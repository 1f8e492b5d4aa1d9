#!/usr/bin/env python3
"""What --chimeras adds to a self-alignment: wall seconds of `burst_hip -r reads.fa -q reads.fa -m FORAGE -fr` without and with the flag on
the synthetic amplicon families of tools/cluster_e2e.py, made in sibling pairs (the second base a few evenly spread substitutions away from
the first) with about 2 % planted two-parent chimeras A[:c] + B[c:] of the siblings' bases, in alternated repetitions.  The identity cutoff
is lower than cluster_e2e's (0.95 for 0.97) so that a planted read still aligns end to end against both parents.  The bases carry
`;size=100`, the other reads 1 .. 49, the chimeras 1.  --parent-cli names the burst_hip of the parent commit: the same run without the
flag, in the same alternation -- the time with the flag off must not move.  The `Chimeras:` line gives the device milliseconds; the table
says how many planted reads came out `Y`.  The .b6 of all legs must be byte-identical.  One JSON document on standard output and in --out."""
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


def write_families(path, families, per_family, length, max_subs, copies, sibling_subs, chimera_share, seed):
    """families (in sibling pairs) x per_family reads of `length` bases: the base itself first, then reads 0 .. max_subs substitutions from
    it, `copies` of them exact copies of the read before; behind every pair its share of chimeras.  Returns (reads, planted: name -> the
    smaller number of sibling positions on either side of the cut)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    planted, n = {}, 0
    per_pair = chimera_share * 2 * per_family
    with open(path, "wb") as f:
        for pair in range(families // 2):
            a = rng.integers(0, 4, size=length)
            b = a.copy()
            sib = np.arange(sibling_subs) * (length // sibling_subs) + length // (2 * sibling_subs)
            b[sib] = (b[sib] + rng.integers(1, 4, size=len(sib))) % 4
            for base in (a, b):
                prev = base
                for k in range(per_family):
                    if k == 0:
                        s, size = base, 100
                    elif rng.random() < copies:
                        s, size = prev, int(rng.integers(1, 50))
                    else:
                        s = base.copy()
                        pos = rng.choice(length, size=int(rng.integers(0, max_subs + 1)), replace=False)
                        s[pos] = (s[pos] + rng.integers(1, 4, size=len(pos))) % 4
                        size = int(rng.integers(1, 50))
                    prev = s
                    f.write(b">amp%07d;size=%d\n" % (n, size) + acgt[s].tobytes() + b"\n")
                    n += 1
            for _ in range(int(per_pair) + (rng.random() < per_pair - int(per_pair))):
                c = int(rng.integers(length // 4, 3 * length // 4))
                name = "chim%07d;size=1" % n
                planted[name] = int(min((sib < c).sum(), (sib >= c).sum()))
                f.write(b">" + name.encode() + b"\n" + acgt[np.concatenate([a[:c], b[c:]])].tobytes() + b"\n")
                n += 1
    return n, planted


def main():
    import samples_e2e as se
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=400)
    ap.add_argument("--per-family", type=int, default=25)
    ap.add_argument("--length", type=int, default=250)
    ap.add_argument("--max-subs", type=int, default=3)
    ap.add_argument("--copies", type=float, default=0.2)
    ap.add_argument("--sibling-subs", type=int, default=10)
    ap.add_argument("--chimeras", type=float, default=0.02)
    ap.add_argument("--id", type=float, default=0.95)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workdir", default=os.environ.get("BURST_BENCH_DIR") or ("/dev/shm/burst_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/burst_amd_bench"))
    ap.add_argument("--parent-cli", default="", help="burst_hip of the parent commit (optional)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chimera_e2e.json"))
    a = ap.parse_args()
    wd = os.path.join(a.workdir, "chimera")
    os.makedirs(wd, exist_ok=True)
    fa = os.path.join(wd, "amplicons_%d_%d_%d.fa" % (a.families, a.per_family, a.length))
    n_reads, planted = write_families(fa, a.families, a.per_family, a.length, a.max_subs, a.copies, a.sibling_subs, a.chimeras, 7)
    flags = ["-r", fa, "-q", fa, "-m", "FORAGE", "-i", str(a.id), "-fr"]
    prefix = os.path.join(wd, "ch_")
    legs = {"off": (CLI, []), "on": (CLI, ["--chimeras", prefix, "--chimera-sizes"])}
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
                lines += re.findall(r"^Chimeras: (\d+) reads, (\d+) lines, (\d+) foreign lines, (\d+) pairs kept, (\d+) reads evaluated, (\d+) chimeric, device ([0-9.]+) ms$", text, re.M)
        same = len({open(outs[leg], "rb").read() for leg in legs}) == 1
        sys.stderr.write("[chimera_e2e] rep %d: %s, outputs identical: %s\n" % (rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
        if not same:
            raise SystemExit("the outputs of the legs differ")
    role = {c[0]: c[1] for c in (ln.split("\t") for ln in open(prefix + "chimeras.txt").read().splitlines()[1:])}
    gain = 3      # --chimera-min-gain's default: a planted read with fewer sibling positions on one side of its cut cannot reach it
    res = {"what": "wall seconds of burst_hip -r reads.fa -q reads.fa -m FORAGE -i %s -fr (%d families of %d reads of %d bases in sibling pairs %d substitutions apart, up to %d "
                   "substitutions per read, %.0f %% exact copies, %.0f %% planted two-parent chimeras) without and with --chimeras --chimera-sizes%s"
                   % (a.id, a.families, a.per_family, a.length, a.sibling_subs, a.max_subs, 100 * a.copies, 100 * a.chimeras,
                      ", and the parent commit's binary without it" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "reads": n_reads, "b6_lines": int(lines[0][1]) if lines else 0,
           "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs},
           "chimeras_lines": {"device_ms": se.spread([float(x[6]) for x in lines]), "pairs_kept": int(lines[0][3]) if lines else 0,
                              "evaluated": int(lines[0][4]) if lines else 0, "chimeric": int(lines[0][5]) if lines else 0},
           "planted": {"reads": len(planted), "flagged_Y": sum(1 for nm in planted if role.get(nm) == "Y"),
                       "with_at_least_%d_sibling_positions_on_both_sides" % gain: sum(1 for v in planted.values() if v >= gain),
                       "of_those_flagged_Y": sum(1 for nm, v in planted.items() if v >= gain and role.get(nm) == "Y"),
                       "other_reads_flagged_Y": sum(1 for nm, r in role.items() if r == "Y" and nm not in planted)},
           "outputs_identical": True}
    for o in outs.values():
        os.remove(o)
    os.remove(prefix + "chimeras.txt")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
