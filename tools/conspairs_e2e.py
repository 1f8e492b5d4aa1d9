#!/usr/bin/env python3
"""What --consensus and --consensus-pairs add to a study: wall seconds of `burst_hip --samples LIST -m BEST` in four legs -- --consensus
off, --consensus on, --consensus --consensus-pairs, and (with --parent-cli, the burst_hip of the parent commit) the parent's binary with
--consensus on -- in three alternated repetitions, on the --samples set-up of tools/variants_e2e.py (bench.py's database, synthetic
reads) with TWO DEEP SAMPLES, deep enough to call: `depth` reads over one window of each of the first `windows` references, the second
from a haplotype with three substitutions per window, so that the two differ by planted substitutions; the further samples are shallow.
The .b6 outputs of all legs and the consensus files of the three legs that write them must be byte-identical.  From the run's own lines:
the `consensus pairs` phase, the `ConsensusPairs:` line (records, headers, union positions, pairs, host bytes kept, device milliseconds).

--micro adds a run of the primitive alone on synthetic segments: one fully called header of --micro-long positions (default 4 Mb)
across 64 samples plus --micro-headers (default 20 000) headers of 1.5 kb across 64 samples: the device time of bhip_consensus_pairs
(its own figure and the wall time of the call), and beside it, for scale, the single-thread time of bh_consensus_pairs_host on the same
input (--micro-host 0 leaves it out: it walks samples^2 x positions).  No time is fixed in advance: the record states what was measured
and the spread.  One JSON document on standard output and in --out."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")
PAIRS_LINE = re.compile(r"^ConsensusPairs: (\d+) samples done, (\d+) failed, (\d+) records, (\d+) headers with two or more, (\d+) union positions, (\d+) pairs examined, "
                        r"(\d+) written, (\d+) host bytes kept, device ([0-9.]+) ms$", re.M)
PAIRS_PHASE = re.compile(r"^ \[consensus pairs\s+([0-9.]+) s\]$", re.M)
PLANTED = (200, 260, 320)


def deep_sample(refs, path, windows, depth, planted, seed=5):
    """`depth` reads of 100 symbols over the window 160 .. 440 of each of the first `windows` references; with `planted` they come from a
    haplotype with a substitution at each of PLANTED"""
    import numpy as np
    import vcf_e2e as ve
    rng = np.random.default_rng(seed)
    n = 0
    with open(path, "w") as f:
        for w, (_, seq) in enumerate(ve.first_records(refs, windows)):
            if len(seq) < 600:
                continue
            src = seq
            if planted:
                for p in PLANTED:
                    src = src[:p] + "CGTA"["ACGT".find(src[p].upper())] + src[p + 1:]
            for k in range(depth):
                s = int(rng.integers(160, 340))
                f.write(">deep_w%d_r%d\n%s\n" % (w, k, src[s:s + 100]))
                n += 1
    return n


def micro_input(n_samples, long_len, n_headers, short_len, seed=3):
    """header 0: one segment of long_len per sample; headers 1 .. n_headers: one of short_len.  Letters A C G T with one in 200 changed per
    sample, so that the pairs differ"""
    import numpy as np
    from burst_amd import capi
    rng = np.random.default_rng(seed)
    total = long_len + n_headers * short_len
    base = rng.integers(0, 4, size=total, dtype=np.uint8)
    segs = np.zeros(n_samples * (1 + n_headers), capi.PAIR_SEG_DTYPE)
    letters = np.zeros(n_samples * total, np.uint8)
    lut = np.frombuffer(b"ACGT", np.uint8)
    lens = np.concatenate(([long_len], np.full(n_headers, short_len, np.int64)))
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    for s in range(n_samples):
        row = base.copy()
        hit = rng.integers(0, total, size=total // 200)
        row[hit] = (row[hit] + 1) % 4
        letters[s * total:(s + 1) * total] = lut[row]
        k = slice(s * (1 + n_headers), (s + 1) * (1 + n_headers))
        segs["sample"][k], segs["header"][k], segs["pos"][k], segs["len"][k], segs["off"][k] = s, np.arange(1 + n_headers), 1, lens, s * total + offs
    return segs, letters


def run_micro(a, se):
    """the primitive alone on the synthetic segments"""
    import numpy as np
    from burst_amd import capi, host
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dbutil
    import oraclelib as ol
    n = 64
    segs, letters = micro_input(n, a.micro_long, a.micro_headers, 1500)
    rng = np.random.default_rng(2)
    packed, clump_len, tot = dbutil.pack_clumps([rng.integers(1, 5, size=200, dtype=np.uint8) for _ in range(4)])
    dev = capi.Device(packed, clump_len, tot, ol.score_lut(1), device=0)
    cap = (1 + a.micro_headers) * n * (n - 1) // 2
    wall, dev_ms, infos = [], [], None
    for rep in range(a.reps + 1):      # (the first call makes the buffers: left out)
        t0 = time.perf_counter()
        pairs = dev.consensus_pairs(n, segs, letters, 1, pair_cap=cap)
        t = time.perf_counter() - t0
        infos = dev.consensus_pairs_info()
        if rep:
            wall.append(t)
            dev_ms.append(infos["device_us"] / 1e3)
    dev.close()
    out = {"samples": n, "long_header_positions": a.micro_long, "short_headers": a.micro_headers, "short_header_positions": 1500, "pairs": int(len(pairs)),
           "union_positions": infos["union_positions"], "peak_device_bytes": infos["peak_bytes"], "device_ms": se.spread(dev_ms), "call_wall_seconds": se.spread(wall)}
    if a.micro_host:
        t0 = time.perf_counter()
        want, _ = host.consensus_pairs_host(n, segs, letters, 1, pair_cap=cap)
        out["host_single_thread_seconds"] = time.perf_counter() - t0
        out["host_equals_device"] = bool(want.tobytes() == pairs.tobytes())
    return out


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
    ap.add_argument("--micro", action="store_true", help="also the primitive alone on synthetic segments")
    ap.add_argument("--micro-long", type=int, default=4000000)
    ap.add_argument("--micro-headers", type=int, default=20000)
    ap.add_argument("--micro-host", type=int, default=1)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conspairs_e2e.json"))
    a = ap.parse_args()
    res = {"what": "wall seconds of burst_hip --samples (two deep samples of %d windows x %d reads, the second with %d planted substitutions per window, %d samples of %d reads; "
                   "-ad -k %d -m BEST -i %s) without --consensus, with it, with --consensus --consensus-pairs%s" %
                   (a.windows, a.depth, len(PLANTED), max(a.samples - 2, 0), a.reads, a.K, a.id, ", and the parent commit's binary with --consensus" if a.parent_cli else ""),
           "commit": a.commit, "reps": a.reps, "profiles": {}}
    for profile in [p for p in a.profiles.split(",") if p]:      # (--profiles "" --micro: the primitive alone)
        wd = os.path.join(a.workdir, profile)
        b = argparse.Namespace(read_len=100, n_base=int(1600000 * a.db_scale), n_variants=2, ref_len=1400, variant_rate=0.05, id=a.id, K=a.K, db_profile=profile,
                               reads=a.reads, pool=1, edits="0,1,2", fr=False, iupac=0.0, drop_refs=False)
        refs, edx, acx, done = bench.build_db(wd, b)
        if not os.path.exists(refs):
            host.synth_refs(refs, b.n_base, b.n_variants, b.ref_len, b.variant_rate, 7)
        files, n_deep = [], 0
        for planted in (False, True):
            deep = os.path.join(wd, "cp_deep_w%d_d%d_%d.fa" % (a.windows, a.depth, planted))
            n_deep = deep_sample(refs, deep, a.windows, a.depth, planted)
            files.append(deep)
        for k in range(2, a.samples):
            fa = os.path.join(wd, "sample_%d_of_%d_r%d.fa" % (k, a.samples, a.reads))
            if not os.path.exists(fa + ".done"):
                host.synth_reads(refs, fa, a.reads, 100, [0, 1, 2], rc=False, seed=42, first_read=k * a.reads)
                open(fa + ".done", "w").write("ok")
            files.append(fa)
        flags = ["-r", edx, "-ad", "-k", str(a.K), "-m", "BEST", "-i", str(a.id)]
        legs = {"off": (CLI, lambda p: []), "consensus": (CLI, lambda p: ["--consensus", p]), "pairs": (CLI, lambda p: ["--consensus", p, "--consensus-pairs"])}
        if a.parent_cli:
            legs["parent_consensus"] = (a.parent_cli, lambda p: ["--consensus", p])
        outs = {leg: [os.path.join(wd, "cp_%s" % leg, "s%d.b6" % k) for k in range(len(files))] for leg in legs}      # (the same sample names in every leg)
        prefix = {leg: os.path.join(wd, "cp_%s" % leg, "P_") for leg in legs}
        lists = {}
        for leg in legs:
            os.makedirs(os.path.join(wd, "cp_%s" % leg), exist_ok=True)
            lists[leg] = os.path.join(wd, "cplist_%s.txt" % leg)
            open(lists[leg], "w").write("".join("%s\t%s\n" % p for p in zip(files, outs[leg])))
        se.run([CLI] + flags + ["--samples", lists["off"]])      # (the files into the page cache)
        wall = {leg: [] for leg in legs}
        line, phase = [], []
        for rep in range(a.reps):
            for leg, (cli, extra) in legs.items():
                t, text = se.run([cli] + flags + ["--samples", lists[leg]] + extra(prefix[leg]))
                wall[leg].append(t)
                if leg == "pairs":
                    found, ph = PAIRS_LINE.findall(text), PAIRS_PHASE.findall(text)
                    if len(found) != 1:
                        raise SystemExit("%d ConsensusPairs: lines in one run" % len(found))
                    line.append(found[0])
                    phase += [float(x) for x in ph]
            same = all(len({open(outs[leg][k], "rb").read() for leg in legs}) == 1 for k in range(len(files)))
            same = same and all(len({open(prefix[leg] + sfx, "rb").read() for leg in legs if leg != "off"}) == 1 for sfx in ("consensus.fa", "consensus.txt"))
            sys.stderr.write("[conspairs_e2e] %s rep %d: %s, outputs identical: %s\n" % (profile, rep, ", ".join("%s %.2f s" % (leg, wall[leg][-1]) for leg in legs), same))
            if not same:
                raise SystemExit("the outputs of the legs differ")
        differ = [ln.split("\t") for ln in open(prefix["pairs"] + "consensus_pairs.txt").read().split("\n")[1:] if ln]
        names = ("samples_done", "samples_failed", "records", "headers", "union_positions", "pairs_examined", "pairs_written", "host_bytes_kept", "device_ms")
        res["profiles"][profile] = {
            "edx_bytes": os.path.getsize(edx), "reads_per_deep_sample": n_deep, "reads_per_further_sample": a.reads,
            "wall_seconds": {leg: se.spread(wall[leg]) for leg in legs},
            "pairs_phase_seconds": se.spread(phase) if phase else None,
            "pairs_line": {name: se.spread([(float if name == "device_ms" else int)(x[k]) for x in line]) for k, name in enumerate(names)},
            "differ_between_the_deep_samples": sum(int(r[6]) for r in differ if r[1] == "s0" and r[2] == "s1"),
            "consensus_fa_bytes": os.path.getsize(prefix["pairs"] + "consensus.fa"),
            "outputs_identical": True}
        for leg in legs:
            for o in outs[leg]:
                os.remove(o)
            for sfx in ("consensus.fa", "consensus.txt", "consensus_pairs.txt", "consensus_identity.txt", "consensus_compared.txt"):
                if os.path.exists(prefix[leg] + sfx):
                    os.remove(prefix[leg] + sfx)
    if a.micro:
        res["micro"] = run_micro(a, se)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
