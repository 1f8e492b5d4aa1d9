#!/usr/bin/env python3
"""Micro-run behind EM_THREAD_MAX / EM_WAVE_MAX of csrc/bhip_em.hip: microseconds per iteration of bhip_em_run with every class forced onto
one kernel path (options em_thread_max / em_wave_max), per candidate-set size, and a synthetic sample shaped like the `strains` profile.
Needs an MI355X.  One JSON document in the file named by the first argument (default profiles/abundance_thresholds.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbutil
import oraclelib as ol
from burst_amd import capi

rng = np.random.default_rng(3)
seqs = [rng.integers(1, 5, size=int(n), dtype=np.uint8) for n in rng.integers(90, 400, size=40)]
packed, clump_len, tot = dbutil.pack_clumps(seqs)
dev = capi.Device(packed, clump_len, tot, ol.score_lut(1))

def make(C, s, H):
    refs = rng.integers(0, H, size=(C, s), dtype=np.int64)
    ln = np.zeros(C * s, capi.EM_LINE_DTYPE)
    ln["group"] = np.repeat(np.arange(C), s); ln["ref"] = refs.reshape(-1)
    # single-candidate groups beside them, as on real inputs
    single = np.zeros(C, capi.EM_LINE_DTYPE); single["group"] = C + np.arange(C); single["ref"] = rng.integers(0, H, size=C)
    return H, np.ones(2 * C, np.uint32), np.concatenate([ln, single])

def per_iter(case, opts):
    for k, v in opts.items(): dev.set_option(k, v)
    best = None
    for rep in range(3):
        _, a = dev.em_run(*case, max_iters=8, tol=0)
        _, b = dev.em_run(*case, max_iters=40, tol=0)
        if int(b[0]) > int(a[0]):
            us = (int(b[5]) - int(a[5])) / (int(b[0]) - int(a[0]))
            best = us if best is None else min(best, us)
    for k in opts: dev.set_option(k, 0)
    return best, int(b[0]), int(b[2])

out = {"thread_vs_wave": [], "wave_vs_block": []}
dev.em_run(*make(100000, 2, 1 << 16), max_iters=8, tol=0)      # (the process's first call pays for the allocations)
for s in (2, 3, 4, 6, 8, 12, 16, 28, 48):
    case = make(100000, s, 1 << 16)
    t, it, cls = per_iter(case, {"em_thread_max": 64})
    w, _, _ = per_iter(case, {"em_thread_max": 1, "em_wave_max": 1 << 24})
    out["thread_vs_wave"].append({"set_size": s, "classes": cls, "iterations": it, "thread_us_per_iter": t, "wave_us_per_iter": w})
    print(out["thread_vs_wave"][-1], flush=True)
for s, C in ((256, 4000), (1024, 2000), (2048, 1000), (4096, 500), (16384, 200), (65536, 50)):
    case = make(C, s, 1 << 20)
    w, it, cls = per_iter(case, {"em_thread_max": 1, "em_wave_max": 1 << 24})
    b, _, _ = per_iter(case, {"em_thread_max": 1, "em_wave_max": 1})
    out["wave_vs_block"].append({"set_size": s, "classes": cls, "iterations": it, "wave_us_per_iter": w, "block_us_per_iter": b})
    print(out["wave_vs_block"][-1], flush=True)
# a "strains"-like sample: 2 M reads, 85 % on one reference, the rest tied on about 28 of 20 000
C = 300000
case = make(C, 28, 20000)
for name, opts in (("built-in", {}), ("all-wave", {"em_thread_max": 1, "em_wave_max": 1 << 24})):
    for k, v in opts.items(): dev.set_option(k, v)
    t0 = time.time(); _, info = dev.em_run(*case, max_iters=1000, tol=1024); wall = time.time() - t0
    for k in opts: dev.set_option(k, 0)
    out["strains_like_" + name] = {"lines": len(case[2]), "iterations": int(info[0]), "classes": int(info[2]), "device_us": int(info[5]), "wall_s": wall, "peak_bytes": int(info[6])}
    print(name, out["strains_like_" + name], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "abundance_thresholds.json"), "w"), indent=1)
dev.close()
