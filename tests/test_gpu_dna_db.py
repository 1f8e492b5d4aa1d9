"""The duplicate marks of the compressive build (-d DNA) on the device (bhip_dna_marks, burst_amd/csrc/bhip_dnadb.hip): the golden
databases through the product path, and the device's flags and tally against the host restatement (bh_dna_marks_host) byte for
byte -- on strain families, tandem repeats and IUPAC codes, at several windows and partitions, with forced small chunks, with a
weak hash (the exact path), and under poisoned allocations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")
D = os.path.join(G, "dna_cases")
CLI = os.path.join(ROOT, "burst_amd", "burst_hip")
REF = os.path.join(ROOT, "oracle", "_ref", "burst12")
CASES = json.load(open(os.path.join(G, "dna_cases.json")))

pytestmark = pytest.mark.gpu


def device_env(**extra):
    env = {k: v for k, v in os.environ.items() if k != "BURST_HOST_DNA_MARKS"}
    env.update(extra)
    return env


def run(args, env):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_on_device(tmp_path, name):
    c = CASES[name]
    edx, acx = str(tmp_path / "x.edx"), str(tmp_path / "x.acx")
    r = run(["-r", os.path.join(D, c["input"]), "-o", edx, "-a", acx] + c["args"], device_env())
    assert r.returncode == 0, r.stdout
    assert "duplicate marks computed on device 0" in r.stdout, r.stdout
    assert open(edx, "rb").read() == open(os.path.join(D, c["edx"]), "rb").read()
    import hashlib
    assert hashlib.sha256(open(acx, "rb").read()).hexdigest() == c["acx_sha256"]


def test_golden_dna_edx_on_device(tmp_path):
    edx = str(tmp_path / "x.edx")
    r = run(["-r", os.path.join(G, "refs.fa"), "-d", "DNA", "320", "-o", edx, "-s", "500", "-i", "0.95"], device_env())
    assert r.returncode == 0 and "duplicate marks computed on device 0" in r.stdout, r.stdout
    assert open(edx, "rb").read() == open(os.path.join(G, "dna.edx"), "rb").read()


def test_poisoned_allocations(tmp_path):
    c = CASES["chain_t0"]
    edx = str(tmp_path / "x.edx")
    r = run(["-r", os.path.join(D, c["input"]), "-o", edx] + c["args"], device_env(BHIP_POISON="165"))
    assert r.returncode == 0 and "duplicate marks computed on device 0" in r.stdout, r.stdout
    assert open(edx, "rb").read() == open(os.path.join(D, c["edx"]), "rb").read()


def layout(seqs):
    """the DNA-mode symbol layout: one array, a single 0 between consecutive sequences"""
    starts, off = [], 0
    for s in seqs:
        starts.append(off)
        off += len(s) + 1
    sym = np.zeros(off, np.uint8)
    for s, a in zip(seqs, starts):
        sym[a:a + len(s)] = s
    return sym, np.array(starts, np.uint64), np.array([len(s) for s in seqs], np.uint32)


def inputs():
    from burst_amd import host
    rng = np.random.default_rng(7)
    out = {}
    fa = "/tmp/burst_dna_gpu_strains_%d.fa" % os.getpid()
    host.synth_refs(fa, 6, 6, 3000, 0.003, 11)
    seqs, cur = [], []
    c2n = np.zeros(256, np.uint8)
    for i, ch in enumerate(b".ACGTNKMRYSWBVHD"):
        c2n[ch] = i
    for line in open(fa, "rb"):
        if line.startswith(b">"):
            if cur:
                seqs.append(c2n[np.frombuffer(b"".join(cur), np.uint8)])
            cur = []
        else:
            cur.append(line.strip().upper())
    if cur:
        seqs.append(c2n[np.frombuffer(b"".join(cur), np.uint8)])
    os.unlink(fa)
    out["strains"] = seqs
    rep = []
    for k in range(8):
        unit = rng.integers(1, 5, size=int(rng.integers(1, 9)), dtype=np.uint8)
        body = np.tile(unit, 4000 // len(unit))
        rep.append(np.concatenate([rng.integers(1, 5, 300, dtype=np.uint8), body, rng.integers(1, 5, 300, dtype=np.uint8)]))
    rep += [r.copy() for r in rep[:3]]
    out["repeats"] = rep + seqs[:6]
    iu = [s.copy() for s in seqs[:12]]
    for s in iu:
        m = np.flatnonzero(rng.random(len(s)) < 0.02)
        s[m] = rng.integers(0, 16, size=len(m))
    out["iupac"] = iu
    return out


def partitions(n, P):
    r = n // P + (n % P != 0)
    return [(a, min(n, a + r)) for a in range(0, n, r)]


def compare(seqs, W, P, **env):
    from burst_amd import capi, host
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sym, rs, rl = layout(seqs)
        hs = ds = (0, 0)
        exact = 0
        for a, b in partitions(len(seqs), P):
            base = int(rs[a])
            end = int(rs[b - 1]) + int(rl[b - 1])
            part, prs = sym[base:end], rs[a:b] - np.uint64(base)
            hf, hc, hsh = host.dna_marks(part, prs, rl[a:b], W, *hs)
            df, dc, dsh, info = capi.dna_marks(part, prs, rl[a:b], W, *ds)
            assert (hc, hsh) == (dc, dsh), (W, P, a, hc, hsh, dc, dsh)
            assert np.array_equal(hf, df), (W, P, a, np.flatnonzero(hf != df)[:10])
            hs, ds = (hc, hsh), (dc, dsh)
            exact += int(info[2])
        return hs, exact
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def synthetic():
    return inputs()


@pytest.mark.parametrize("kind", ["strains", "repeats", "iupac"])
@pytest.mark.parametrize("W,P", [(24, 1), (200, 1), (658, 2), (836, 3)])
def test_device_flags_equal_host(synthetic, kind, W, P):
    (mc, ms), _ = compare(synthetic[kind], W, P)
    if kind == "repeats" and P == 1:
        assert mc > 0 and ms > 0


def test_small_chunks(synthetic):
    compare(synthetic["repeats"], 300, 1, BURST_DNA_CHUNK="1000")
    compare(synthetic["strains"], 836, 2, BURST_DNA_CHUNK="1")


def test_weak_hash_takes_the_exact_path(synthetic):
    _, exact = compare(synthetic["repeats"], 300, 1, BURST_DNA_WEAK_HASH="1")
    assert exact > 0
    _, exact = compare(synthetic["strains"], 120, 2, BURST_DNA_WEAK_HASH="1", BURST_DNA_CHUNK="5000")
    assert exact > 0


@pytest.mark.skipif(not os.path.exists(REF), reason="no compiled reference (oracle/_ref/burst12)")
def test_differential_on_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dna_db_diff.py"), "--seed", "5", "--", "-d", "DNA", "120", "-s", "200", "-i", "0.97"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=device_env(), timeout=600)
    assert r.returncode == 0 and "on device 0" in r.stdout, r.stdout
