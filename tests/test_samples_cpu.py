"""A list of query files against one resident database (bh_session.c: host.Session, burst_hip --samples) where there is no device:
the session runs with the ORACLE as the ranks' align back end (BhMultiRank.align, handed the query tables of the sample being
searched), so everything around the kernels is the product's -- ingest ahead, bins, shear check, the ranks' ranges, record buffers
kept and grown across samples, the hand-over, the consolidation starting afresh per sample, the error rule -- and the outputs must
be the reference's golden files.  Short-long-short and long-short-long lists are there on purpose: buffers that must grow, then
larger stale state."""
import os
import subprocess
import sys

import numpy as np
import pytest

import goldenlib as gl

CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
Q100, Q292 = os.path.join(gl.G, "q100.fa"), os.path.join(gl.G, "q292.fa")
E_USAGE, E_IO = -1, -2

# the back end of the worker of tests/test_distributed_cpu.py, on the sample it is handed
ORACLE = r'''
def make_align(db):
    import numpy as np
    from burst_amd import capi, host
    import oraclelib as ol
    lut = ol.score_lut(1)
    clump_len = host._view(db.c.clumpLen, db.c.numRclumps, np.uint32)
    packed = host._view(db.c.packed, db.c.packedWords * 16, np.uint8)
    def align(qs, ranges, mode_no):
        parts = []
        for u0, u1 in ranges:
            q = qs.batch(u0, u1)
            h = ol.search(packed, clump_len, db.c.totR, q.codes, q.off, q.emac.astype(np.uint32), q.six, q.rc, q.n_shared, lut, mode_no == host.MODES["FORAGE"])
            h = h.copy(); h["q"] = q.entry_index[h["q"]].astype(np.uint32)      # local entry -> global entry
            parts.append(h.view(capi.HIT_DTYPE))
        h = np.concatenate(parts) if parts else np.zeros(0, capi.HIT_DTYPE)
        return h[np.lexsort((h["refIx"], h["q"]))]
    return align
'''
exec(ORACLE)


def golden(name):
    return gl.golden_lines([x for x in gl.cases() if x["name"] == name][0])


def run_list(db, files, tmp_path, tag, **kw):
    """the files through one session (the next one prefetched while the current one is searched): [(result, output path)]"""
    from burst_amd import host
    out = []
    with host.Session(db, None, accel=False, align=make_align(db), **kw) as s:
        for i, q in enumerate(files):
            if i + 1 < len(files):
                s.prefetch(files[i + 1])
            o = str(tmp_path / ("%s%d.b6" % (tag, i)))
            out.append((s.run(q, o), o))
        assert not s.ended
    return out


def test_session_with_oracle_backend_one_process(tmp_path):
    """1a: -m ALLPATHS -i 0.95 -fr, q100, q292, q100"""
    from burst_amd import host
    db = host.Db.read(EDX)
    kw = dict(mode="ALLPATHS", thres=0.95, rc=True)
    r = run_list(db, [Q100, Q292, Q100], tmp_path, "a", **kw)
    assert [x[0]["rc"] for x in r] == [0, 0, 0], r
    o = [open(x[1], "rb").read() for x in r]
    assert o[0] == o[2] and sorted(o[0].splitlines()) == golden("dna_q100_allpaths_noacx_fr")
    fresh = run_list(db, [Q292], tmp_path, "f", **kw)
    assert fresh[0][0]["rc"] == 0 and o[1] == open(fresh[0][1], "rb").read() and len(o[1]) > 0
    assert r[1][0]["nLines"] == len(o[1].splitlines()) and r[0][0]["totQ"] > 0
    db.close()


def test_session_capitalist_taxonomy_starts_afresh(tmp_path):
    """1c: -m CAPITALIST -b tax.txt, q100 twice: the vote and the interpolated taxonomy of sample 1 do not reach sample 2"""
    from burst_amd import host
    db = host.Db.read(EDX)
    r = run_list(db, [Q100, Q100], tmp_path, "c", mode="CAPITALIST", thres=0.95, rc=True, taxonomy=os.path.join(gl.G, "tax.txt"))
    want = golden("dna_q100_capitalist_tax_noacx_t1_fr")
    for res, o in r:
        assert res["rc"] == 0 and sorted(open(o, "rb").read().splitlines()) == want
    db.close()


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, torch.distributed as dist
from burst_amd import host
''' + ORACLE + r'''
edx, outdir, files = sys.argv[2], sys.argv[3], sys.argv[4:]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
db = host.Db.read(edx)
jt = torch.tensor([int.from_bytes(os.urandom(6), "little") if rank == 0 else 0], dtype=torch.int64)
dist.broadcast(jt, 0)
job = "ts%x" % int(jt.item())
node = host.Node(job, rank, world, 200000) if rank == 0 else None
dist.barrier()
if rank != 0:
    node = host.Node(job, rank, world, 200000)
with host.Session(db, None, mode="FORAGE", thres=0.95, rc=True, accel=False, align=make_align(db), rank=rank, world=world, node=node) as s:
    for i, q in enumerate(files):
        if i + 1 < len(files):
            s.prefetch(files[i + 1])
        res = s.run(q, os.path.join(outdir, "o%d.b6" % i))
        st = torch.tensor([res["rc"]], dtype=torch.int64)
        dist.all_reduce(st, op=dist.ReduceOp.MIN)
        assert int(st.item()) == 0, res
        assert (rank == 0) == (res["nLines"] > 0)       # only rank 0 reports and writes
    dist.barrier()
node.close()
dist.barrier()
assert not [f for f in os.listdir("/dev/shm") if job in f]
dist.destroy_process_group()
'''


def test_session_two_processes_over_gloo(tmp_path):
    """1b: two processes (query-sharded, the records meet in shared memory), -m FORAGE, q292, q100, q292"""
    import socket
    w = tmp_path / "worker.py"
    w.write_text(WORKER)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        str(w), gl.ROOT, EDX, str(tmp_path), Q292, Q100, Q292], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    for i, name in enumerate(["dna_q292_forage_noacx_t1_fr", "dna_q100_forage_noacx_t1_fr", "dna_q292_forage_noacx_t1_fr"]):
        assert sorted(open(str(tmp_path / ("o%d.b6" % i)), "rb").read().splitlines()) == golden(name), name
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("burst_hip.ts")]


def test_failing_sample_does_not_poison_the_next(tmp_path):
    """2: -i 0.85 against a database sheared for 336 symbols: the longest read of q100.fa divided by 0.85 fits, that of q292.fa does not
    (asserted from the header's shear and the loaded maxLen before it is relied on)"""
    from burst_amd import host
    db = host.Db.read(EDX)
    qa, qb = host.QuerySet(Q100, 0.85, rc=True, accel=False), host.QuerySet(Q292, 0.85, rc=True, accel=False)
    assert db.c.shear == 336 and int(np.float32(qa.c.maxLen) / np.float32(0.85)) <= db.c.shear < int(np.float32(qb.c.maxLen) / np.float32(0.85))
    qa.close(); qb.close()
    bad_fq = str(tmp_path / "bad.fq")
    open(bad_fq, "w").write("@r1\nACGTACGTACGTACGTACGTACGT\nIIII\nIIIIIIIIIIIIIIIIIIIIIIII\n")
    kw = dict(mode="ALLPATHS", thres=0.85, rc=True)
    r = run_list(db, [Q100, str(tmp_path / "missing.fa"), bad_fq, Q292, Q100], tmp_path, "e", **kw)
    assert [x[0]["rc"] for x in r] == [0, E_IO, E_USAGE, E_USAGE, 0], [(x[0]["rc"], x[0]["err"]) for x in r]
    assert "DB incompatible with selected queries/identity" in r[3][0]["err"] and "FASTQ" in r[2][0]["err"]
    one = run_list(db, [Q100], tmp_path, "g", **kw)
    a, b, c = (open(p, "rb").read() for p in (r[0][1], r[4][1], one[0][1]))
    assert a == b == c and len(a) > 0
    for k in (1, 2, 3):
        assert not os.path.exists(r[k][1])
    db.close()


def _cli(args, cwd):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=cwd, timeout=120)
    return r.returncode, r.stdout


def test_command_line_validation_without_a_device(tmp_path):
    """3: everything --samples refuses is refused before a device is touched, with the reference's exit codes, and creates nothing"""
    d = str(tmp_path)
    outs = []

    def lst(name, text):
        p = os.path.join(d, name)
        open(p, "w").write(text)
        return p

    def out(name):
        outs.append(os.path.join(d, name))
        return outs[-1]
    good = lst("good.txt", "# two samples\n\n%s\t%s\n%s\t%s\n" % (Q100, out("g1.b6"), Q292, out("g2.b6")))
    base = ["-r", EDX, "-m", "BEST", "-i", "0.95"]
    acx = os.path.join(d, "db.acx")
    usage = [
        base + ["--samples", good, "-q", Q100],
        base + ["--samples", good, "-o", out("x.b6")],
        ["-r", os.path.join(gl.G, "refs.fa"), "--samples", good, "-d", "QUICK"],
        base + ["--samples", good, "--make-acx", out("x.acx")],
        base + ["--samples", lst("one.txt", "%s\n" % Q100)],
        base + ["--samples", lst("three.txt", "%s\t%s\t%s\n" % (Q100, out("t1.b6"), out("t2.b6")))],
        base + ["--samples", lst("nofile.txt", "%s\t\n" % Q100)],
        base + ["--samples", lst("empty.txt", "# nothing\n\n")],
        base + ["--samples", lst("twice.txt", "%s\t%s\n%s\t%s\n" % (Q100, out("tw.b6"), Q292, outs[-1]))],
        base + ["--samples", lst("onquery.txt", "%s\t%s\n%s\t%s\n" % (Q100, out("oq.b6"), Q292, Q100))],
        base + ["--samples", lst("ondb.txt", "%s\t%s\n" % (Q100, EDX))],
        base + ["-a", acx, "--samples", lst("onacx.txt", "%s\t%s\n" % (Q100, acx))],
        base + ["--samples", lst("onlist.txt", "%s\t%s\n" % (Q100, os.path.join(d, "onlist.txt")))],
        # out of scope under --samples
        ["-r", os.path.join(gl.G, "refs.fa"), "--samples", good],
        base + ["--samples", good, "-x"],
        base + ["--samples", good, "--gather", "rccl"],
        base + ["--samples", good, "--gpus", "2", "--gather", "rccl"],
        base + ["--samples", good, "--gpus", "1", "--shards", "2"],
    ]
    sizes = {p: os.path.getsize(p) for p in (Q100, Q292, EDX)}
    for args in usage:
        code, text = _cli(args, d)
        assert code == 1 and "ERROR" in text, (args, code, text[-500:])
    code, text = _cli(base + ["--samples", os.path.join(d, "no_such_list.txt")], d)
    assert code == 2, text[-500:]
    assert "line 1" in _cli(usage[4], d)[1] and "line 2" in _cli(usage[8], d)[1]      # the message names the line
    assert not [p for p in outs if os.path.exists(p)] and not os.path.exists(acx)
    assert sizes == {p: os.path.getsize(p) for p in sizes} and open(os.path.join(d, "onlist.txt")).read().startswith(Q100)
    assert "--samples" in _cli(["-h"], d)[1]


COUNTER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from burst_amd import capi, host
db = host.Db.read(sys.argv[2])
files = sys.argv[4:]
def align(qs, ranges, mode_no):          # (what is counted are the tables around the search, not its records)
    return np.zeros(0, capi.HIT_DTYPE)
with host.Session(db, None, mode="BEST", thres=0.95, rc=True, accel=False, align=align) as s:
    for i, q in enumerate(files):
        if i + 1 < len(files):
            s.prefetch(files[i + 1])
        assert s.run(q, os.path.join(sys.argv[3], "m%d.b6" % i))["rc"] == 0
'''


@pytest.mark.parametrize("serial", [False, True])
def test_at_most_two_query_tables_alive(serial, tmp_path):
    """4: BURST_HOST_DEBUG=1 prints one line per query-table allocation and release; over six samples never more than two are alive
    (the current sample's and the prefetched one's), and with BURST_HOST_SERIAL_INGEST (no ingest thread, no prefetch) one"""
    env = dict(os.environ, BURST_HOST_DEBUG="1")
    env.pop("BURST_HOST_SERIAL_INGEST", None)
    if serial:
        env["BURST_HOST_SERIAL_INGEST"] = "1"
    r = subprocess.run([sys.executable, "-c", COUNTER, gl.ROOT, EDX, str(tmp_path), Q100, Q292, Q100, Q292, Q292, Q100], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[bh_session] query tables")]
    alive, peak = 0, 0
    for ln in lines:
        alive += 1 if " allocated: " in ln else -1
        assert 0 <= alive <= 2 and ln.endswith("(alive %d)" % alive), ln
        peak = max(peak, alive)
    assert alive == 0 and sum(" allocated: " in ln for ln in lines) == 6 and peak == (1 if serial else 2)
