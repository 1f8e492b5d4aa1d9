"""burst_hip --samples, host.Session and python -m burst_amd.run --samples on the MI355X: a list of query files against one resident
database.  The contract is per sample: exactly the .b6 a separate invocation of the same binary with the same flags writes for that
query file alone -- while the database is read, uploaded and (with -ad) indexed once."""
import os
import subprocess
import sys

import numpy as np
import pytest

import goldenlib as gl

pytestmark = pytest.mark.gpu
CLI = os.path.join(gl.ROOT, "burst_amd", "burst_hip")
EDX = os.path.join(gl.G, "dna.edx")
Q100, Q292 = os.path.join(gl.G, "q100.fa"), os.path.join(gl.G, "q292.fa")
TAX = os.path.join(gl.G, "tax.txt")
LIST3 = (Q100, Q292, Q100)
_acx, _runs, _singles, _n = {}, {}, {}, [0]


def acx_for(tmp):
    if "dna" not in _acx:
        path = os.path.join(tmp, "samples_dna_1.acx")
        subprocess.check_call([CLI, "-r", EDX, "--make-acx", path], stdout=subprocess.DEVNULL)
        _acx["dna"] = path
    return _acx["dna"]


def accel(kind, tmp):
    return ["-a", acx_for(tmp)] if kind == "a" else ["-ad"]


def fresh_dir(tmp):
    _n[0] += 1
    d = os.path.join(tmp, "s%d" % _n[0])
    os.makedirs(d)
    return d


def write_list(d, files):
    outs = [os.path.join(d, "o%d.b6" % i) for i in range(len(files))]
    lst = os.path.join(d, "list.txt")
    open(lst, "w").write("# queries<TAB>output\n\n" + "".join("%s\t%s\n" % p for p in zip(files, outs)))
    return lst, outs


def samples_run(tmp, kind, flags, files=LIST3, ident="0.95"):
    """one burst_hip --samples invocation (cached): exit status, standard output, the outputs' bytes (None = no file)"""
    key = (kind, tuple(flags), tuple(files), ident)
    if key not in _runs:
        d = fresh_dir(tmp)
        lst, outs = write_list(d, files)
        r = subprocess.run([CLI, "-r", EDX] + accel(kind, tmp) + ["--samples", lst, "-i", ident, "-fr"] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        _runs[key] = (r.returncode, r.stdout, [open(o, "rb").read() if os.path.exists(o) else None for o in outs])
    return _runs[key]


def single_run(tmp, kind, flags, q, ident="0.95", again=False):
    """the same binary, the same flags, that query file alone (-q / -o): the bytes it writes"""
    key = (kind, tuple(flags), q, ident)
    if key not in _singles or again:
        out = os.path.join(fresh_dir(tmp), "single.b6")
        r = subprocess.run([CLI, "-r", EDX] + accel(kind, tmp) + ["-q", q, "-o", out, "-i", ident, "-fr"] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:]
        got = open(out, "rb").read()
        if again:
            return got
        _singles[key] = got
    return _singles[key]


def case(name):
    return [x for x in gl.cases() if x["name"] == name][0]


RUNS = [("BEST", ["-m", "BEST"]), ("ALLPATHS", ["-m", "ALLPATHS"]), ("CAPITALIST", ["-m", "CAPITALIST"]), ("FORAGE", ["-m", "FORAGE"]), ("ANY", ["-m", "ANY"]),
        ("BEST_TAX", ["-m", "BEST", "-b", TAX])]


@pytest.mark.parametrize("kind", ["a", "ad"])
@pytest.mark.parametrize("name,flags", RUNS, ids=[r[0] for r in RUNS])
def test_per_sample_what_a_separate_invocation_writes(kind, name, flags, tmp_path_factory):
    """6 + 7: q100, q292, q100 through one invocation: every .b6 byte-identical to the single invocation's, sample 1 the golden lines;
    the database phases once, three sample blocks"""
    tmp = str(tmp_path_factory.getbasetemp())
    code, text, outs = samples_run(tmp, kind, flags)
    assert code == 0 and all(o is not None for o in outs), text[-3000:]
    singles = [single_run(tmp, kind, flags, q) for q in LIST3]
    found = "bytes"
    if name == "ANY":
        # single-device order is pinned byte for byte in the other four modes (test_cli_multi_gpu_paths); for ANY the single invocation
        # is run twice first, and the comparison is as strict as the single invocation is with itself
        twice = [single_run(tmp, kind, flags, q, again=True) for q in LIST3]
        if twice != singles:
            found = "sorted lines" if [sorted(x.splitlines()) for x in twice] == [sorted(x.splitlines()) for x in singles] else "goldenlib.compare"
        print("ANY: two single invocations agree in: %s" % found)
    if found == "bytes":
        assert outs == singles
    elif found == "sorted lines":
        assert [sorted(x.splitlines()) for x in outs] == [sorted(x.splitlines()) for x in singles]
    assert outs[0] == outs[2] or found != "bytes"
    # the goldens (sample 1; FORAGE: sample 2 as well), under the contract the single invocation is held to
    def nd(q, mode):      # the --no-dupe-hunt companion run of test_cli_matches_reference
        return sorted(single_run(tmp, kind, ["-m", mode, "--no-dupe-hunt"], q).splitlines())
    s1 = sorted(outs[0].splitlines())
    if name == "BEST":
        assert s1 == gl.golden_lines(case("dna_q100_best_fr"))
    elif name == "ALLPATHS":
        assert s1 == gl.golden_lines(case("dna_q100_allpaths_fr"))
    elif name == "BEST_TAX":
        assert s1 == gl.golden_lines(case("dna_q100_best_tax_fr"))
    elif name == "CAPITALIST":
        gl.compare(case("dna_q100_capitalist_fr"), s1, nd(Q100, "CAPITALIST"))
    elif name == "FORAGE":
        gl.compare(case("dna_q100_forage_fr"), s1, nd(Q100, "FORAGE"))
        gl.compare(case("dna_q292_forage_fr"), sorted(outs[1].splitlines()), nd(Q292, "FORAGE"))
    elif name == "ANY":
        gl.compare(case("dna_q100_any_fr"), s1, nd(Q100, "FORAGE"))
    # 7: the database is brought up once
    assert text.count("device database upload") == 1 and text.count("database read") == 1, text[-3000:]
    if kind == "ad":
        assert text.count("built on the device from the database") == 1
    assert sum(text.count("Sample %d/3: " % k) for k in (1, 2, 3)) == 3 and text.count("Wrote ") == 3 and "Samples: 3 done, 0 failed" in text


@pytest.mark.parametrize("kind,mode,flags,exact", [("a", "ALLPATHS", ["--batch", "37"], False),
                                                   ("a", "CAPITALIST", ["--gpus", "3", "--devices", "0,0,0", "--gather", "host"], False),
                                                   ("ad", "BEST", ["--gpus", "2", "--devices", "0,0", "--gather", "host", "--shard", "db"], True),
                                                   ("a", "FORAGE", ["--gpus", "4", "--devices", "0,0,0,0", "--gather", "host", "--shards", "2"], True)])
def test_small_batches_and_several_ranks(kind, mode, flags, exact, tmp_path_factory):
    """8: per sample the lines of the single-device --samples run; database-sharded runs byte for byte (the record set and its order are
    those of one device holding the whole database, as test_cli_multi_gpu_paths requires of a single sample)"""
    tmp = str(tmp_path_factory.getbasetemp())
    code0, text0, base = samples_run(tmp, kind, ["-m", mode])
    code, text, outs = samples_run(tmp, kind, ["-m", mode] + flags)
    assert code0 == 0 and code == 0 and all(o is not None for o in outs), text[-3000:]
    if "--gpus" in flags:
        assert text.count("host gather: %s rank(s)" % flags[flags.index("--gpus") + 1]) == 3 and text.count("device database upload") == 1, text[-3000:]
    if exact:
        assert outs == base
    assert [sorted(o.splitlines()) for o in outs] == [sorted(o.splitlines()) for o in base] and len(outs[0]) > 0


def test_failure_in_the_middle_on_the_device_path(tmp_path_factory, tmp_path):
    """9: q100, a missing file, a FASTQ whose third line lacks '+', q292 (too long for the database's shear at -i 0.85), q100"""
    tmp = str(tmp_path_factory.getbasetemp())
    bad_fq = str(tmp_path / "bad.fq")
    open(bad_fq, "w").write("@r1\nACGTACGTACGTACGTACGTACGT\nIIII\nIIIIIIIIIIIIIIIIIIIIIIII\n")
    files = (Q100, str(tmp_path / "missing.fa"), bad_fq, Q292, Q100)
    code, text, outs = samples_run(tmp, "a", ["-m", "ALLPATHS"], files=files, ident="0.85")
    assert code == 2, text[-3000:]                      # the first failure is the missing file
    assert outs[0] is not None and outs[0] == outs[4] and len(outs[0]) > 0 and outs[1:4] == [None, None, None]
    assert outs[0] == single_run(tmp, "a", ["-m", "ALLPATHS"], Q100, ident="0.85")
    for k, c in ((2, 2), (3, 1), (4, 1)):
        assert "Sample %d/5 FAILED (exit code %d)" % (k, c) in text, text[-3000:]
    assert "DB incompatible with selected queries/identity" in text and "Samples: 2 done, 3 failed" in text
    assert text.count("device database upload") == 1


def _launcher_env(**kw):
    env = dict(os.environ, PYTHONPATH=gl.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **kw)
    return env


def test_launcher_samples_single_process(tmp_path_factory, tmp_path):
    """10a: python -m burst_amd.run --samples with one process"""
    tmp = str(tmp_path_factory.getbasetemp())
    code0, text0, base = samples_run(tmp, "a", ["-m", "ALLPATHS"])
    lst, outs = write_list(str(tmp_path), LIST3)
    env = _launcher_env()
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", EDX, "-a", acx_for(tmp), "--samples", lst, "-m", "ALLPATHS", "-i", "0.95", "-fr"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=gl.ROOT, timeout=600)
    assert r.returncode == 0 and code0 == 0 and "Samples: 3 done, 0 failed" in r.stdout, r.stdout[-3000:]
    assert [sorted(open(o, "rb").read().splitlines()) for o in outs] == [sorted(b.splitlines()) for b in base]


def test_launcher_samples_two_processes_grow_the_handover(tmp_path_factory, tmp_path):
    """10b: two processes on one device over gloo; the middle sample (120 000 synthetic reads) needs larger segments than the first:
    the hand-over is reopened under a fresh job name, the third sample runs through the larger one; nothing is left in /dev/shm"""
    from burst_amd import host
    tmp = str(tmp_path_factory.getbasetemp())
    big = str(tmp_path / "big.fa")
    host.synth_reads(os.path.join(gl.G, "refs.fa"), big, 120000, 100, [0, 1, 2], rc=True, seed=7)
    files = (Q100, big, Q100)
    code0, text0, base = samples_run(tmp, "a", ["-m", "FORAGE"], files=files)
    assert code0 == 0, text0[-3000:]
    lst, outs = write_list(str(tmp_path), files)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29633",
           "-m", "burst_amd.run", "-r", EDX, "-a", acx_for(tmp), "--samples", lst, "-m", "FORAGE", "-i", "0.95", "-fr"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=_launcher_env(BURST_RUN_DEVICE="0"), cwd=gl.ROOT, timeout=900)
    assert r.returncode == 0 and r.stdout.count("from 2 rank(s)") == 3, r.stdout[-3000:]
    assert r.stdout.count("hand-over: shared-memory segments") == 2, r.stdout[-3000:]
    assert [sorted(open(o, "rb").read().splitlines()) for o in outs] == [sorted(b.splitlines()) for b in base] and len(base[1]) > len(base[0])
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("burst_hip.run")]


@pytest.mark.parametrize("mode", ["BEST", "FORAGE"])
def test_the_hot_path_is_untouched(mode, tmp_path_factory, tmp_path):
    """11: the device counters of a sample that went through a session equal those of host.align_ranges on the same queries"""
    from burst_amd import host
    tmp = str(tmp_path_factory.getbasetemp())
    db = host.Db.read(EDX, acx_for(tmp))
    dev = db.open_device(0)
    with host.Session(db, dev, mode=mode, thres=0.95, rc=True) as s:
        res = s.run(Q100, str(tmp_path / "o.b6"))
        assert res["rc"] == 0 and res["nLines"] > 0, res
    qs = host.QuerySet(Q100, 0.95, rc=True, accel=True, K=int(db.c.K))
    run = host.align_ranges(dev, qs, [(0, qs.n_uniq)], mode, 1 << 21)
    want = run.stats()
    for k in ("n_pairs", "n_raw_hits", "n_hits", "n_lane_tasks", "myers_launches", "prefilter_launches"):
        assert res["stats"][k] == want[k], (k, res["stats"][k], want[k])
    assert res["nHits"] == int(run.c.nHits) and want["n_hits"] > 0
    run.close(); qs.close(); dev.close(); db.close()
