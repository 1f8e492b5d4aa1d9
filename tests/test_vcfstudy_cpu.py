"""The study VCF without a device: bh_site_counts_host (bhip_site_counts' definition in plain sequential C) against vcfstudylib (dictionary
counts) on the pool of the variants tests and on ranges written by hand for every edge; the collector and the writer of bh_vcfstudy.c
through their C entry points with the three host solvers and three samples -- one with edits of all three kinds, one that covers the same
windows unedited, one that lies elsewhere -- the file's bytes, OUT.vcf unchanged, OUT.vcf as a projection of the study file; a failed
sample, a solver error, two samples of one name; the refusals of the command line; the host file under the sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarlib as cg
import pilecases
import test_vcf_cpu as tv
import vcfstudycases as vc
import vcfstudylib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")
CONTIGS = list(zip(tv.SN, tv.LENGTHS))


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


@pytest.fixture(scope="module")
def pool(L):
    return tv.Pool(L, 1)


# ---- bh_site_counts_host = the model -------------------------------------------------------------------------------------------------------
def test_yardstick_on_ranges_written_by_hand():
    from burst_amd import host
    ranges, sites, alleles, records, want = vc.hand()
    got = host.site_counts_host(*vc.to_arrays(ranges, sites, alleles, records))
    assert vc.cells_as_tuples(got) == want


@pytest.mark.parametrize("n", [1, 65, 700])
def test_yardstick_on_the_pool(pool, n):
    from burst_amd import host
    rng = np.random.default_rng(n)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=n)] if n < 700 else list(range(len(pool.cases)))
    arrays, want = vc.sample_case(pool.model_lines(idx), rng)
    got = vc.cells_as_tuples(host.site_counts_host(*arrays))
    assert got == want
    if n == 700:      # what the pool has to yield: sites and alleles found and not found, depth with and without a site
        sites, alleles, records = arrays[1], arrays[2], arrays[3]
        assert len(sites) > 100 and len(alleles) > 100 and len(records) > 3000
        assert any(d and c for d, _, c in want) and any(d and not c and not any(n4) for d, n4, c in want) and any(not d for d, _, _ in want)
        assert any(d and sum(n4) == d and max(n4) == d for d, n4, _ in want) and any(d and max(n4) < d for d, n4, _ in want if any(n4))


def test_a_permutation_of_ranges_and_records_changes_nothing():
    from burst_amd import host
    r, s, a, q = vc.random_case(500, 800, 5)
    rng = np.random.default_rng(6)
    base = host.site_counts_host(r, s, a, q)
    assert base["depth"].max() > 4 and base["count"].max() > 0
    pr, pq = rng.permutation(len(r)), rng.permutation(len(q))
    assert host.site_counts_host(r[pr], s, a, q).tobytes() == base.tobytes()
    assert host.site_counts_host(r, s, a, q[pq]).tobytes() == base[pq].tobytes()
    assert len(host.site_counts_host(r, s, a, q[:0])) == 0 and not host.site_counts_host(r[:0], s[:0], a[:0], q)["depth"].any()


BAD = [("range 1: position 0", lambda r, s, a, q: r["pos"].__setitem__(1, 0)), ("range 1 has weight 0", lambda r, s, a, q: r["w"].__setitem__(1, 0)),
       ("range 1: position 4294967290 + span 6", lambda r, s, a, q: (r["pos"].__setitem__(1, vc.TOP - 5), r["span"].__setitem__(1, 6))),
       ("more than 2^31 - 1 reads", lambda r, s, a, q: r["w"].__setitem__(slice(0, 2), 1 << 30)),
       ("sites not strictly ascending", lambda r, s, a, q: s.__setitem__(1, s[0])), ("alleles not strictly ascending", lambda r, s, a, q: a.__setitem__(1, a[0])),
       ("record 2 has position 0", lambda r, s, a, q: q["pos"].__setitem__(2, 0)),
       ("site record 0 has ref 5", lambda r, s, a, q: (q["allele"].__setitem__(0, 0), q["ref"].__setitem__(0, 5))),
       ("site record 0 has ref 0", lambda r, s, a, q: (q["allele"].__setitem__(0, 0), q["ref"].__setitem__(0, 0)))]


@pytest.mark.parametrize("text,spoil", BAD, ids=[b[0] for b in BAD])
def test_the_yardstick_refuses_what_the_device_refuses(text, spoil):
    from burst_amd import host
    r, s, a, q = vc.random_case(20, 20, 1)
    spoil(r, s, a, q)
    with pytest.raises(host.HostError) as e:
        host.site_counts_host(r, s, a, q)
    assert text in str(e.value)


def test_the_abi_version_stays_and_the_entry_points_exist():
    from burst_amd import capi, host
    assert capi.lib().bhip_abi_version() == 8
    assert {"bhip_site_counts", "bhip_site_counts_info"} <= set(capi.EXPORTS)
    assert hasattr(capi.lib(), "bhip_site_counts") and hasattr(capi.lib(), "bhip_site_counts_info")
    assert hasattr(capi.Device, "site_counts") and hasattr(capi.Device, "site_counts_info")
    for s in ("bh_vcfstudy_open", "bh_vcfstudy_set_solver", "bh_vcfstudy_check_names", "bh_vcfstudy_add", "bh_vcfstudy_sample_failed", "bh_vcfstudy_abort", "bh_vcfstudy_write",
              "bh_vcfstudy_print_info", "bh_vcfstudy_last_info", "bh_vcfstudy_close", "bh_site_counts_host", "bh_vcf_set_study", "bh_vcf_study_sample_failed"):
        assert hasattr(host.lib(), s), s
    assert (capi.COUNT_RANGE_DTYPE.itemsize, capi.COUNT_RECORD_DTYPE.itemsize, capi.COUNT_CELL_DTYPE.itemsize) == (16, 24, 24)


# ---- the collector and the writer --------------------------------------------------------------------------------------------------------
def group(st, pool, idx, rng, exact=False, shift=0, dup=3):
    """the cases idx of the pool as one traced group, as test_vcf_cpu.pool_group makes it: per record one to `dup` printed lines.  exact: every
    read is replaced by the reference window its path covers, so the sample lies on the same positions and shows the reference everywhere;
    shift: the lanes lie that far to the right on their headers.  Returns the query list the group's records index"""
    queries, records, notes = list(pool.queries), [], []
    for k, i in enumerate(idx):
        c = pool.cases[i]
        q, words = c["q"], c["ops"]
        if exact:
            span = pilecases.span_of(c["ops"])
            queries.append(np.asarray(pool.seqs[c["refIx"]][c["ref_first"] - 1:c["ref_first"] - 1 + span], np.uint8))
            q, words = len(queries) - 1, [span << 4 | 7]
        records.append((q, c["refIx"], c["ref_first"], words))
        for _ in range(int(rng.integers(1, dup + 1))):
            notes.append((k, 6000 * c["refIx"] + 3 + shift, c["refIx"] % len(tv.HEADS), int(rng.integers(0, 2))))
    st.group(records, notes, queries, lambda refIx: pool.seqs[refIx])
    return queries


def q_arrays(queries):
    off = np.zeros(len(queries) + 1, np.uint64)
    off[1:] = np.cumsum([len(q) for q in queries])
    return np.concatenate(queries).astype(np.uint8), off


class StudyFile:
    """a test_vcf_cpu.Study with a bh_vcfstudy.c object attached (or not), and the three samples of these tests"""
    def __init__(self, pool, tmp_path, attach=True, solver="host", md=2, ma=2):
        from burst_amd import host
        self.host, self.pool, self.dir, self.md, self.ma = host, pool, tmp_path, md, ma
        self.st = tv.Study(pool.refs, md, ma)
        assert self.st.rc == 0
        self.prefix = str(tmp_path / "S_")
        self.h = C.c_void_p()
        if attach:
            assert host.lib().bh_vcfstudy_open(self.prefix.encode(), C.byref(self.h)) == 0
            if solver == "host":
                host.lib().bh_vcfstudy_set_solver(self.h, C.cast(host.lib().bh_site_counts_host, C.c_void_p), None)
            host.lib().bh_vcf_set_study(self.st.h, self.h)
        self.names, self.samples, self.single = [], [], {}

    def sample(self, name, idx, seed, **kw):
        queries = group(self.st, self.pool, idx, np.random.default_rng(seed), **kw)
        lines = list(self.st.model)
        codes, off = q_arrays(queries)
        got, exp, count = self.st.sample(str(self.dir / (name + ".b6")), codes, off)
        assert got == exp      # (thresholds (1, 1) and the filter on the host, or the thresholds themselves: the same bytes)
        self.names.append(name)
        self.samples.append(lines)
        self.single[name] = got
        return count

    def failed(self, name):
        assert self.host.lib().bh_vcf_study_sample_failed(self.st.h, str(self.dir / (name + ".b6")).encode()) == 0
        self.names.append(name)
        self.samples.append(None)

    def three(self):
        kinds = lambda *ks: [i for i, c in enumerate(self.pool.cases) if c["kind"] in ks]
        a = kinds("repeat", "row1", "m100_e7", "m100_e15")
        count = self.sample("edited", a, 11)
        assert count["snv"] >= 1 and count["del"] >= 1 and count["ins"] >= 1, count
        self.sample("plain", a, 12, exact=True)
        self.sample("elsewhere", kinds("m33_e1", "m292_e15"), 13, shift=3000000)
        return count

    def write(self):
        rc = self.host.lib().bh_vcfstudy_write(self.h, self.st.h, None)
        return rc, (open(self.prefix + "study.vcf", "rb").read() if not rc else None)

    def info(self):
        info = np.zeros(8, np.uint64)
        self.host.lib().bh_vcfstudy_last_info(self.h, info.ctypes.data)
        return dict(zip(self.host.VCF_STUDY_INFO, (int(x) for x in info)))

    def close(self):
        self.host.lib().bh_vcfstudy_close(self.h)
        self.st.close()


def body(vcf_bytes):
    return [ln for ln in vcf_bytes.decode().split("\n") if ln and not ln.startswith("#")]


def test_file_bytes_single_files_unchanged_and_projections(pool, tmp_path):
    sf = StudyFile(pool, tmp_path)
    count = sf.three()
    assert tv.files_of(tmp_path) == ["edited.b6.vcf", "elsewhere.b6.vcf", "plain.b6.vcf"]      # (no study file, no temporary file before the write)
    rc, got = sf.write()
    assert rc == 0, sf.host.lib().bh_last_error()
    exp, n = vcfstudylib.render(CONTIGS, sf.names, sf.samples, sf.md, sf.ma)
    assert got == exp
    info = sf.info()
    assert (info["samples"], info["failed"], info["snv"], info["del"], info["ins"]) == (3, 0, n["snv"], n["del"], n["ins"])
    assert info["cells"] == 3 * sum(n.values()) and info["host_bytes"] > 16 * sum(len(s) for s in sf.samples)
    assert n["snv"] >= count["snv"] and n["del"] >= count["del"] and n["ins"] >= count["ins"]
    text = got.decode().split("\n")
    assert text[7] == '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads observing the position">' and text[8] == vcfstudylib.NS_LINE[:-1]
    assert text[11] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tedited\tplain\telsewhere"
    # every sample's own file is what the same object writes without the study ...
    other = tmp_path / "without"
    other.mkdir()
    plain = StudyFile(pool, other, attach=False)
    plain.three()
    plain.close()
    assert all(plain.single[k] == sf.single[k] for k in sf.names) and tv.files_of(other) == ["edited.b6.vcf", "elsewhere.b6.vcf", "plain.b6.vcf"]
    # ... and the projection of the study file onto the records that sample reports
    for k, name in enumerate(sf.names):
        assert vcfstudylib.project(got, k, sf.md, sf.ma) == body(sf.single[name]), name
    # where the edited sample reports, the unedited one has its reads on the reference and the one elsewhere has none
    mine = set(ln.split("\t")[0] + ":" + ln.split("\t")[1] for ln in body(sf.single["edited"]))
    rows = [ln.split("\t") for ln in body(got) if ln.split("\t")[0] + ":" + ln.split("\t")[1] in mine]
    assert len(rows) >= 3
    for r in rows:
        dp, ad = r[10].split(":")
        assert int(dp) > 0 and ad.split(",")[0] == dp and set(ad.split(",")[1:]) == {"0"} and r[11].split(":")[0] == "0" and set(r[11].split(":")[1].split(",")) == {"0"}
    sf.close()
    assert tv.files_of(tmp_path) == ["S_study.vcf", "edited.b6.vcf", "elsewhere.b6.vcf", "plain.b6.vcf", "without"]


def test_a_failed_sample_has_a_dot_in_its_column(pool, tmp_path):
    sf = StudyFile(pool, tmp_path)
    kinds = lambda *ks: [i for i, c in enumerate(pool.cases) if c["kind"] in ks]
    sf.sample("first", kinds("repeat", "row1"), 21)
    sf.failed("broken")
    sf.sample("third", kinds("row1", "m100_e7"), 22)
    rc, got = sf.write()
    assert rc == 0
    exp, n = vcfstudylib.render(CONTIGS, sf.names, sf.samples, sf.md, sf.ma)
    assert got == exp and sum(n.values()) >= 3
    assert all(ln.split("\t")[10] == "." for ln in body(got)) and sf.info()["failed"] == 1 and sf.info()["cells"] == 2 * sum(n.values())
    assert sf.host.lib().bh_vcfstudy_write(sf.h, sf.st.h, None) != 0      # written once
    sf.close()
    assert tv.files_of(tmp_path) == ["S_study.vcf", "first.b6.vcf", "third.b6.vcf"]


def test_a_solver_error_leaves_no_file_and_no_temporary_file(pool, tmp_path):
    sf = StudyFile(pool, tmp_path, solver="device")      # the device, and there is no handle
    sf.three()
    rc, _ = sf.write()
    assert rc != 0 and b"no device handle" in sf.host.lib().bh_last_error()
    assert sf.host.lib().bh_vcfstudy_write(sf.h, sf.st.h, None) != 0      # final
    sf.close()
    assert tv.files_of(tmp_path) == ["edited.b6.vcf", "elsewhere.b6.vcf", "plain.b6.vcf"]
    # a list that comes back inconsistent is an internal error, and no file either
    def depth_zero_counts_one(ctx, r, nr, s, ns, a, na, q, nq, cells, info):
        words = (C.c_uint32 * (6 * nq)).from_address(cells)
        for k in range(6 * nq):
            words[k] = 0 if k % 6 == 0 else 1
        return 0
    bad = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)(depth_zero_counts_one)
    work = tmp_path / "w"
    work.mkdir()
    sf = StudyFile(pool, work)
    sf.host.lib().bh_vcfstudy_set_solver(sf.h, C.cast(bad, C.c_void_p), None)
    sf.sample("s", [i for i, c in enumerate(pool.cases) if c["kind"] == "m100_e15"], 3, dup=4)
    rc, _ = sf.write()
    assert rc == sf.host.E_INTERNAL and b"more reads" in sf.host.lib().bh_last_error()
    sf.close()
    assert tv.files_of(work) == ["s.b6.vcf"]


def test_two_samples_of_one_name_are_refused_and_both_are_named(pool, tmp_path):
    from burst_amd import host
    paths = [b"runs/a/reads.b6", b"other.b6", b"runs/b/reads.txt"]
    assert host.lib().bh_vcfstudy_check_names((C.c_char_p * 3)(*paths), 3) == host.E_USAGE
    msg = host.lib().bh_last_error().decode()
    assert "--vcf-study" in msg and "'runs/a/reads.b6'" in msg and "'runs/b/reads.txt'" in msg and "'reads'" in msg
    assert host.lib().bh_vcfstudy_check_names((C.c_char_p * 2)(*paths[:2]), 2) == 0
    # the collector refuses the second one too, and the first sample's column stays
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    sf = StudyFile(pool, tmp_path)
    idx = [i for i, c in enumerate(pool.cases) if c["kind"] == "row1"]
    sf.sample("a/reads", idx, 1)
    group(sf.st, pool, idx, np.random.default_rng(2))
    codes, off = q_arrays(list(pool.queries))
    rc = host.lib().bh_vcf_sample(sf.st.h, None, str(tmp_path / "b" / "reads.b6").encode(), codes.ctypes.data, off.ctypes.data, len(off) - 1)
    assert rc == host.E_USAGE and "a/reads.b6" in host.lib().bh_last_error().decode() and "b/reads.b6" in host.lib().bh_last_error().decode()
    sf.names = ["reads"]
    rc, got = sf.write()
    assert rc == 0 and got == vcfstudylib.render(CONTIGS, sf.names, sf.samples, sf.md, sf.ma)[0]
    sf.close()


# ---- the command line refuses before a device is touched --------------------------------------------------------------------------------
QO = ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", "out.b6"]


def test_the_flag_goes_with_vcf(tmp_path):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--vcf-study", "P_"] + QO, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "ERROR: --vcf-study goes with --vcf" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "--vcf", "--vcf-study"] + QO, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "--vcf-study requires an argument" in r.stdout, r.stdout + r.stderr
    assert tv.files_of(tmp_path) == []


@pytest.mark.parametrize("extra,word", [
    (QO + ["-x"], "-x"), (QO + ["-d"], "-d"), (QO + ["--make-acx", "x.acx"], "--make-acx"),
    (QO + ["--gpus", "2", "--shard", "db"], "--shard db"), (QO + ["--shards", "2"], "--shards"), (QO + ["--gpus", "2", "--gather", "rccl"], "rccl"),
    (QO + ["--mates", os.path.join(GOLDEN, "q100.fa")], "--mates"),
    (QO + ["-m", "FORAGE", "--cluster", "C"], "--cluster"), (QO + ["-m", "FORAGE", "--chimeras", "C"], "--chimeras"),
])
def test_everything_that_refuses_vcf_refuses_the_study(tmp_path, extra, word):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--vcf", "--vcf-study", "P_"] + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "ERROR: --vcf" in r.stdout and word in r.stdout, r.stdout + r.stderr
    assert tv.files_of(tmp_path) == []


def test_two_outputs_of_one_name_in_a_sample_list(tmp_path):
    lst = tmp_path / "list.txt"
    q = os.path.join(GOLDEN, "q100.fa")
    lst.write_text("%s\t%s\n%s\t%s\n" % (q, tmp_path / "a" / "x.b6", q, tmp_path / "b" / "x.tsv"))
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--vcf", "--vcf-study", str(tmp_path / "P_"), "--samples", str(lst)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: --vcf-study" in r.stdout and "a/x.b6" in r.stdout and "b/x.tsv" in r.stdout and "'x'" in r.stdout, r.stdout + r.stderr
    assert "Parsing" not in r.stdout      # (before the database is read, let alone a device touched)
    assert tv.files_of(tmp_path) == ["list.txt"]


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--vcf-study", "P_"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--vcf is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flag():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--vcf-study <prefix>" in r.stdout and "study.vcf" in r.stdout


def test_python_session_wants_vcf_with_the_study():
    from burst_amd import host
    with pytest.raises(ValueError, match="vcf_study goes with vcf"):
        host.Session(None, None, vcf_study="P_")


def test_host_files_under_the_sanitizers(tmp_path):
    """csrc/host/bh_vcfstudy.c and bh_vcf.c as a stand-alone program (tests/csrc/vcfstudy_host_main.c) with ASan and UBSan linked in: the
    yardstick, the collector, the writer, the life cycle"""
    exe = str(tmp_path / "vcfstudy_host_main")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "vcfstudy_host_main.c")] +
                          [os.path.join(CSRC, "host", f) for f in ("bh_vcfstudy.c", "bh_vcf.c", "bh_pile.c", "bh_sam.c", "bh_tables.c")] + ["-o", exe])
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "vcfstudy_host_main ok" in r.stdout, r.stdout + r.stderr
    assert "VcfStudy: 2 samples done, 1 failed" in r.stdout
    assert tv.files_of(work) == []
