"""VCF output without a device: bh_alleles_host (the allele definition in plain sequential C) against vcflib (the dictionary count) on the
inputs of the kernel test and on lines written by hand for every rule; the collector and the writer of bh_vcf.c through their C entry
points with bh_pile_host and bh_alleles_host as the solvers -- the file's bytes, the header block, the clash of two names, a failed
sample, no temporary file left behind; and every refusal of the command line, which comes before a device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarlib as cg
import pilecases
import pilelib
import vcfcases
import vcflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


class Pool(pilecases.PileCases):
    def __init__(self, L, z=1, iupac_only=False):
        from burst_amd import host
        super().__init__(L, z, iupac_only)
        self.refs = host.pile_refs(self.packed, self.clump_len, self.tot)

    def check(self, idx, min_depth=1, min_alt=1, weights=None):
        from burst_amd import host
        lines, ops = self.arrays(idx, weights)
        got, codes, info = host.alleles_host(self.refs, self.q_codes, self.q_off, lines, ops, min_depth, min_alt)
        rows, fig = vcfcases.expect(self.model_lines(idx, weights), min_depth, min_alt)
        vcfcases.same(got, codes, rows)
        vcfcases.info_matches(info, fig, len(rows))
        return rows, fig


@pytest.fixture(scope="module")
def pool(L):
    return Pool(L, 1)


def run_hand(pool, h, min_depth=1, min_alt=1):
    from burst_amd import host
    codes, off = h.q_arrays()
    got, dcodes, info = host.alleles_host(pool.refs, codes, off, h.rows, h.ops, min_depth, min_alt)
    rows, fig = vcfcases.expect(h.model, min_depth, min_alt)
    vcfcases.same(got, dcodes, rows)
    vcfcases.info_matches(info, fig, len(rows))
    return rows, fig


# ---- bh_alleles_host = the model -----------------------------------------------------------------------------------------------------------
def test_whole_pool_then_every_kind(pool):
    assert pool.shared is not None and pool.shared[3] >= 1
    idx = list(range(len(pool.cases)))
    rows, fig = pool.check(idx)
    # what the pool has to yield: a Del, an Ins, a skipped end run, and an allele on the header two lanes share
    assert any(r[5] == vcflib.DEL for r in rows) and any(r[5] == vcflib.INS for r in rows) and fig["end"] >= 1
    assert any(r[0] == pool.header[pool.shared[0]] for r in rows)
    assert len(rows) > 200 and max(r[6] for r in rows if r[5] == vcflib.DEL) >= 2 and max(r[6] for r in rows if r[5] == vcflib.INS) >= 2
    for kd in sorted(set(c["kind"] for c in pool.cases)):
        pool.check([i for i in idx if pool.cases[i]["kind"] == kd])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_line_counts(pool, n):
    rng = np.random.default_rng(n)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=n)]
    pool.check(idx, min_depth=1 if n < 5000 else 3, min_alt=1 if n < 5000 else 2)


def test_a_permutation_of_the_lines_changes_nothing(pool):
    from burst_amd import host
    rng = np.random.default_rng(3)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=700)]
    lines, ops = pool.arrays(idx)
    a, ca, _ = host.alleles_host(pool.refs, pool.q_codes, pool.q_off, lines, ops, 2, 1)
    b, cb, _ = host.alleles_host(pool.refs, pool.q_codes, pool.q_off, lines[rng.permutation(len(lines))], ops, 2, 1)
    assert len(a) > 50 and a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()


def test_every_rule_on_lines_written_by_hand(pool):
    for name, h, check in vcfcases.scenarios(pool):
        rows, fig = run_hand(pool, h)
        check(rows, fig)


@pytest.mark.parametrize("min_depth,min_alt", [(4, 2), (10, 3)])
def test_planted_deletion_either_side_of_both_thresholds(pool, min_depth, min_alt):
    for n_lines, k, want in pilecases.planted_cases(min_depth, min_alt):
        rows, _ = run_hand(pool, vcfcases.planted_del(pool, n_lines, k), min_depth, min_alt)
        vcfcases.check_planted_del(rows, n_lines, k, want)


def test_the_yardstick_refuses_what_the_device_refuses(pool):
    from burst_amd import capi, host
    lines, ops = pool.arrays([0, 5, 9])
    for field, value in [("q", len(pool.queries)), ("refIx", pool.tot), ("op_off", len(ops)), ("ref_first", 0), ("pos", 0), ("w", 0)]:
        bad = lines.copy()
        bad[field][2] = value
        with pytest.raises(host.HostError, match="line 2"):
            host.alleles_host(pool.refs, pool.q_codes, pool.q_off, bad, ops, 1, 1)
    for md, ma in [(0, 1), (1, 0), (1 << 31, 1), (1, 1 << 31)]:
        with pytest.raises(host.HostError):
            host.alleles_host(pool.refs, pool.q_codes, pool.q_off, lines, ops, md, ma)
    # room for one allele fewer, then for one code fewer, than there are: the numbers wanted come back
    idx = list(range(0, len(pool.cases), 2))
    lines, ops = pool.arrays(idx)
    rows, _ = vcfcases.expect(pool.model_lines(idx))
    n_codes = sum(len(r[8]) for r in rows)
    assert len(rows) > 1 and n_codes > 1
    for cap, code_cap in [(len(rows) - 1, n_codes), (len(rows), n_codes - 1)]:
        na, nc, out, codes = C.c_uint64(0), C.c_uint64(0), np.zeros(len(rows), capi.ALLELE_DTYPE), np.zeros(n_codes, np.uint8)
        rc = host.lib().bh_alleles_host(C.byref(pool.refs), pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.q_off) - 1, lines.ctypes.data, len(lines),
                                        ops.ctypes.data, len(ops), 1, 1, out.ctypes.data, cap, C.byref(na), codes.ctypes.data, code_cap, C.byref(nc), None)
        assert rc == host.E_CAPACITY and (na.value, nc.value) == (len(rows), n_codes) and not out.tobytes().strip(b"\0") and not codes.any()


def test_the_abi_version_stays_and_the_entry_points_exist():
    from burst_amd import capi, host
    assert capi.lib().bhip_abi_version() == 8
    assert {"bhip_alleles_run", "bhip_alleles_info"} <= set(capi.EXPORTS)
    for s in ("bh_vcf_open", "bh_vcf_open_heads", "bh_vcf_set_solver", "bh_vcf_collect", "bh_vcf_sample", "bh_vcf_sample_failed", "bh_vcf_abort", "bh_vcf_print_info",
              "bh_vcf_last_info", "bh_vcf_close", "bh_alleles_host", "bh_session_set_vcf", "bh_paths_set_vcf"):
        assert hasattr(host.lib(), s), s


# ---- the collector and the writer --------------------------------------------------------------------------------------------------------
HEADS = [b"zeta ref", b"alpha", b"beta\tsecond word", b"Zed", b"mid|7"]      # header numbers 0 .. 4: the file's order, whatever the names
SN = ["zeta", "alpha", "beta", "Zed", "mid|7"]
LENGTHS = [200000, 210000, 220000, 230000, 240000]


class Study:
    """bh_vcf.c driven as the report drives it: groups of traced records with the notes of their printed lines"""
    def __init__(self, refs, min_depth=1, min_alt=1, unique_only=False, heads=HEADS):
        from burst_amd import host
        self.host, self.md, self.ma, self.unique_only = host, min_depth, min_alt, unique_only
        self.h = C.c_void_p()
        arr = (C.c_char_p * len(heads))(*heads)
        lengths = np.array(LENGTHS[:len(heads)], np.uint32)
        self.rc = host.lib().bh_vcf_open_heads(len(heads), arr, lengths.ctypes.data, min_depth, min_alt, int(unique_only), C.byref(self.h))
        if not self.rc:
            ctx = C.cast(C.pointer(refs), C.c_void_p)
            host.lib().bh_vcf_set_solver(self.h, C.cast(host.lib().bh_pile_host, C.c_void_p), ctx, C.cast(host.lib().bh_alleles_host, C.c_void_p), ctx)
        self.model = []

    def group(self, records, notes, queries, ref_of):
        """one traced group.  records: [(query entry, refIx, first lane column, op words)]; notes: per printed line (record number in
        records, refOff, header number, unique); ref_of(refIx) -> the lane's codes"""
        from burst_amd import capi
        host = self.host
        rec = np.arange(10, 10 + len(records), dtype=np.uint64) * 3      # record numbers in the report's array: ascending, not dense
        req = np.zeros(len(records), capi.PATH_REQ_DTYPE)
        first = np.zeros(len(records), np.uint32)
        off = np.zeros(len(records) + 1, np.uint64)
        ops = []
        for k, (q, refIx, ref_first, words) in enumerate(records):
            req[k] = (q, refIx, 0, 0)
            first[k] = ref_first
            ops.append(np.asarray(words, np.uint32))
            off[k + 1] = off[k] + len(words)
        ops = np.concatenate(ops).astype(np.uint32)
        half = len(notes) // 2      # the notes come in two chunks
        bufs, keep = (host.BhPathBuf * 2)(), []
        for b, part in enumerate((notes[:half], notes[half:])):
            a = np.zeros(len(part), host.PATH_LINE_DTYPE)
            for j, (k, ref_off, header, uniq) in enumerate(part):
                a[j] = (rec[k], ref_off, header, uniq)
            keep.append(a)
            bufs[b].l, bufs[b].n, bufs[b].cap = a.ctypes.data, len(a), len(a)
        assert host.lib().bh_vcf_collect(self.h, rec.ctypes.data, req.ctypes.data, first.ctypes.data, off.ctypes.data, ops.ctypes.data, len(records), bufs, 2) == 0
        for k, ref_off, header, uniq in notes:
            if self.unique_only and not uniq:
                continue
            q, refIx, ref_first, words = records[k]
            seq = ref_of(refIx)
            self.model.append(dict(header=header, pos=ref_off + ref_first, w=1, query=queries[q],
                                   ops=[(int(w) >> 4, pilecases.OP_CHAR[int(w) & 15]) for w in words],
                                   ref=lambda p, seq=seq, o=ref_off: int(seq[p - o - 1]) if 0 <= p - o - 1 < len(seq) else 0))

    def sample(self, path, q_codes, q_off):
        """the sample ends: returns (the file's bytes, the model's bytes, the model's record counts)"""
        rc = self.host.lib().bh_vcf_sample(self.h, None, path.encode(), q_codes.ctypes.data, q_off.ctypes.data, len(q_off) - 1)
        assert rc == 0, self.host.lib().bh_last_error()
        exp, count = vcflib.render(list(zip(SN, LENGTHS)), os.path.splitext(os.path.basename(path))[0], self.model, self.md, self.ma)
        self.model = []
        return open(path + ".vcf", "rb").read(), exp, count

    def info(self):
        info = np.zeros(12, np.uint64)
        self.host.lib().bh_vcf_last_info(self.h, info.ctypes.data)
        return dict(zip(self.host.VCF_INFO, (int(x) for x in info)))

    def close(self):
        self.host.lib().bh_vcf_close(self.h)
        self.h = C.c_void_p()


def pool_group(st, pool, idx, rng, dup=3):
    """the cases idx of the pool as one group: per record one to `dup` printed lines in a row (a duplicate read prints its unique query's line
    again), headers and offsets by lane"""
    records = [(pool.cases[i]["q"], pool.cases[i]["refIx"], pool.cases[i]["ref_first"], pool.cases[i]["ops"]) for i in idx]
    notes = []
    for k, i in enumerate(idx):
        lane = pool.cases[i]["refIx"]
        for _ in range(int(rng.integers(1, dup + 1))):
            notes.append((k, 6000 * lane + 3, lane % len(HEADS), int(rng.integers(0, 2))))      # (lanes that share a header do not overlap)
    st.group(records, notes, pool.queries, lambda refIx: pool.seqs[refIx])


def files_of(tmp_path):
    return sorted(os.listdir(str(tmp_path)))


@pytest.mark.parametrize("unique_only", [False, True])
def test_file_bytes_header_block_order_and_a_failed_sample(pool, tmp_path, unique_only):
    rng = np.random.default_rng(7)
    st = Study(pool.refs, 2, 2, unique_only)
    assert st.rc == 0 and files_of(tmp_path) == []
    kinds = lambda *ks: [i for i, c in enumerate(pool.cases) if c["kind"] in ks]
    a, b = kinds("repeat", "row1", "m100_e7", "m100_e15"), kinds("iupac", "first_columns", "last_columns", "m33_e1", "m292_e15", "m292_e30")
    pool_group(st, pool, a[:30], rng)
    pool_group(st, pool, a[30:], rng)
    got, exp, count = st.sample(str(tmp_path / "second_sample.b6"), pool.q_codes, pool.q_off)
    assert got == exp and count["snv"] >= 1 and count["del"] >= 1 and count["ins"] >= 1, count
    info = st.info()
    assert (info["snv"], info["del"], info["ins"]) == (count["snv"], count["del"], count["ins"]) and info["lines"] > 0
    text = got.decode().split("\n")
    assert text[:2] == ["##fileformat=VCFv4.2", "##source=burst_hip"]
    assert text[2:7] == ["##contig=<ID=%s,length=%d>" % c for c in zip(SN, LENGTHS)]      # header-number order, SN up to the first white space
    assert text[10] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsecond_sample"
    body = [ln.split("\t") for ln in text[11:] if ln]
    keys = [(SN.index(r[0]), int(r[1])) for r in body]
    assert keys == sorted(keys) and len(set(k[0] for k in keys)) >= 3      # header-number order (zeta first), then POS
    assert all(r[2] == r[5] == r[6] == "." and r[8] == "DP:AD" and r[7] == "DP=" + r[9].split(":")[0] and set(r[3] + r[4]) <= set("ACGTN,") for r in body)
    # a sample that failed alone: its lines are dropped, it leaves no file, and the next sample does not see them
    pool_group(st, pool, b, rng)
    st.host.lib().bh_vcf_sample_failed(st.h)
    st.model = []
    pool_group(st, pool, b, rng)
    got, exp, count = st.sample(str(tmp_path / "first.sample.b6"), pool.q_codes, pool.q_off)
    assert got == exp and sum(count.values()) >= 3
    st.close()
    assert files_of(tmp_path) == ["first.sample.b6.vcf", "second_sample.b6.vcf"]


def test_hand_made_lines_through_the_writer(pool, tmp_path):
    """every hand-made scenario as a sample of its own: SNV, Del and Ins records at one position, N for a code outside A/C/G/T"""
    st = Study(pool.refs, 1, 1)
    for k, (name, h, check) in enumerate(vcfcases.scenarios(pool)):
        records = [(int(r[0]), int(r[1]), int(r[2]), h.ops[int(r[7]):int(r[7]) + int(r[6])]) for r in h.rows]
        notes = [(i, int(r[4]) - int(r[2]), 2, 1) for i, r in enumerate(h.rows) for _ in range(int(r[5]))]      # a weight w is w printed lines in a row
        st.group(records, notes, h.queries, lambda refIx: pool.seqs[refIx])
        codes, off = h.q_arrays()
        got, exp, count = st.sample(str(tmp_path / ("hand%d.b6" % k)), codes, off)
        assert got == exp, name
        if "prints N" in name:
            line = [ln for ln in got.decode().split("\n") if ln and not ln.startswith("#")][-1].split("\t")
            assert line[4] == line[3] + "NNA"
        if "behind X" in name:
            assert count["snv"] == 1      # the X column is an SNV record and an insertion's anchor at one POS: the SNV first
            pos = [ln.split("\t")[1] for ln in got.decode().split("\n") if ln and not ln.startswith("#")]
            assert pos[0] == pos[1]
    st.close()
    assert all(f.endswith(".b6.vcf") for f in files_of(tmp_path))


def test_two_headers_of_one_name_are_refused_and_name_both(pool):
    st = Study(pool.refs, heads=[b"alpha one", b"beta", b"alpha two"])
    assert st.rc != 0
    msg = st.host.lib().bh_last_error().decode()
    assert "--vcf" in msg and "'alpha one'" in msg and "'alpha two'" in msg and "'alpha'" in msg
    st2 = Study(pool.refs, heads=[b"alpha one", b"alpha one"])      # the same header twice is no clash of two headers
    assert st2.rc == 0
    st2.close()


def test_a_solver_error_is_final_and_leaves_no_file(pool, tmp_path):
    from burst_amd import host
    rng = np.random.default_rng(9)
    st = Study(pool.refs)
    host.lib().bh_vcf_set_solver(st.h, None, None, None, None)      # the device, and there is no handle
    pool_group(st, pool, list(range(20)), rng)
    path = str(tmp_path / "x.b6").encode()
    assert host.lib().bh_vcf_sample(st.h, None, path, pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries)) != 0
    assert b"no device handle" in host.lib().bh_last_error()
    assert host.lib().bh_vcf_sample(st.h, None, path, pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries)) != 0
    st.close()
    assert files_of(tmp_path) == []


# ---- the command line refuses before a device is touched --------------------------------------------------------------------------------
QO = ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", "out.b6"]


@pytest.mark.parametrize("extra,word", [
    (QO + ["-x"], "-x"), (QO + ["-d"], "-d"), (QO + ["--make-acx", "x.acx"], "--make-acx"),
    (QO + ["--gpus", "2", "--shard", "db"], "--shard db"), (QO + ["--shards", "2"], "--shards"), (QO + ["--gpus", "2", "--gather", "rccl"], "rccl"),
    (QO + ["--mates", os.path.join(GOLDEN, "q100.fa")], "--mates"),
    (QO + ["-m", "FORAGE", "--cluster", "C"], "--cluster"), (QO + ["-m", "FORAGE", "--chimeras", "C"], "--chimeras"),
])
def test_what_variants_refuses_and_the_self_alignment_outputs(tmp_path, extra, word):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--vcf"] + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --vcf" in r.stdout and word in r.stdout, r.stdout
    assert files_of(tmp_path) == []


def test_mates_line_in_a_sample_list_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\t%s\n" % (os.path.join(GOLDEN, "q100.fa"), tmp_path / "o.b6", os.path.join(GOLDEN, "q100.fa")))
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "-fr", "--vcf", "--samples", str(lst)], capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: --vcf" in r.stdout and "mates" in r.stdout, r.stdout + r.stderr
    assert files_of(tmp_path) == ["list.txt"]


@pytest.mark.parametrize("extra", [["--vcf-min-depth", "5"], ["--vcf-min-alt", "3"], ["--vcf-reads", "unique"], ["--vcf-lengths", "L.txt"],
                                   ["--vcf", "--vcf-min-depth", "0"], ["--vcf", "--vcf-min-depth", "2147483648"], ["--vcf", "--vcf-min-alt", "0"],
                                   ["--vcf", "--vcf-min-alt", "2147483648"], ["--vcf", "--vcf-reads", "some"]])
def test_sub_options_need_the_flag_and_values_in_range(tmp_path, extra):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx")] + QO + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "ERROR: --vcf" in r.stdout, r.stdout + r.stderr
    assert files_of(tmp_path) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--vcf"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--vcf is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert all(w in r.stdout for w in ("--vcf [", "--vcf-min-depth", "--vcf-min-alt", "--vcf-reads", "--vcf-lengths"))
