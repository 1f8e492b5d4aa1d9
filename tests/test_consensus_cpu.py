"""The consensus without a device: bh_consensus_host (the definition in plain C) against conslib (the dictionary model) on the inputs of
the kernel test -- segments, letters and figures byte for byte; the hand-made segment shapes and calling rules; the collector and the
writer of bh_consensus.c through their C entry points with bh_consensus_host as the solver -- both files' bytes, the order of blocks and
headers, a failed sample, an abort, lengths that are too short, no temporary file left behind; the same file as a stand-alone program
under the sanitizers; and every refusal of the command line, which comes before a device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarlib as cg
import conscases
import conslib
import pilecases
import pilelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")
E_USAGE = -1


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


class Pool(pilecases.PileCases):
    def __init__(self, L, z=1, iupac_only=False):
        from burst_amd import host
        super().__init__(L, z, iupac_only)
        self.refs = host.pile_refs(self.packed, self.clump_len, self.tot)

    def check(self, idx, min_depth=1, weights=None):
        from burst_amd import host
        lines, ops = self.arrays(idx, weights)
        segs, letters, info = host.consensus_host(self.refs, self.q_codes, self.q_off, lines, ops, min_depth)
        model = self.model_lines(idx, weights)
        sites = pilelib.pile(model)
        exp_segs, exp_letters = conslib.consensus(model, min_depth, sites)
        assert letters == exp_letters.encode()
        assert segs.tobytes() == conslib.seg_bytes(exp_segs)
        assert tuple(int(x) for x in info[:4]) == conslib.info(model, exp_segs, sites)
        return exp_segs, exp_letters


@pytest.fixture(scope="module")
def pool(L):
    return Pool(L, 1)


def run_hand(pool, h, min_depth):
    from burst_amd import host
    codes, off = h.q_arrays()
    segs, letters, info = host.consensus_host(pool.refs, codes, off, h.rows, h.ops, min_depth)
    exp_segs, exp_letters = conslib.consensus(h.model, min_depth)
    assert letters == exp_letters.encode() and segs.tobytes() == conslib.seg_bytes(exp_segs)
    assert tuple(int(x) for x in info[:4]) == conslib.info(h.model, exp_segs)
    return exp_segs, exp_letters


# ---- bh_consensus_host = the model -------------------------------------------------------------------------------------------------------
def test_whole_pool_then_every_kind(pool):
    idx = list(range(len(pool.cases)))
    segs, letters = pool.check(idx)
    assert len(segs) >= 10 and "-" in letters and sum(g["subst"] for g in segs) > 0 and sum(g["ins_major"] for g in segs) > 0
    for kd in sorted(set(c["kind"] for c in pool.cases)):
        pool.check([i for i in idx if pool.cases[i]["kind"] == kd])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_line_counts(pool, n):
    rng = np.random.default_rng(n)
    pool.check([int(i) for i in rng.integers(0, len(pool.cases), size=n)], min_depth=1 if n < 5000 else 3)


@pytest.mark.parametrize("min_depth", [1, 2, 1000])
def test_min_depth(pool, min_depth):
    segs, letters = pool.check(list(range(0, len(pool.cases), 3)), min_depth)
    if min_depth == 1000:
        assert set(letters) == {"N"} and not any(g["called"] for g in segs)
    else:
        assert any(g["called"] for g in segs)


def test_a_permutation_of_the_lines_changes_nothing(pool):
    from burst_amd import host
    rng = np.random.default_rng(3)
    idx = [int(i) for i in rng.integers(0, len(pool.cases), size=700)]
    lines, ops = pool.arrays(idx)
    a = host.consensus_host(pool.refs, pool.q_codes, pool.q_off, lines, ops, 2)
    b = host.consensus_host(pool.refs, pool.q_codes, pool.q_off, lines[rng.permutation(len(lines))], ops, 2)
    assert len(a[0]) > 5 and a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("shape", conscases.SHAPES, ids=lambda f: f.__name__)
def test_segment_shapes(pool, shape):
    h, check = shape(pool)
    for m in (1, 2):
        segs, letters = run_hand(pool, h, m)
        assert check(segs, letters)


@pytest.mark.parametrize("rule", conscases.RULES, ids=lambda f: f.__name__)
def test_calling_rules(pool, rule):
    h, check = rule(pool)
    segs, letters = run_hand(pool, h, conscases.MIN_DEPTH)
    assert check(segs, letters)


@pytest.mark.parametrize("z", [0, 1])
def test_an_ambiguous_reference_column_keeps_its_letter(L, z):
    p = Pool(L, z, iupac_only=True)
    idx = list(range(len(p.cases)))
    segs, letters = p.check(idx)
    assert sum(g["ambig"] for g in segs) > 0 and set(letters) - set("ACGTN-"), "no ambiguity code among the letters"


def test_capacity_and_arguments(pool):
    from burst_amd import capi, host
    idx = list(range(0, len(pool.cases), 2))
    lines, ops = pool.arrays(idx)
    exp_segs, exp_letters = conslib.consensus(pool.model_lines(idx), 1)
    ns, nl, info = C.c_uint64(0), C.c_uint64(0), np.zeros(8, np.uint64)

    def call(seg_cap, letter_cap, ln=lines, min_depth=1):
        segs, letters = np.zeros(max(seg_cap, 1), capi.CONS_SEG_DTYPE), np.full(max(letter_cap, 1), 0xAB, np.uint8)
        rc = host.lib().bh_consensus_host(C.byref(pool.refs), pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries), ln.ctypes.data, len(ln), ops.ctypes.data, len(ops),
                                          min_depth, segs.ctypes.data, seg_cap, C.byref(ns), letters.ctypes.data, letter_cap, C.byref(nl), info.ctypes.data)
        return rc, segs, letters
    rc, _, letters = call(len(exp_segs) - 1, len(exp_letters))
    assert rc == host.E_CAPACITY and (ns.value, nl.value) == (len(exp_segs), len(exp_letters)) and set(letters.tolist()) == {0xAB}
    rc, _, letters = call(len(exp_segs), len(exp_letters) - 1)
    assert rc == host.E_CAPACITY and (ns.value, nl.value) == (len(exp_segs), len(exp_letters)) and set(letters.tolist()) == {0xAB}
    rc, segs, letters = call(len(exp_segs), len(exp_letters))
    assert rc == 0 and segs.tobytes() == conslib.seg_bytes(exp_segs) and letters.tobytes() == exp_letters.encode()
    for field, value, word in (("q", len(pool.queries), "names query"), ("refIx", pool.tot, "names reference"), ("op_off", len(ops), "owns ops"),
                               ("ref_first", 0, "leave a clump"), ("pos", 0, "position"), ("pos", 0xFFFFFFFF, "position"), ("w", 0, "weight 0")):
        ln = lines.copy()
        ln[field][2] = value
        rc, _, _ = call(len(exp_segs), len(exp_letters), ln)
        assert rc == E_USAGE and "line 2" in host.lib().bh_last_error().decode() and word in host.lib().bh_last_error().decode(), field
    assert call(len(exp_segs), len(exp_letters), min_depth=0)[0] == E_USAGE and "min_depth" in host.lib().bh_last_error().decode()
    segs, letters, info = host.consensus_host(pool.refs, pool.q_codes, pool.q_off, np.zeros(0, capi.PILE_LINE_DTYPE), np.zeros(0, np.uint32), 1)
    assert len(segs) == 0 and letters == b"" and not info.any()


# ---- the collector and the writer --------------------------------------------------------------------------------------------------------
HEADS = [b"zeta ref", b"alpha", b"alpha beta", b"Zed", b"mid|7"]      # header numbers 0 .. 4; strcmp order: Zed, alpha, alpha beta, mid|7, zeta ref
LENGTH = 4000


class Study:
    """bh_consensus.c driven as the report drives it: groups of traced records with the notes of their printed lines"""
    def __init__(self, pool, prefix, min_depth=1, min_breadth=0, unique_only=False, lengths=None):
        from burst_amd import host
        self.pool, self.host, self.prefix, self.md, self.mb, self.unique_only = pool, host, prefix, min_depth, min_breadth, unique_only
        self.lengths = np.array(lengths if lengths is not None else [LENGTH + k for k in range(len(HEADS))], np.uint32)
        self.h = C.c_void_p()
        heads = (C.c_char_p * len(HEADS))(*HEADS)
        assert host.lib().bh_consensus_open_heads(prefix.encode(), len(HEADS), heads, self.lengths.ctypes.data, min_depth, min_breadth, int(unique_only), C.byref(self.h)) == 0
        host.lib().bh_consensus_set_solver(self.h, C.cast(host.lib().bh_consensus_host, C.c_void_p), C.cast(C.pointer(pool.refs), C.c_void_p))
        self.samples, self.model = [], []

    def group(self, idx, notes):
        """one traced group: the records idx (cases of the pool) and per printed line (record number in idx, refOff, header number, unique)"""
        from burst_amd import capi
        host, cases = self.host, self.pool.cases
        rec = np.arange(10, 10 + len(idx), dtype=np.uint64) * 3      # record numbers in the report's array: ascending, not dense
        req = np.zeros(len(idx), capi.PATH_REQ_DTYPE)
        first = np.zeros(len(idx), np.uint32)
        off = np.zeros(len(idx) + 1, np.uint64)
        ops = []
        for k, i in enumerate(idx):
            c = cases[i]
            req[k] = (c["q"], c["refIx"], c["finalPos"], c["ed"])
            first[k] = c["ref_first"]
            ops.append(c["ops"])
            off[k + 1] = off[k] + len(c["ops"])
        ops = np.concatenate(ops).astype(np.uint32)
        half = len(notes) // 2      # the notes come in two chunks
        bufs, keep = (host.BhPathBuf * 2)(), []
        for b, part in enumerate((notes[:half], notes[half:])):
            a = np.zeros(len(part), host.PATH_LINE_DTYPE)
            for j, (k, ref_off, header, uniq) in enumerate(part):
                a[j] = (rec[k], ref_off, header, uniq)
            keep.append(a)
            bufs[b].l, bufs[b].n, bufs[b].cap = a.ctypes.data, len(a), len(a)
        assert host.lib().bh_consensus_collect(self.h, rec.ctypes.data, req.ctypes.data, first.ctypes.data, off.ctypes.data, ops.ctypes.data, len(idx), bufs, 2) == 0
        for k, ref_off, header, uniq in notes:
            if self.unique_only and not uniq:
                continue
            c = cases[idx[k]]
            seq = self.pool.seqs[c["refIx"]]
            self.model.append(dict(header=HEADS[header].decode(), pos=ref_off + c["ref_first"], w=1, query=self.pool.queries[c["q"]],
                                   ops=[(int(w) >> 4, pilecases.OP_CHAR[int(w) & 15]) for w in c["ops"]],
                                   ref=lambda p, seq=seq, o=ref_off: int(seq[p - o - 1]) if 0 <= p - o - 1 < len(seq) else 0))

    def sample(self, path, want=0):
        rc = self.host.lib().bh_consensus_sample(self.h, None, path.encode(), self.pool.q_codes.ctypes.data, self.pool.q_off.ctypes.data, len(self.pool.queries))
        assert rc == want, self.host.lib().bh_last_error()
        self.samples.append((os.path.splitext(os.path.basename(path))[0], self.model))
        self.model = []

    def failed(self, path):
        assert self.host.lib().bh_consensus_sample_failed(self.h, path.encode()) == 0
        self.samples.append((os.path.splitext(os.path.basename(path))[0], None))
        self.model = []

    def expected(self):
        return conslib.files(self.samples, {h.decode(): int(n) for h, n in zip(HEADS, self.lengths)}, self.md, self.mb)

    def rows(self):
        n = self.host.lib().bh_consensus_rows(self.h, None, 0)
        rows = np.zeros(max(n, 1), self.host.CONS_ROW_DTYPE)
        self.host.lib().bh_consensus_rows(self.h, rows.ctypes.data, n)
        return rows[:n]

    def close(self):
        self.host.lib().bh_consensus_close(self.h)
        self.h = C.c_void_p()


def notes_for(pool, idx, rng, dup=3):
    """per record one to `dup` printed lines in a row (a duplicate read prints its unique query's line again), headers and offsets by lane"""
    notes = []
    for k, i in enumerate(idx):
        lane = pool.cases[i]["refIx"]
        for _ in range(int(rng.integers(1, dup + 1))):
            notes.append((k, 50 * lane + 3, lane % len(HEADS), int(rng.integers(0, 2))))
    return notes


def files_of(tmp_path):
    return sorted(os.listdir(str(tmp_path)))


def feed(pool, st):
    """two samples and a failed one between them"""
    rng = np.random.default_rng(7)
    kinds = lambda *ks: [i for i, c in enumerate(pool.cases) if c["kind"] in ks]
    a, b = kinds("repeat", "row1"), kinds("iupac", "first_columns", "last_columns", "m33_e1", "m100_e7")
    st.group(a[:40], notes_for(pool, a[:40], rng))
    st.group(a[40:], notes_for(pool, a[40:], rng))
    st.sample("/somewhere/second_sample.b6")      # (study order, not name order)
    st.group(b, notes_for(pool, b, rng))
    st.failed("/somewhere/broken.b6")             # its lines are dropped, it has no rows
    st.group(b, notes_for(pool, b, rng))
    st.sample("first.sample.b6")


@pytest.mark.parametrize("unique_only,min_breadth", [(False, 0), (True, 0), (False, "mid"), (False, 1000)])
def test_both_files_of_a_study_of_two_samples_and_a_failed_one(pool, tmp_path, unique_only, min_breadth):
    prefix = str(tmp_path / "P_")
    if min_breadth == "mid":      # a cut-off between the breadths the model finds in this study: some records stay, some go
        st = Study(pool, str(tmp_path / "Q_"), 2, 0, unique_only)
        feed(pool, st)
        permille = sorted(1000 * r[4] // r[2] for r in st.expected()[2] if r[4])
        st.close()
        assert permille[0] < permille[-1] and files_of(tmp_path) == []
        min_breadth = permille[len(permille) // 2] + (permille[len(permille) // 2] == permille[0])
    st = Study(pool, prefix, 2, min_breadth, unique_only)
    assert len(files_of(tmp_path)) == 2 and all(".tmp" in f for f in files_of(tmp_path))      # both files grow under temporary names
    feed(pool, st)
    fa, txt, rows = st.expected()
    got_rows = st.rows()
    assert len(got_rows) == len(rows) and sorted(set(got_rows["sample"].tolist())) == [0, 2]
    assert [(HEADS[r["header"]].decode(), int(r["length"]), int(r["covered"]), int(r["called"]), int(r["record"])) for r in got_rows] == [(r[0], r[2], r[3], r[4], r[10]) for r in rows]
    assert st.host.lib().bh_consensus_write(st.h) == 0
    st.close()
    assert files_of(tmp_path) == ["P_consensus.fa", "P_consensus.txt"]
    assert open(prefix + "consensus.txt", "rb").read() == txt
    assert open(prefix + "consensus.fa", "rb").read() == fa
    # blocks in study order, headers in strcmp order inside a block; every record has its header's length
    assert [r[1] for r in rows] == sorted((r[1] for r in rows), key=["second_sample", "first.sample"].index) and len(rows) >= 6
    for name in ("second_sample", "first.sample"):
        heads = [r[0].encode() for r in rows if r[1] == name]
        assert heads == sorted(heads) and len(heads) >= 3
    recs = pilelib.read_fasta(prefix + "consensus.fa")
    assert len(recs) == sum(r[10] for r in rows) and all(len(seq) == dict(zip((h.decode() for h in HEADS), st.lengths))[name.split("|", 1)[1]] for name, seq in recs)
    if min_breadth == 0:
        assert len(recs) == len(rows) and any("-" in seq for _, seq in recs)
    if 0 < min_breadth < 1000:
        assert 0 < len(recs) < len(rows), "the breadth cut-off does not cut between the headers of this study"
    if min_breadth == 1000:
        assert fa == b"" and len(rows) >= 6


def test_a_placement_beyond_the_length_is_a_usage_error_that_names_the_header(pool, tmp_path):
    rng = np.random.default_rng(9)
    idx = [i for i, c in enumerate(pool.cases) if c["refIx"] % len(HEADS) in (1, 2)][:60]      # lines on 'alpha' and on 'alpha beta'
    assert {pool.cases[i]["refIx"] % len(HEADS) for i in idx} == {1, 2}
    st = Study(pool, str(tmp_path / "S_"), lengths=[LENGTH, LENGTH, 40, LENGTH, LENGTH])
    st.group(idx, notes_for(pool, idx, rng))
    st.sample("one.b6", want=E_USAGE)
    err = st.host.lib().bh_last_error().decode()
    assert "'alpha beta'" in err and "--consensus" in err and "40" in err
    assert st.host.lib().bh_consensus_write(st.h) != 0
    st.close()
    assert files_of(tmp_path) == []


def test_no_file_after_an_abort_and_none_without_a_write(pool, tmp_path):
    rng = np.random.default_rng(8)
    idx = list(range(0, 60))
    st = Study(pool, str(tmp_path / "A_"))
    st.group(idx, notes_for(pool, idx, rng))
    st.sample("one.b6")
    st.host.lib().bh_consensus_abort(st.h)
    assert st.host.lib().bh_consensus_write(st.h) != 0
    assert st.host.lib().bh_consensus_sample(st.h, None, b"two.b6", pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries)) != 0
    st.close()
    assert files_of(tmp_path) == []
    st = Study(pool, str(tmp_path / "B_"))      # closed without a write: the run ended elsewhere
    st.group(idx, notes_for(pool, idx, rng))
    st.close()
    assert files_of(tmp_path) == []


def test_a_solver_error_is_final(pool, tmp_path):
    from burst_amd import host
    st = Study(pool, str(tmp_path / "E_"))
    host.lib().bh_consensus_set_solver(st.h, None, None)      # the device, and there is no handle
    st.group([0, 1], [(0, 0, 0, 1), (1, 0, 1, 1)])
    assert host.lib().bh_consensus_sample(st.h, None, b"x.b6", pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries)) != 0
    assert b"no device handle" in host.lib().bh_last_error()
    assert host.lib().bh_consensus_write(st.h) != 0
    st.close()
    assert files_of(tmp_path) == []


def test_host_file_under_the_sanitizers(tmp_path):
    """csrc/host/bh_consensus.c as a stand-alone program with ASan and UBSan linked in: the yardstick on hand-made lines, both capacities, the
    files of a study byte for byte, unique reads, the breadth cut-off, a length that is too short, an abort"""
    exe = str(tmp_path / "consensus_host_main")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "consensus_host_main.c"), os.path.join(CSRC, "host", "bh_consensus.c"), os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "consensus_host_main ok" in r.stdout, r.stdout + r.stderr
    assert "Consensus: 11 lines" in r.stdout and "'gamma'" in r.stdout
    assert files_of(work) == []


def test_the_interface_is_there():
    from burst_amd import capi, host
    assert capi.lib().bhip_abi_version() == 8
    assert capi.CONS_SEG_DTYPE.itemsize == 48 and capi.CONS_SEG_DTYPE == conslib.SEG_DTYPE and host.CONS_ROW_DTYPE.itemsize == 48
    for s in ("bhip_consensus_run", "bhip_consensus_info"):
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s
    for s in ("bh_consensus_open", "bh_consensus_open_heads", "bh_consensus_collect", "bh_consensus_sample", "bh_consensus_sample_failed", "bh_consensus_abort", "bh_consensus_write",
              "bh_consensus_rows", "bh_consensus_print_info", "bh_consensus_last_info", "bh_consensus_close", "bh_consensus_set_solver", "bh_consensus_host",
              "bh_session_set_consensus", "bh_paths_set_consensus"):
        assert hasattr(host.lib(), s), s


# ---- the command line refuses before a device is touched --------------------------------------------------------------------------------
QO = ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", "out.b6"]


@pytest.mark.parametrize("extra,word", [
    (QO + ["-x"], "-x"), (QO + ["-d"], "-d"), (QO + ["--make-acx", "x.acx"], "--make-acx"),
    (QO + ["--gpus", "2", "--shard", "db"], "--shard db"), (QO + ["--shards", "2"], "--shards"), (QO + ["--gpus", "2", "--gather", "rccl"], "rccl"),
    (QO + ["--mates", os.path.join(GOLDEN, "q100.fa")], "--mates"),
    (QO + ["-m", "FORAGE", "--cluster", "C"], "--cluster"), (QO + ["-m", "FORAGE", "--chimeras", "C"], "--chimeras"),
])
def test_what_variants_refuse(tmp_path, extra, word):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--consensus", "P"] + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --consensus" in r.stdout and word in r.stdout, r.stdout
    assert files_of(tmp_path) == []


def test_mates_line_in_a_sample_list_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\t%s\n" % (os.path.join(GOLDEN, "q100.fa"), tmp_path / "o.b6", os.path.join(GOLDEN, "q100.fa")))
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "-fr", "--consensus", str(tmp_path / "P"), "--samples", str(lst)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: --consensus" in r.stdout and "mates" in r.stdout, r.stdout + r.stderr
    assert files_of(tmp_path) == ["list.txt"]


@pytest.mark.parametrize("extra", [["--consensus-min-depth", "5"], ["--consensus-min-breadth", "3"], ["--consensus-reads", "unique"], ["--consensus-lengths", "x.txt"],
                                   ["--consensus", "P", "--consensus-min-depth", "0"], ["--consensus", "P", "--consensus-min-depth", "2147483648"],
                                   ["--consensus", "P", "--consensus-min-breadth", "1001"], ["--consensus", "P", "--consensus-min-breadth", "-1"],
                                   ["--consensus", "P", "--consensus-reads", "some"]])
def test_sub_options_need_the_flag_and_values_in_range(tmp_path, extra):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx")] + QO + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "--consensus" in r.stdout, r.stdout + r.stderr
    assert files_of(tmp_path) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--consensus", "P"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--consensus is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert all(w in r.stdout for w in ("--consensus <prefix>", "--consensus-min-depth", "--consensus-min-breadth", "--consensus-reads", "--consensus-lengths"))
