"""Variant sites without a device: bh_pile_host (the definition in plain C) against pilelib (the dictionary count) on the inputs of the
kernel test; the collector and the writer of bh_pile.c through their C entry points with bh_pile_host as the solver -- the table's bytes,
the order of its rows and blocks, a failed sample, an aborted run, no temporary file left behind; and every refusal of the command line,
which comes before a device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarlib as cg
import pilecases
import pilelib

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
        got, info = host.pile_host(self.refs, self.q_codes, self.q_off, lines, ops, min_depth, min_alt)
        sites = pilelib.pile(self.model_lines(idx, weights))
        exp = pilelib.reported(sites, min_depth, min_alt)
        assert pilecases.rows_of(got) == exp
        assert (int(info[0]), int(info[1]), int(info[2])) == pilelib.figures(sites) + (len(exp),)
        return exp, sites


@pytest.fixture(scope="module")
def pool(L):
    return Pool(L, 1)


def run_hand(pool, h, min_depth=1, min_alt=1):
    from burst_amd import host
    codes, off = h.q_arrays()
    got, info = host.pile_host(pool.refs, codes, off, h.rows, h.ops, min_depth, min_alt)
    sites = pilelib.pile(h.model)
    exp = pilelib.reported(sites, min_depth, min_alt)
    assert pilecases.rows_of(got) == exp
    assert (int(info[0]), int(info[1]), int(info[2])) == pilelib.figures(sites) + (len(exp),)
    return exp


# ---- bh_pile_host = the model ----------------------------------------------------------------------------------------------------------
def test_whole_pool_then_every_kind(pool):
    assert pool.shared is not None and pool.shared[3] >= 1
    idx = list(range(len(pool.cases)))
    rows, _ = pool.check(idx)
    assert len(rows) > 500 and any(r[10] for r in rows) and any(r[8] for r in rows) and any(r[9] for r in rows)
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
    a, _ = host.pile_host(pool.refs, pool.q_codes, pool.q_off, lines, ops, 2, 1)
    b, _ = host.pile_host(pool.refs, pool.q_codes, pool.q_off, lines[rng.permutation(len(lines))], ops, 2, 1)
    assert len(a) > 50 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("min_depth,min_alt", [(4, 2), (10, 3)])
def test_planted_pile_up_either_side_of_both_thresholds(pool, min_depth, min_alt):
    for n_lines, k, want in pilecases.planted_cases(min_depth, min_alt):
        pilecases.check_planted(run_hand(pool, pilecases.planted(pool, n_lines, k), min_depth, min_alt), n_lines, k, want)


def test_boundaries_and_insertions(pool):
    pilecases.check_boundaries(run_hand(pool, pilecases.boundaries(pool)))
    pilecases.check_insertions(run_hand(pool, pilecases.insertions(pool)))
    idx = [i for i, c in enumerate(pool.cases) if c["kind"] == "leading_I"]
    rows, _ = pool.check(idx, weights=[1] * len(idx))
    assert not pool.before_paths(idx) & {(r[0], r[1]) for r in rows}


@pytest.mark.parametrize("z", [0, 1])
def test_ambiguous_codes_on_both_sides(L, z):
    p = Pool(L, z, iupac_only=True)
    rows, sites = p.check(list(range(len(p.cases))))
    assert any(r[9] for r in rows) and all(1 <= r[2] <= 4 for r in rows)
    assert any(not 1 <= s["ref"] <= 4 and s["events"] for s in sites.values())


def test_the_yardstick_refuses_what_the_device_refuses(pool):
    from burst_amd import host
    lines, ops = pool.arrays([0, 5, 9])
    for field, value in [("q", len(pool.queries)), ("refIx", pool.tot), ("op_off", len(ops)), ("ref_first", 0), ("pos", 0), ("w", 0)]:
        bad = lines.copy()
        bad[field][2] = value
        with pytest.raises(host.HostError, match="line 2"):
            host.pile_host(pool.refs, pool.q_codes, pool.q_off, bad, ops, 1, 1)
    for md, ma in [(0, 1), (1, 0)]:
        with pytest.raises(host.HostError):
            host.pile_host(pool.refs, pool.q_codes, pool.q_off, lines, ops, md, ma)
    # room for one site fewer than there are: the number wanted comes back
    from burst_amd import capi
    exp = pilelib.reported(pilelib.pile(pool.model_lines([0, 5, 9])), 1, 1)
    assert len(exp) > 1
    n, sites = C.c_uint64(0), np.zeros(len(exp), capi.PILE_SITE_DTYPE)
    rc = host.lib().bh_pile_host(C.byref(pool.refs), pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.q_off) - 1, lines.ctypes.data, len(lines),
                                 ops.ctypes.data, len(ops), 1, 1, sites.ctypes.data, len(exp) - 1, C.byref(n), None)
    assert rc == host.E_CAPACITY and n.value == len(exp)


# ---- the collector and the writer --------------------------------------------------------------------------------------------------------
HEADS = [b"zeta ref", b"alpha", b"alpha beta", b"Zed", b"mid|7"]      # header numbers 0 .. 4; strcmp order: Zed, alpha, alpha beta, mid|7, zeta ref


class Study:
    """bh_pile.c driven as the report drives it: groups of traced records with the notes of their printed lines"""
    def __init__(self, pool, prefix, min_depth=1, min_alt=1, unique_only=False):
        from burst_amd import host
        self.pool, self.host, self.prefix, self.md, self.ma, self.unique_only = pool, host, prefix, min_depth, min_alt, unique_only
        self.h = C.c_void_p()
        heads = (C.c_char_p * len(HEADS))(*HEADS)
        assert host.lib().bh_pile_open_heads(prefix.encode(), len(HEADS), heads, min_depth, min_alt, int(unique_only), C.byref(self.h)) == 0
        host.lib().bh_pile_set_solver(self.h, C.cast(host.lib().bh_pile_host, C.c_void_p), C.cast(C.pointer(pool.refs), C.c_void_p))
        self.blocks, self.model = [], []

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
        assert host.lib().bh_pile_collect(self.h, rec.ctypes.data, req.ctypes.data, first.ctypes.data, off.ctypes.data, ops.ctypes.data, len(idx), bufs, 2) == 0
        for k, ref_off, header, uniq in notes:
            if self.unique_only and not uniq:
                continue
            c = cases[idx[k]]
            seq = self.pool.seqs[c["refIx"]]
            self.model.append(dict(header=HEADS[header].decode(), pos=ref_off + c["ref_first"], w=1, query=self.pool.queries[c["q"]],
                                   ops=[(int(w) >> 4, pilecases.OP_CHAR[int(w) & 15]) for w in c["ops"]],
                                   ref=lambda p, seq=seq, o=ref_off: int(seq[p - o - 1]) if 0 <= p - o - 1 < len(seq) else 0))

    def sample(self, path):
        rc = self.host.lib().bh_pile_sample(self.h, None, path.encode(), self.pool.q_codes.ctypes.data, self.pool.q_off.ctypes.data, len(self.pool.queries))
        assert rc == 0, self.host.lib().bh_last_error()
        name = os.path.splitext(os.path.basename(path))[0]
        self.blocks.append((name, pilelib.reported(pilelib.pile(self.model), self.md, self.ma)))
        self.model = []

    def failed(self, path):
        assert self.host.lib().bh_pile_sample_failed(self.h, path.encode()) == 0
        self.model = []

    def rows(self):
        from burst_amd import capi
        n = self.host.lib().bh_pile_rows(self.h, None, None, 0)
        rows, samples = np.zeros(max(n, 1), capi.PILE_SITE_DTYPE), np.zeros(max(n, 1), np.uint32)
        self.host.lib().bh_pile_rows(self.h, rows.ctypes.data, samples.ctypes.data, n)
        return rows[:n], samples[:n]

    def close(self):
        self.host.lib().bh_pile_close(self.h)
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


@pytest.mark.parametrize("unique_only", [False, True])
def test_table_bytes_row_order_blocks_and_a_failed_sample(pool, tmp_path, unique_only):
    rng = np.random.default_rng(7)
    prefix = str(tmp_path / "P_")
    st = Study(pool, prefix, 2, 1, unique_only)
    assert files_of(tmp_path) and all(f.startswith("P_variants.txt.tmp") for f in files_of(tmp_path))      # the table grows under a temporary name
    kinds = lambda *ks: [i for i, c in enumerate(pool.cases) if c["kind"] in ks]
    a, b = kinds("repeat", "row1"), kinds("iupac", "first_columns", "last_columns", "m33_e1", "m100_e7")
    st.group(a[:40], notes_for(pool, a[:40], rng))
    st.group(a[40:], notes_for(pool, a[40:], rng))
    st.sample("/somewhere/second_sample.b6")      # (study order, not name order)
    st.group(b, notes_for(pool, b, rng))
    st.failed("/somewhere/broken.b6")             # its lines are dropped, it has no rows
    st.group(b, notes_for(pool, b, rng))
    st.sample("first.sample.b6")
    rows, samples = st.rows()
    assert len(rows) == sum(len(r) for _, r in st.blocks) and sorted(set(samples.tolist())) == [0, 2]
    assert st.host.lib().bh_pile_write(st.h) == 0
    st.close()
    assert files_of(tmp_path) == ["P_variants.txt"]
    got = open(prefix + "variants.txt", "rb").read()
    assert [n for n, _ in st.blocks] == ["second_sample", "first.sample"] and all(len(r) > 20 for _, r in st.blocks)
    assert got == pilelib.table(st.blocks)
    # inside a block: strcmp order of the whole header, then ascending position
    body = [ln.split("\t") for ln in got.decode().split("\n")[1:] if ln]
    for name, _ in st.blocks:
        keys = [(r[0].encode(), int(r[1])) for r in body if r[3] == name]
        assert keys == sorted(keys) and len(set(k[0] for k in keys)) >= 3
    assert [r[3] for r in body] == ["second_sample"] * len(st.blocks[0][1]) + ["first.sample"] * len(st.blocks[1][1])


def test_no_file_after_an_abort_and_none_without_a_write(pool, tmp_path):
    rng = np.random.default_rng(8)
    idx = list(range(0, 60))
    st = Study(pool, str(tmp_path / "A_"))
    st.group(idx, notes_for(pool, idx, rng))
    st.sample("one.b6")
    st.host.lib().bh_pile_abort(st.h)
    assert st.host.lib().bh_pile_write(st.h) != 0
    assert st.host.lib().bh_pile_sample(st.h, None, b"two.b6", pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries)) != 0
    st.close()
    assert files_of(tmp_path) == []
    st = Study(pool, str(tmp_path / "B_"))      # closed without a write: the run ended elsewhere
    st.group(idx, notes_for(pool, idx, rng))
    st.close()
    assert files_of(tmp_path) == []


def test_a_solver_error_is_final(pool, tmp_path):
    from burst_amd import host
    st = Study(pool, str(tmp_path / "E_"))
    host.lib().bh_pile_set_solver(st.h, None, None)      # the device, and there is no handle
    st.group([0, 1], [(0, 0, 0, 1), (1, 0, 1, 1)])
    assert host.lib().bh_pile_sample(st.h, None, b"x.b6", pool.q_codes.ctypes.data, pool.q_off.ctypes.data, len(pool.queries)) != 0
    assert b"no device handle" in host.lib().bh_last_error()
    assert host.lib().bh_pile_write(st.h) != 0
    st.close()
    assert files_of(tmp_path) == []


def test_session_options_are_checked():
    from burst_amd import host
    assert ("pile", C.c_void_p) == host.BhSessionOpts._fields_[-1]      # appended at the end of BhSessionOpts
    for s in ("bh_pile_open", "bh_pile_sample", "bh_pile_sample_failed", "bh_pile_abort", "bh_pile_write", "bh_pile_print_info", "bh_pile_close", "bh_pile_set_solver",
              "bh_pile_host", "bh_session_set_variants", "bh_paths_set_pile"):
        assert hasattr(host.lib(), s), s


# ---- the command line refuses before a device is touched --------------------------------------------------------------------------------
QO = ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", "out.b6"]


@pytest.mark.parametrize("extra,word", [
    (QO + ["-x"], "-x"), (QO + ["-d"], "-d"), (QO + ["--make-acx", "x.acx"], "--make-acx"),
    (QO + ["--gpus", "2", "--shard", "db"], "--shard db"), (QO + ["--shards", "2"], "--shards"), (QO + ["--gpus", "2", "--gather", "rccl"], "rccl"),
    (QO + ["--mates", os.path.join(GOLDEN, "q100.fa")], "--mates"),
])
def test_what_cigar_refuses_and_mates(tmp_path, extra, word):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--variants", "P"] + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "ERROR: --variants" in r.stdout and word in r.stdout, r.stdout
    assert files_of(tmp_path) == []


def test_mates_line_in_a_sample_list_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("%s\t%s\t%s\n" % (os.path.join(GOLDEN, "q100.fa"), tmp_path / "o.b6", os.path.join(GOLDEN, "q100.fa")))
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "-fr", "--variants", str(tmp_path / "P"), "--samples", str(lst)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: --variants" in r.stdout and "mates" in r.stdout, r.stdout + r.stderr
    assert files_of(tmp_path) == ["list.txt"]


@pytest.mark.parametrize("extra", [["--variants-min-depth", "5"], ["--variants-min-alt", "3"], ["--variants-reads", "unique"],
                                   ["--variants", "P", "--variants-min-depth", "0"], ["--variants", "P", "--variants-min-alt", "2147483648"],
                                   ["--variants", "P", "--variants-reads", "some"]])
def test_sub_options_need_the_flag_and_values_in_range(tmp_path, extra):
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx")] + QO + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "--variants" in r.stdout, r.stdout + r.stderr
    assert files_of(tmp_path) == []


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--variants", "P"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--variants is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--variants <prefix>" in r.stdout and "--variants-min-depth" in r.stdout and "--variants-min-alt" in r.stdout and "--variants-reads" in r.stdout
