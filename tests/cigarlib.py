"""Helpers of the --cigar tests: ctypes access to tests/cigar_restate.c (the full-matrix restatement of the canonical alignment path,
compiled by the test that asks first into the directory it hands in), the inputs the CPU and GPU tests share, and a parser of CIGAR
text.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OP_CODE = {"I": 1, "D": 2, "=": 7, "X": 8}
OP_CHAR = {v: k for k, v in OP_CODE.items()}


class CgOut(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("ed", "gapQ", "gapR", "finalPos", "v_final", "n_best_cols", "n_ops", "ref_first", "n_I", "n_D", "n_X", "n_EQ", "n_same_cols")]


_lib = None


def restate(tmpdir):
    """the restatement's library (built once per process)"""
    global _lib
    if _lib is None:
        so = os.path.join(str(tmpdir), "cigar_restate.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-std=gnu11", "-Wall", os.path.join(HERE, "cigar_restate.c"), "-o", so])
        L = C.CDLL(so)
        L.cg_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(CgOut)]
        L.cg_trace.restype = C.c_int
        _lib = L
    return _lib


def trace(L, q, r, bound, lut, final_pos=0):
    """(ok, ops uint32[], CgOut).  final_pos = 0: the end column the re-scorer chooses; else the path must end there scoring `bound`"""
    q = np.ascontiguousarray(q, np.uint8)
    r = np.ascontiguousarray(r, np.uint8)
    lut = np.ascontiguousarray(lut, np.uint8)
    ops = np.zeros(2 * len(q) + 2 * int(bound) + 8, np.uint32)
    out = CgOut()
    rc = L.cg_trace(q.ctypes.data, len(q), r.ctypes.data, len(r), int(bound), lut.ctypes.data, int(final_pos), ops.ctypes.data, len(ops), C.byref(out))
    assert rc >= 0, "ops array too small"
    return bool(rc), ops[:out.n_ops].copy(), out


def parse_cigar(text):
    """[(length, op char)]; raises on anything that is not =XID text"""
    items = re.findall(r"(\d+)([=XID])", text)
    assert "".join(a + b for a, b in items) == text and text, text
    return [(int(a), b) for a, b in items]


def ops_of(text):
    return np.array([n << 4 | OP_CODE[c] for n, c in parse_cigar(text)], np.uint32)


def text_of(ops):
    return "".join("%d%s" % (int(w) >> 4, OP_CHAR[int(w) & 15]) for w in ops)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def edit_read(rng, ref, start, length, n_sub, n_ins, n_del):
    """a read cut from ref[start : start + length] with exactly placed edits (kinds shuffled, positions distinct)"""
    seg = np.array(ref[start:start + length], np.uint8)
    kinds = ["s"] * n_sub + ["i"] * n_ins + ["d"] * n_del
    if not kinds:
        return seg
    pos = np.sort(rng.choice(np.arange(1, max(2, len(seg) - 1)), size=min(len(kinds), max(1, len(seg) - 2)), replace=False))
    order = rng.permutation(len(kinds))
    out, last = [], 0
    for p, k in zip(pos, order):
        out.append(seg[last:p])
        kind = kinds[k]
        if kind == "s":
            b = int(seg[p]) if 1 <= seg[p] <= 4 else 1
            out.append(np.array([b % 4 + 1], np.uint8)); last = p + 1
        elif kind == "d":
            last = p + 1
        else:
            out.append(np.array([rng.integers(1, 5)], np.uint8)); last = p
    out.append(seg[last:])
    return np.concatenate(out).astype(np.uint8)


def random_lane(rng, n, kind="random"):
    if kind == "homopolymer":      # long runs: where a gap goes is decided by the tie-breaks alone
        out = []
        while sum(len(x) for x in out) < n:
            out.append(np.full(int(rng.integers(3, 12)), int(rng.integers(1, 5)), np.uint8))
        return np.concatenate(out)[:n]
    if kind == "tandem":
        unit = rng.integers(1, 5, size=int(rng.integers(2, 5)), dtype=np.uint8)
        return np.tile(unit, n // len(unit) + 1)[:n]
    return rng.integers(1, 5, size=n, dtype=np.uint8)


def build_pool(L, lut, seed=11, iupac_only=False):
    """The lanes, query entries and expected paths the GPU kernel tests share (computed once, on the CPU, by the restatement).
    Returns (seqs, queries, rc flags, cases); a case = dict(q, refIx, finalPos, ed, ops, ref_first, n_I, gapR, n_best_cols, kind, m).
    Lanes 0 .. 15 are one clump, 16 .. 20 a second one with dead lanes behind it (tot_refs = 21)."""
    from burst_amd import synth
    rng = np.random.default_rng(seed)
    seqs = [random_lane(rng, 1600), random_lane(rng, 1490), random_lane(rng, 700, "homopolymer"), random_lane(rng, 700, "tandem")]
    iu = random_lane(rng, 500)
    iu[rng.choice(500, size=40, replace=False)] = rng.integers(5, 16, size=40)
    seqs.append(iu)
    seqs += [random_lane(rng, int(rng.integers(300, 900)), ("random", "homopolymer", "tandem")[k % 3]) for k in range(11)]
    seqs += [random_lane(rng, 420), random_lane(rng, 400, "tandem"), random_lane(rng, 333, "homopolymer"), random_lane(rng, 64), random_lane(rng, 420)]
    clump_len = [max(len(s) for s in seqs[:16]), max(len(s) for s in seqs[16:])]
    queries, rcs, cases = [], [], []

    def add(q, ref, bound, kind, strand=0):
        lane = np.zeros(clump_len[ref >> 4], np.uint8)
        lane[:len(seqs[ref])] = seqs[ref]
        ok, _, o = trace(L, q, lane, bound, lut)
        if not ok:
            return False
        ok, ops, e = trace(L, q, lane, o.ed, lut, final_pos=o.finalPos)
        assert ok
        if strand:      # the read came from the reverse strand: its forward entry and the reverse-complement entry that aligns
            queries.append(synth.revcomp(q)); rcs.append(0)
        queries.append(np.asarray(q, np.uint8)); rcs.append(strand)
        cases.append(dict(q=len(queries) - 1, refIx=ref, finalPos=int(o.finalPos), ed=int(o.ed), ops=ops, ref_first=int(e.ref_first), n_I=int(e.n_I),
                          gapR=int(o.gapR), gapQ=int(o.gapQ), n_best_cols=int(e.n_best_cols), kind=kind, m=len(q)))
        return True

    lens = [2, 31, 32, 33, 64, 65, 100, 292, 1100]
    eds = [0, 1, 7, 8, 15, 16, 30]
    if iupac_only:
        for k in range(40):
            m = int(rng.choice([33, 64, 100, 292]))
            st = int(rng.integers(0, 500 - m))
            q = edit_read(rng, seqs[4], st, m, *(int(x) for x in rng.integers(0, 3, size=3)))
            for p in rng.choice(len(q), size=2, replace=False):
                q[p] = int(rng.integers(5, 16))
            add(q, 4, 12, "iupac")
        return seqs, queries, rcs, cases
    for m in lens:
        for ed in eds:
            if ed > m // 3 and not (m == 2 and ed <= 1):
                continue
            for rep in range(2 if m < 1100 else 1):
                ref = (0, 1, 5, 16, 20)[int(rng.integers(0, 5))] if m <= 300 else int(rng.integers(0, 2))
                n_ref = len(seqs[ref])
                where = rep if m > 2 else 2
                st = 0 if where == 0 else (n_ref - m if where == 1 and ed == 0 else int(rng.integers(0, n_ref - m - ed)))
                if m == 2:
                    q = edit_read(rng, seqs[ref], st, 2, 0, 0, 0)
                    if ed:
                        q[1] = q[1] % 4 + 1
                else:
                    ns = ed - 2 * (ed // 3)
                    q = edit_read(rng, seqs[ref], st, m, ns, ed // 3, ed // 3)
                add(q, ref, ed, "m%d_e%d" % (m, ed), strand=rep)
    # ends of a lane: the first columns, the last columns of the clump's longest lane (an end at ClumpLen), a lane with trailing pads
    for ref in (0, 16, 19, 3):
        n_ref = len(seqs[ref])
        for m in (31, 64):
            if m + 4 > n_ref:
                continue
            add(edit_read(rng, seqs[ref], 0, m, 1, 0, 1), ref, 4, "first_columns")
            add(edit_read(rng, seqs[ref], n_ref - m, m, 1, 1, 0), ref, 4, "last_columns")
            add(np.array(seqs[ref][n_ref - m:], np.uint8), ref, 2, "end_exact")
            add(np.concatenate([[seqs[ref][0] % 4 + 1], seqs[ref][:m - 1]]).astype(np.uint8), ref, 3, "leading_I")
            add(np.array(seqs[ref][:m], np.uint8), ref, 0, "begins_at_column_1")
    # row 1: the first base matches, the next reference symbol is deleted
    for k in range(12):
        ref = (0, 1, 16)[k % 3]
        st = int(rng.integers(2, 300))
        q = np.concatenate([seqs[ref][st:st + 1], seqs[ref][st + 2:st + 40]]).astype(np.uint8)
        add(q, ref, 2, "row1")
    # repeats: where a gap goes, and which of several equally good end columns carries which gapR, is the tie-breaks' business
    for k in range(90):
        ref = (2, 3, 6, 7, 17, 18)[k % 6]
        n_ref = len(seqs[ref])
        m = int(rng.choice([33, 65, 100]))
        st = int(rng.integers(0, n_ref - m - 4))
        ns, ni, nd = (int(x) for x in rng.integers(0, 3, size=3))
        add(edit_read(rng, seqs[ref], st, m, ns, ni + (k % 2), nd), ref, ns + ni + nd + 2, "repeat", strand=k % 2)
    # IUPAC symbols on both sides
    for k in range(30):
        m = int(rng.choice([33, 100]))
        st = int(rng.integers(0, 500 - m))
        q = edit_read(rng, seqs[4], st, m, 1, k % 2, (k // 2) % 2)
        q[int(rng.integers(0, len(q)))] = int(rng.integers(5, 16))
        add(q, 4, 8, "iupac")
    return seqs, queries, rcs, cases
