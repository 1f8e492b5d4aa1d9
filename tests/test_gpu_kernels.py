"""Parity of the HIP path (through the C ABI of include/burst_hip.h) against the oracle on seeded inputs.
Bit-exact: edit distances, hit sets, gap counts, end positions and the f32 identity score."""
import os
import sys

import numpy as np
import pytest

import dbutil
import oraclelib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CW_DEFAULT = 2          # library default of option prefilter_cw (the tests run the other counting-filter kernel as a variant)
from burst_amd import synth

pytestmark = pytest.mark.gpu


def family_db(seed, n_base, n_var, length, rate=0.03, short=False, iupac=0.0):
    rng = np.random.default_rng(seed)
    seqs = []
    for b in range(n_base):
        base = rng.integers(1, 5, size=int(length + rng.integers(-20, 20)), dtype=np.uint8)
        for v in synth.mutate_family(base, n_var, rate, rng):
            if short and rng.random() < 0.2:
                v = v[:int(rng.integers(len(v) // 2, len(v)))]
            if iupac:
                m = np.flatnonzero(rng.random(len(v)) < iupac)
                v[m] = rng.integers(5, 16, size=len(m))
            seqs.append(v)
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order]


def best_per_entry(recs, order):
    """the reference's BEST scan inside each entry (burst.c:4847-4891): fewest edits, then the higher score, then the lower RefIxSrt"""
    keep = {}
    for r in recs:
        k = int(r["q"])
        b = keep.get(k)
        if b is None or r["ed"] < b["ed"] or (r["ed"] == b["ed"] and (r["score"] > b["score"] or (r["score"] == b["score"] and order[r["refIx"]] < order[b["refIx"]]))):
            keep[k] = r
    return np.array([keep[k] for k in sorted(keep)], dtype=recs.dtype)


def budget(thres, n):
    return int(ol.oracle().orc_error_budget(thres, n))


def make_queries(seqs, n, qlen, edits, seed, rc_frac=0.5, iupac=0.0, thres=0.97):
    """forward entries followed by their reverse complements (the layout process_queries builds, burst.c:3087-3107)"""
    from burst_amd.capi import Queries
    reads, _ = synth.make_reads(seqs, n, qlen, edits, seed, rc_frac=rc_frac, iupac_frac=iupac)
    fwd = reads
    rcs = [synth.revcomp(r) for r in reads]
    allq = fwd + rcs
    E = [budget(thres, len(r)) for r in fwd] * 2
    six = list(range(n)) * 2
    rc = [0] * n + [1] * n
    return Queries(allq, E, six, rc), allq


def oracle_hits(packed, clump_len, tot, q, lut, all_hits):
    return ol.search(packed, clump_len, tot, q.codes, q.off, q.emac.astype(np.uint32), q.six, q.rc, q.n_shared, lut, all_hits)


def assert_hits_equal(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    assert got.tobytes() == exp.tobytes()


@pytest.mark.parametrize("qlen,edits,thres,seed", [(100, [0, 1, 2, 3], 0.97, 11), (60, [0, 1], 0.95, 12), (150, [0, 2, 4, 6], 0.95, 13),
                                                   (292, [0, 3, 9], 0.97, 14), (320, [0, 5, 16], 0.95, 15), (33, [0, 1], 0.9, 16),
                                                   (128, [1], 0.97, 17), (129, [1], 0.97, 18), (600, [0, 7], 0.98, 19)])
def test_align_pairs_matches_oracle(qlen, edits, thres, seed):
    from burst_amd import capi
    seqs = family_db(seed, 6, 11, qlen + 150, short=True)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut)
    q, allq = make_queries(seqs, 24, qlen, edits, seed, thres=thres)
    nc = len(clump_len)
    pq = np.repeat(np.arange(q.n, dtype=np.uint32), nc)
    pc = np.tile(np.arange(nc, dtype=np.uint32), q.n)
    mins = dev.align_pairs(q, pq, pc)
    n_le = 0
    for p in range(len(pq)):
        rows = dbutil.clump_rows(seqs, int(pc[p]))
        _, omins = ol.aded_clump(rows, allq[pq[p]], int(q.emac[pq[p]]), lut)
        assert np.array_equal(mins[p], omins), (p, mins[p], omins)
        n_le += int((omins != 255).sum())
    assert n_le > 0
    st = dev.stats()
    assert st["n_pairs"] == len(pq) and st["n_columns"] == int(clump_len[pc].sum())
    dev.close()


@pytest.mark.parametrize("all_hits", [False, True])
@pytest.mark.parametrize("qlen,edits,thres,iupac,seed", [(100, [0, 1, 2, 3, 5], 0.97, 0.0, 21), (292, [0, 4, 9, 12], 0.97, 0.0, 22),
                                                         (320, [0, 8, 16], 0.95, 0.01, 23), (50, [0, 1, 2], 0.95, 0.03, 24)])
def test_align_batch_exhaustive_matches_oracle(qlen, edits, thres, iupac, seed, all_hits):
    from burst_amd import capi
    seqs = family_db(seed, 5, 13, qlen + 200, short=True, iupac=iupac / 2)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut)
    q, _ = make_queries(seqs, 40, qlen, edits, seed, iupac=iupac, thres=thres)
    got = dev.align_batch(q, all_hits=all_hits)
    exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
    assert len(exp) > 20
    assert_hits_equal(got, exp)
    dev.close()


@pytest.mark.parametrize("n_var", [40, 70, 150, 333])
def test_many_records_per_query_come_out_in_the_oracle_order(n_var):
    """k_hit_fix: a query's records leave the device ordered like the host's list (reference number, then the rest) whatever the order the
    lanes finished in -- groups of up to 64 records ranked in registers, larger ones through the scratch copy 64 at a time"""
    from burst_amd import capi
    seqs = family_db(700 + n_var, 2, n_var, 260, rate=0.004)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut)
    q, _ = make_queries(seqs, 30, 100, [0, 1, 2], 700 + n_var, thres=0.95)
    for all_hits in (True, False):
        got = dev.align_batch(q, all_hits=all_hits)
        exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        if all_hits:
            assert np.bincount(exp["q"]).max() > min(n_var, 300) * 0.8       # groups on both sides of 64 and of a multiple of it
        assert_hits_equal(got, exp)
    dev.close()


def test_product_library_alone_refuses_the_superseded_prefilter_kernels():
    """k_prefilter_cf and k_prefilter_cw<0 / 1> are not part of libburst_hip.so (round 6): a process that has not loaded the test-only
    libburst_hip_legacy.so gets an error for prefilter_cw = 0 / 1, and the same batch through the default kernel"""
    import subprocess
    code = (
        "import sys, numpy as np; sys.path[:0] = [%r, %r]\n"
        "import dbutil, oraclelib as ol\n"
        "from burst_amd import capi, synth\n"
        "assert not capi.LOAD_LEGACY_PREFILTERS\n"
        "rng = np.random.default_rng(5); seqs = []\n"
        "for _ in range(4): seqs += synth.mutate_family(rng.integers(1, 5, size=400, dtype=np.uint8), 8, 0.03, rng)\n"
        "packed, clump_len, tot = dbutil.pack_clumps(seqs)\n"
        "lens, entries, offs = dbutil.build_acx(seqs, 10)\n"
        "dev = capi.Device(packed, clump_len, tot, ol.score_lut(1), acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=10)\n"
        "reads, _ = synth.make_reads(seqs, 16, 100, [0, 1, 2], 3)\n"
        "q = capi.Queries(reads, [3] * 16, list(range(16)), [0] * 16)\n"
        "base = dev.align_batch(q)\n"
        "for cw in (0, 1):\n"
        "    dev.set_option('prefilter_cw', cw)\n"
        "    try:\n"
        "        dev.align_batch(q); print('NOT REFUSED', cw)\n"
        "    except capi.BurstHipError as e:\n"
        "        print('refused', cw, 'superseded' in str(e))\n"
        "dev.set_option('prefilter_cw', 2)\n"
        "print('same', dev.align_batch(q).tobytes() == base.tobytes(), len(base))\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "refused 0 True" in r.stdout and "refused 1 True" in r.stdout and "NOT REFUSED" not in r.stdout and "same True" in r.stdout, r.stdout


def test_one_long_read_does_not_move_the_others_to_the_long_kernel(capfd, monkeypatch):
    """Reads of 513 .. 1 024 symbols keep the register kernel of 32 words (k_myers<32>) when ONE read of the batch is longer than 1 024
    symbols: the long ones are a length class of their own (round 6; before, the last class took the word count of the lane's longest
    query and every read in it went through k_myers_long).  Records against the oracle, the classes from the library's debug lines."""
    from burst_amd import capi
    seqs = family_db(4242, 3, 5, 3300, short=False)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut)
    reads = []
    for n, qlen, edits, seed in ((6, 600, [0, 5], 1), (6, 1000, [0, 9], 2), (1, 3000, [12], 3), (8, 100, [0, 2], 4)):
        reads += synth.make_reads(seqs, n, qlen, edits, 4242 + seed, rc_frac=0.0)[0]
    E = [budget(0.98, len(r)) for r in reads]
    q = capi.Queries(reads, E, list(range(len(reads))), [0] * len(reads))
    monkeypatch.setenv("BHIP_DEBUG", "1")
    capfd.readouterr()
    got = dev.align_batch(q, all_hits=False)
    err = capfd.readouterr().err
    monkeypatch.delenv("BHIP_DEBUG")
    exp = oracle_hits(packed, clump_len, tot, q, lut, False)
    assert len(exp) >= len(reads)
    assert_hits_equal(got, exp)
    cls = {int(ln.split("class NW=")[1].split(":")[0]): ln for ln in err.splitlines() if "class NW=" in ln}
    assert 32 in cls and "exhaustive 12 " in cls[32], cls                 # the twelve 600- and 1 000-symbol reads: the 32-word class
    assert 128 in cls and "exhaustive 1 " in cls[128], cls                # the 3 000-symbol read alone in the class beyond 1 024 symbols
    assert 4 in cls
    dev.close()


@pytest.mark.parametrize("n_var,with_acx", [(40, False), (150, False), (90, True)])
def test_best_record_per_entry_chosen_on_the_device(n_var, with_acx):
    """all_hits = 2 (BHIP_HITS_BEST): of an entry's minimum-edit records the device returns the ONE the reference's BEST scan keeps --
    higher f32 score, then lower RefIxSrt[refIx] (burst.c:4847-4891) -- computed here from the oracle's full record set with a random
    permutation as RefIxSrt.  Families of near-identical references: dozens of equally good records per entry, both strands."""
    from burst_amd import capi
    seqs = family_db(900 + n_var, 2, n_var, 260, rate=0.004)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    kw = {}
    if with_acx:
        lens, entries, _ = dbutil.build_acx(seqs, 10)
        kw = dict(acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=10)
    dev = capi.Device(packed, clump_len, tot, lut, **kw)
    q, _ = make_queries(seqs, 30, 100, [0, 1, 2, 3], 900 + n_var, thres=0.95)
    with pytest.raises(capi.BurstHipError):
        dev.align_batch(q, all_hits=2)                    # no table yet
    order = np.random.default_rng(n_var).permutation(tot).astype(np.uint32)
    dev.set_ref_order(order)
    exp_all = oracle_hits(packed, clump_len, tot, q, lut, False)
    assert np.bincount(exp_all["q"]).max() > 20
    # the reference's choice inside each entry: ed is the same for all of an entry's records here; max score, then min order
    exp = best_per_entry(exp_all, order)
    got = dev.align_batch(q, all_hits=2)
    assert len(got) == len(exp) == len(set(exp_all["q"].tolist()))
    assert_hits_equal(got, exp)
    assert_hits_equal(dev.align_batch(q, all_hits=False), exp_all)      # (and the plain mode is untouched by the table)
    # a caller's buffer that is too small: the count comes back, the resident records are delivered by the next call
    dev.stage(q)
    small = np.zeros(3, dtype=capi.HIT_DTYPE)
    got2, _ = dev.align_staged(all_hits=2, out=small)
    assert_hits_equal(got2, exp)
    dev.close()


@pytest.mark.parametrize("qlen,edits,thres,seed", [(1025, [0, 3, 20], 0.98, 61), (1500, [0, 10, 44], 0.97, 62), (2600, [0, 25], 0.99, 63), (4050, [0, 12, 40], 0.99, 64)])
def test_queries_beyond_1024_symbols(qlen, edits, thres, seed):
    """k_myers_long (vector in LDS, any number of words up to BHIP_MAX_QLEN symbols): the sweep on its own against aded of the oracle,
    then whole batches -- exhaustive, and through an accelerator with a few ambiguous symbols in the reads and mixed with short reads
    (one lane then holds classes of 4 and of ceil(len / 32) words) -- record for record against the oracle's search"""
    from burst_amd import capi
    assert capi.BHIP_MAX_QLEN == 4095
    seqs = family_db(seed, 3, 6, qlen + 120, short=False)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut)
    q, allq = make_queries(seqs, 5, qlen, edits, seed, thres=thres)
    nc = len(clump_len)
    pq = np.repeat(np.arange(q.n, dtype=np.uint32), nc)
    pc = np.tile(np.arange(nc, dtype=np.uint32), q.n)
    mins = dev.align_pairs(q, pq, pc)
    n_le = 0
    for p in range(len(pq)):
        rows = dbutil.clump_rows(seqs, int(pc[p]))
        _, omins = ol.aded_clump(rows, allq[pq[p]], int(q.emac[pq[p]]), lut)
        assert np.array_equal(mins[p], omins), (p, mins[p], omins)
        n_le += int((omins != 255).sum())
    assert n_le > 0
    for all_hits in (False, True):
        got = dev.align_batch(q, all_hits=all_hits)
        exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        assert len(exp) >= 5
        assert_hits_equal(got, exp)
    dev.close()
    # with an accelerator: long reads (some with ambiguous symbols) beside short ones
    K = 12
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lists = dbutil.pack_acx_lists(lens, entries, 0)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=0, K=K)
    long_reads, _ = synth.make_reads(seqs, 4, qlen, edits, seed + 1, rc_frac=0.0, iupac_frac=0.002)
    short_reads, _ = synth.make_reads(seqs, 6, 100, [0, 1, 2], seed + 2, rc_frac=0.0)
    reads = [long_reads[0], short_reads[0], short_reads[1], long_reads[1], short_reads[2], long_reads[2], short_reads[3], short_reads[4], long_reads[3], short_reads[5]]
    E = [budget(thres, len(r)) for r in reads]
    qa = capi.Queries(reads, E, list(range(len(reads))), [0] * len(reads))
    for all_hits in (False, True):
        got = dev.align_batch(qa, all_hits=all_hits)
        exp = oracle_hits(packed, clump_len, tot, qa, lut, all_hits)
        assert len(exp) >= 8
        assert_hits_equal(got, exp)
    st = dev.stats()
    assert st["n_pairs"] <= qa.n * nc
    dev.close()
    # exactly BHIP_MAX_QLEN symbols (128 words: all of the 64 KB of LDS a block may ask for); one symbol more is refused, loudly
    if qlen == 4050:
        dev = capi.Device(packed, clump_len, tot, lut)
        src = max(seqs, key=len)
        assert len(src) >= 4096
        q1 = capi.Queries([src[:4095].copy()], [budget(thres, 4095)], [0], [0])
        got = dev.align_batch(q1, all_hits=True)
        exp = oracle_hits(packed, clump_len, tot, q1, lut, True)
        assert len(exp) >= 1
        assert_hits_equal(got, exp)
        with pytest.raises(capi.BurstHipError):
            dev.align_batch(capi.Queries([src[:4096].copy()], [10], [0], [0]))
        dev.close()


def test_mixed_lengths_and_empty():
    from burst_amd import capi
    seqs = family_db(31, 4, 16, 500)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut)
    rng = np.random.default_rng(5)
    reads = []
    for L in [20, 64, 65, 100, 128, 129, 192, 193, 256, 257, 320, 321, 400, 30, 100, 100]:
        r, _ = synth.make_reads(seqs, 1, L, [0, 1, 2], int(rng.integers(1 << 30)))
        reads += r
    E = [budget(0.96, len(r)) for r in reads]
    q = capi.Queries(reads, E, list(range(len(reads))), [0] * len(reads))
    got = dev.align_batch(q)
    exp = oracle_hits(packed, clump_len, tot, q, lut, False)
    assert_hits_equal(got, exp)
    # empty batch
    q0 = capi.Queries([], [], [], [])
    assert len(dev.align_batch(q0)) == 0
    dev.close()


@pytest.mark.parametrize("K,fmt,stride", [(8, 0, 1), (9, 1, 1), (12, 0, 1), (12, 0, 4), (12, 0, 12), (10, 0, 3)])
def test_prefilter_matches_oracle(K, fmt, stride):
    """stride 1 = the reference's scheme (every word, count > len-(E+1)K); larger strides = sparse seeds"""
    from burst_amd import capi
    seqs = family_db(41 + K, 12, 9, 420)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lists = dbutil.pack_acx_lists(lens, entries, fmt)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=fmt, K=K)
    dev.set_option("prefilter_stride", stride)
    q, allq = make_queries(seqs, 30, 100, [0, 1, 2, 3], 43, thres=0.97)
    oq, oc, on = dev.prefilter(q)
    exp = []
    for j in range(q.n):
        _, counts = ol.prefilter_counts(allq[j], int(q.emac[j]), K, offs, entries, len(clump_len), stride)
        E = int(q.emac[j]); m = len(allq[j])
        need = ((m - K) // stride + 1) - E * ((K + stride - 1) // stride)
        for c in np.flatnonzero(counts > max(need - 1, 0)):
            exp.append((j, int(c), int(counts[c])))
    got = list(zip(oq.tolist(), oc.tolist(), on.tolist()))
    assert got == exp and len(exp) > 0
    dev.close()


def test_sparse_seed_prefilter_never_loses_a_hit():
    """automatic stride: every (query, clump) holding a lane within budget must be a candidate"""
    from burst_amd import capi
    K = 12
    seqs = family_db(77, 16, 10, 500, rate=0.06)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lists = dbutil.pack_acx_lists(lens, entries, 0)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=0, K=K)
    for thres, edits in ((0.97, [0, 1, 2, 3]), (0.93, [0, 3, 5, 7]), (0.98, [0, 1, 2])):
        q, allq = make_queries(seqs, 40, 100, edits, 78, thres=thres)
        oq, oc, _ = dev.prefilter(q)
        cand = set(zip(oq.tolist(), oc.tolist()))
        nc = len(clump_len)
        mins = dev.align_pairs(q, np.repeat(np.arange(q.n, dtype=np.uint32), nc), np.tile(np.arange(nc, dtype=np.uint32), q.n)).reshape(q.n, nc, 16)
        need = {(j, c) for j in range(q.n) for c in range(nc) if (mins[j, c] != 255).any() and len(allq[j]) >= K
                and int(q.emac[j]) < len(allq[j]) // K}
        assert need and need <= cand
        assert len(cand) < q.n * nc // 2
    dev.close()


@pytest.mark.parametrize("all_hits", [False, True])
def test_align_batch_with_accelerator_equals_exhaustive(all_hits):
    from burst_amd import capi
    K = 10
    seqs = family_db(51, 20, 8, 450, short=True)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    nc = len(clump_len)
    lens, entries, offs = dbutil.build_acx(seqs, K, skip_clumps=(nc - 1,))   # BadList clumps carry no words (burst.c:3432-3437)
    lists = dbutil.pack_acx_lists(lens, entries, 0)
    lut = ol.score_lut(1)
    bad = np.array([nc - 1], np.uint32)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=0, K=K, badlist=bad)
    q, _ = make_queries(seqs, 60, 100, [0, 1, 2, 3, 6], 53, thres=0.97)
    q.flags = np.zeros(q.n, np.uint8)
    q.flags[::7] = capi.BHIP_Q_EXHAUSTIVE
    got = dev.align_batch(q, all_hits=all_hits)
    exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
    assert len(exp) > 30
    assert_hits_equal(got, exp)
    st = dev.stats()
    assert st["n_pairs"] < q.n * nc          # the prefilter really pruned
    dev.close()


@pytest.mark.parametrize("thres,iupac", [(0.97, 0.02), (0.94, 0.04)])
def test_ambiguous_queries_through_the_prefilter(thres, iupac):
    """queries with IUPAC codes / N take the accelerated route: words containing them do not vote and the guaranteed
    count shrinks; entries left without any guaranteed word are aligned exhaustively by the library itself"""
    from burst_amd import capi
    K = 12
    seqs = family_db(91, 14, 9, 480, iupac=0.003)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    # (clumps holding an ambiguous reference symbol on the BadList: the test builder does not expand ambiguous reference words the way
    # make_accelerator does -- burst.c:3368-3377 --, so their lanes must not depend on votes)
    bad = sorted({i // 16 for i, s in enumerate(seqs) if (np.asarray(s) > 4).any()})
    lens, entries, offs = dbutil.build_acx(seqs, K, skip_clumps=tuple(bad))
    lists = dbutil.pack_acx_lists(lens, entries, 0)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=0, K=K, badlist=np.array(bad, np.uint32))
    q, allq = make_queries(seqs, 80, 100, [0, 1, 2, 3], 93, iupac=iupac, thres=thres)
    assert sum(int((np.asarray(r) > 4).any()) for r in allq) > 20
    q.flags = np.zeros(q.n, np.uint8)
    for all_hits in (False, True):
        got = dev.align_batch(q, all_hits=all_hits)
        exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        assert len(exp) > 20
        assert_hits_equal(got, exp)
    dev.close()


@pytest.mark.parametrize("K,qlen,thres,iupac,z", [(12, 100, 0.97, 0.03, 1), (12, 150, 0.95, 0.05, 1), (10, 250, 0.95, 0.03, 0), (15, 320, 0.95, 0.015, 1), (12, 100, 0.97, 0.08, 0)])
def test_ambiguous_words_vote_through_expansions(K, qlen, thres, iupac, z):
    """with non-overlapping sampled words (stride K) a word that holds ONE ambiguous symbol votes through its expansions (the first
    alternative in the word's slot, the others in spare word slots: bhip_internal.h, k_seed_ranges; the reference expands query words
    too, burst.c:3232-3236), so reads with several IUPAC codes keep a guaranteed count and stay on the accelerated route.  Identical
    records to the oracle -- with the stride left to the library and forced to K, both prefilter kernels, the clump-level path (whose
    kernels count strictly and take need - x), minima and every hit; z = 0: N matches everything and expands four ways"""
    from burst_amd import capi
    seqs = family_db(300 + K + qlen, 12, 9, qlen + 260, iupac=0.002)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(z)
    # the accelerator built on the device: ambiguous REFERENCE words are expanded into the lists as make_accelerator does (a list
    # without them breaks the vote guarantee for lanes with IUPAC symbols, whoever counts)
    dev = capi.Device(packed, clump_len, tot, lut, K=K, build_acx=True)
    q, allq = make_queries(seqs, 120, qlen, [0, 1, 2, 3], 400 + K, iupac=iupac, thres=thres)
    namb = np.array([int((np.asarray(r) > 4).sum()) for r in allq])
    assert (namb >= 2).sum() > 40 and (namb >= 4).sum() > 5
    q.flags = np.zeros(q.n, np.uint8)
    exp = {ah: oracle_hits(packed, clump_len, tot, q, lut, ah) for ah in (False, True)}
    assert len(exp[False]) > 40
    for opts in ({}, {"prefilter_stride": K}, {"prefilter_stride": K, "prefilter_cw": 0}, {"prefilter_stride": K, "prefilter_cw": 1}, {"prefilter_stride": K, "prefilter_cw": 2}, {"prefilter_stride": K, "prefilter_algo": 1},
                 {"prefilter_stride": K, "lane_masks": 0}, {"prefilter_stride": K, "prefilter_table": 9, "prune": 0}, {"prefilter_stride": K, "prefilter_cw": 1, "prune": 0}, {"prefilter_stride": K, "prefilter_cw": 2, "prune": 0}):
        for k, v in opts.items():
            dev.set_option(k, v)
        for all_hits in (False, True):
            assert_hits_equal(dev.align_batch(q, all_hits=all_hits), exp[all_hits])
        for k in opts:
            dev.set_option(k, {"prefilter_stride": 0, "prefilter_algo": -1, "lane_masks": 1, "prefilter_table": 0, "prune": 1, "prefilter_cw": CW_DEFAULT}[k])
    dev.close()


@pytest.mark.parametrize("qlen,stride,thres", [(100, 0, 0.97), (250, 4, 0.96), (250, 0, 0.95)])
def test_tuning_options_do_not_change_results(qlen, stride, thres):
    """table size of the lane-resolved prefilter, register vs LDS band re-scorer, number of sub-pipelines and seed stride are
    performance knobs only: every combination must return the oracle's records (250-bp reads at stride 4 sample 60 words:
    more than one 16-word chunk per query and more list records than stay in registers between the two passes)"""
    from burst_amd import capi
    K = 12
    seqs = family_db(131, 6, 48, 520, rate=0.04)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lists = dbutil.pack_acx_lists(lens, entries, 0)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=0, K=K)
    q, _ = make_queries(seqs, 90, qlen, [0, 1, 2, 3, 5, 8], 133, thres=thres)
    q.flags = np.zeros(q.n, np.uint8)
    exp = oracle_hits(packed, clump_len, tot, q, lut, False)
    assert len(exp) > 40
    dev.set_option("prefilter_stride", stride)
    dev.set_option("lane_min_entries", 8)
    for table in (9, 10, 11):
        for reg in (1, 0):
            for lanes in (1, 3):
                dev.set_option("prefilter_table", table)
                dev.set_option("rescore_reg", reg)
                dev.set_option("lanes", lanes)
                dev.set_option("prefilter_cw", 0)      # (the table size is k_prefilter_cf's knob)
                got = dev.align_batch(q, all_hits=False)
                assert_hits_equal(got, exp)
    dev.set_option("prefilter_cw", CW_DEFAULT)
    for cw, prune in ((0, 1), (0, 0), (1, 1), (1, 0), (2, 1), (2, 0)):          # the three counting-filter kernels, with and without the deferred second sweep
        for lanes in (1, 3):
            dev.set_option("lanes", lanes)
            dev.set_option("prefilter_cw", cw); dev.set_option("prune", prune)
            assert_hits_equal(dev.align_batch(q, all_hits=False), exp)
    dev.set_option("lanes", 1)
    dev.set_option("prefilter_cw", CW_DEFAULT); dev.set_option("prune", 1)
    dev.set_option("prefilter_table", 0)
    dev.set_option("rescore_reg", 1)
    for oversub, band, band_blocks in ((1, 1, 0), (4, 0, 0), (3, 1, 5), (2, 1, 0)):      # grids of the per-item kernels, banded / full-column windows
        dev.set_option("oversub", oversub); dev.set_option("band", band); dev.set_option("band_blocks", band_blocks)
        assert_hits_equal(dev.align_batch(q, all_hits=False), exp)
    exp_all = oracle_hits(packed, clump_len, tot, q, lut, True)
    assert_hits_equal(dev.align_batch(q, all_hits=True), exp_all)
    dev.close()


@pytest.mark.parametrize("qlen,thres,edits", [(100, 0.97, [0, 1, 2, 3]), (150, 0.95, [0, 3, 7]), (200, 0.97, [0, 2, 6]), (292, 0.97, [0, 4, 8, 9]),
                                              (320, 0.95, [0, 8, 16]), (400, 0.9, [0, 10, 40]), (700, 0.98, [0, 5, 14])])
def test_banded_window_equals_full_column(qlen, thres, edits):
    """k_myers_window_band<2..4> steps only the words of the column the flagged diagonals cross; the full-column kernel takes the
    windows no band holds.  Option "band" 0 sends every window through the full column: same records, both equal to the oracle.
    References with tandem repeats flag long runs of columns (wide windows, several classes in one batch); reads from the first and
    last columns of a lane put the band against the matrix edges."""
    from burst_amd import capi
    K = 12
    rng = np.random.default_rng(7 * qlen)
    seqs = family_db(300 + qlen, 5, 20 if qlen <= 200 else 8, qlen + 260, rate=0.03)
    unit = rng.integers(1, 5, size=int(rng.integers(3, 9)), dtype=np.uint8)
    for i in range(0, len(seqs), 4):                       # a tandem repeat inside every fourth reference
        sq = np.array(seqs[i], np.uint8); a = int(rng.integers(20, len(sq) - 120)); n = int(rng.integers(40, 100))
        sq[a:a + n] = np.resize(unit, n); seqs[i] = sq
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lut = ol.score_lut(1)
    q, allq = make_queries(seqs, 70 if qlen <= 200 else 30, qlen, edits, 500 + qlen, thres=thres)
    # reads cut from the two ends of references
    ends = []
    for i in range(0, len(seqs), 7):
        sq = np.array(seqs[i], np.uint8)
        ends += [sq[:qlen].copy(), sq[len(sq) - qlen:].copy(), sq[1:qlen + 1].copy()]
    nq = len(ends)
    allr = ends + [synth.revcomp(r) for r in ends]
    q2 = capi.Queries(allr, [budget(thres, qlen)] * (2 * nq), list(range(nq)) * 2, [0] * nq + [1] * nq)
    exps = {(i, ah): oracle_hits(packed, clump_len, tot, qq, lut, ah) for i, qq in enumerate((q, q2)) for ah in (False, True)}
    assert all(len(e) > 10 for e in exps.values())
    for accel in (True, False):
        kw = dict(acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=K) if accel else {}
        dev = capi.Device(packed, clump_len, tot, lut, **kw)
        dev.set_option("lane_min_entries", 8)
        for i, qq in enumerate((q, q2)):
            qq.flags = np.zeros(qq.n, np.uint8) if accel else None
            for all_hits in (False, True):
                for band in (1, 0):
                    dev.set_option("band", band)
                    assert_hits_equal(dev.align_batch(qq, all_hits=all_hits), exps[(i, all_hits)])
        dev.close()


def test_prefilter_overflow_paths():
    """one huge family: every query meets > 300 clumps.  With the 512-slot table the per-query hash overflows (dense
    fallback kernel); with 2048 slots it fits but there are far more than 24 candidate clumps per query (clump-level
    pairs handed to the 16-lane sweep).  Same records either way."""
    from burst_amd import capi
    K = 12
    seqs = family_db(141, 1, 5200, 300, rate=0.02)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    assert len(clump_len) > 300
    lens, entries, offs = dbutil.build_acx(seqs, K)
    lists = dbutil.pack_acx_lists(lens, entries, 0)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=lists, acx_fmt=0, K=K)
    q, _ = make_queries(seqs, 12, 100, [0, 1, 3], 143, thres=0.97)
    q.flags = np.zeros(q.n, np.uint8)
    for all_hits in (False, True):
        exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        assert len(exp) > 12
        dev.set_option("prefilter_cw", 0)          # (the table sizes are k_prefilter_cf's)
        for table in (9, 11, 0):
            dev.set_option("prefilter_table", table)
            assert_hits_equal(dev.align_batch(q, all_hits=all_hits), exp)
        # k_prefilter_cw / k_prefilter_cq: > 64 / > 32 surviving clumps overflow the first pass's lane table, > 256 / > 128 the second pass's (dense fallback)
        for cw in (1, 2):
            dev.set_option("prefilter_cw", cw)
            assert_hits_equal(dev.align_batch(q, all_hits=all_hits), exp)
        dev.set_option("prefilter_cw", CW_DEFAULT)
    dev.close()


def test_randomised_configurations():
    """a short run of tests/fuzz_gpu.py: random databases, read sets, budgets and tuning options against the oracle
    (a 7-minute run of the same script, 1331 configurations / 193 k records, is the round's parity stress test)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # BHIP_POISON: every device buffer starts as 0xA5 bytes instead of what its last owner left -- a kernel that reads what nobody wrote
    # fails here and not in the 235th configuration of one long process (round 6)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_gpu.py"), "45", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, BHIP_POISON="165"))
    assert r.returncode == 0 and "fuzz ok" in r.stdout, r.stdout[-3000:]


def test_overflow_list_of_an_earlier_length_class_is_not_taken_for_this_one():
    """Round 6, found by a five-minute fuzzer run (seed 2026, configuration 235; reproduced under BHIP_POISON): 64-symbol reads with a
    budget of 6 take the one-stage sweep and the clump-level prefilter, whose overflowed queries are counted in the lane's shared
    counter; the 65 / 66-symbol reads of the same batch sit in the next length class, whose lane-resolved prefilter found that count
    and ran its second pass over list positions of the OTHER class -- reads beyond its seed ranges (a device fault when the memory
    behind them holds anything but small numbers).  The configuration itself, fast-forwarded, under poisoned allocations."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_gpu.py"), "100000", "2026"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, BHIP_POISON="165", FUZZ_SKIP_TO="235", FUZZ_STOP_AFTER="235"))
    assert r.returncode == 0 and "fuzz ok: 235 configurations" in r.stdout, r.stdout[-3000:]


def test_lane_masks_built_in_slices():
    """databases whose (word, clump, lane) tuples do not fit next to them get their lane masks slice by slice; forced here
    with a slice of 5 000 reference positions (3 clumps): same tasks and records as with one slice"""
    import subprocess
    import sys
    code = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import test_gpu_kernels as T, dbutil, oraclelib as ol
from burst_amd import capi
capi.LOAD_LEGACY_PREFILTERS = True          # (the superseded kernels run as variants here: the test-only library in front of the product's)
seqs = T.family_db(151, 9, 21, 480, rate=0.05)
packed, clump_len, tot = dbutil.pack_clumps(seqs)
lens, entries, offs = dbutil.build_acx(seqs, 12)
lut = ol.score_lut(1)
dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=12)
q, _ = T.make_queries(seqs, 70, 100, [0, 1, 2, 3, 5], 153, thres=0.97)
q.flags = np.zeros(q.n, np.uint8)
got = dev.align_batch(q, all_hits=False)
exp = T.oracle_hits(packed, clump_len, tot, q, lut, False)
assert len(exp) > 40 and got.tobytes() == exp.tobytes()
print("tasks", dev.stats()["n_lane_tasks"])
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for env in ({}, {"BHIP_MASK_SLICE": "5000"}):
        r = subprocess.run([sys.executable, "-c", code, root], env=dict(os.environ, BHIP_DEBUG="1", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append((r.stdout.strip().splitlines()[-1], [ln for ln in r.stderr.splitlines() if "lane masks" in ln][-1]))
    assert outs[0][0] == outs[1][0] and int(outs[0][0].split()[1]) > 0          # same number of lane tasks
    assert "in 1 slice" in outs[0][1] and "in 1 slice" not in outs[1][1]


def test_entry_numbers_beyond_32_bits():
    """The device accelerator numbers its list entries with 40 bits (64-bit block bases + 32-bit offsets inside a block of 256
    words, 5-byte records).  A RefSeq-scale accelerator (~5 * 10^10 entries) does not fit a test, so the test hook
    BHIP_TEST_ENTRY_BIAS makes the entry numbers of a small database START near 2^32 (and, second run, beyond 2^36): every
    offset the kernels compute crosses the 32-bit limit.  Lane-resolved and clump-level prefilter, SMALL and LARGE lists, the
    kernel-level prefilter entry: all must equal the oracle, and the device layout must stay <= 5 bytes per entry + offsets."""
    import subprocess
    import sys
    code = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import test_gpu_kernels as T, dbutil, oraclelib as ol
from burst_amd import capi
capi.LOAD_LEGACY_PREFILTERS = True          # (the superseded kernels run as variants here: the test-only library in front of the product's)
K = 12
seqs = T.family_db(191, 10, 20, 480, rate=0.05)
packed, clump_len, tot = dbutil.pack_clumps(seqs)
lens, entries, offs = dbutil.build_acx(seqs, K)
lut = ol.score_lut(1)
for fmt in (0, 1):
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, fmt), acx_fmt=fmt, K=K)
    q, allq = T.make_queries(seqs, 70, 100, [0, 1, 2, 3, 5], 193, thres=0.97)
    q.flags = np.zeros(q.n, np.uint8)
    for all_hits in (False, True):
        exp = T.oracle_hits(packed, clump_len, tot, q, lut, all_hits)
        assert len(exp) > 40
        for opts in ({"lane_masks": 1, "prefilter_algo": 0, "prefilter_cw": 0}, {"lane_masks": 1, "prefilter_algo": 0, "prefilter_cw": 1}, {"lane_masks": 1, "prefilter_algo": 0, "prefilter_cw": 2},
                     {"lane_masks": 1, "prefilter_algo": 1}, {"lane_masks": 0}):
            for k, v in opts.items():
                dev.set_option(k, v)
            got = dev.align_batch(q, all_hits=all_hits)
            assert got.tobytes() == exp.tobytes(), (fmt, all_hits, opts)
    dev.set_option("prefilter_stride", 1)
    oq, oc, on = dev.prefilter(q)
    n_exp = 0
    for j in range(q.n):
        _, counts = ol.prefilter_counts(allq[j], int(q.emac[j]), K, offs, entries, len(clump_len), 1)
        need = (len(allq[j]) - K + 1) - int(q.emac[j]) * K
        sel = np.flatnonzero(counts > max(need - 1, 0))
        got_j = oc[oq == j]
        assert np.array_equal(got_j, sel.astype(np.uint32)), j
        n_exp += len(sel)
    assert n_exp == len(oq) and n_exp > 0
    dev.close()
print("ok")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for bias in ("0", str((1 << 32) - 1000), str((1 << 36) + 12345)):
        r = subprocess.run([sys.executable, "-c", code, root], env=dict(os.environ, BHIP_DEBUG="1", BHIP_TEST_ENTRY_BIAS=bias), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
        acc = [ln for ln in r.stderr.splitlines() if "[bhip] accelerator:" in ln]
        assert acc and ("first entry number %s)" % bias) in acc[-1], acc
        assert "records 4 B" in acc[-1]


@pytest.mark.parametrize("junk", [False, True])
def test_pipelined_spans_equal_one_call_batches(junk):
    """bhip_stage_spans: a batch = a span of forward entries + a span of their reverse complements, taken straight from the
    caller's arrays (offsets that do not start at 0), staged asynchronously two batches ahead and routed by the device kernel
    (k_route) -- every batch must give the oracle's records with the caller's query numbers, with device and host routing
    alike, also when one batch holds symbols of code 0 (the host pass takes over for that batch only)."""
    from burst_amd import capi
    seqs = family_db(201, 8, 12, 520)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, 12)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=12)
    reads = []
    for L, n, sd in ((100, 70, 203), (150, 30, 204), (64, 20, 205), (20, 8, 206)):
        r, _ = synth.make_reads(seqs, n, L, [0, 1, 2, 3], sd, rc_frac=0.5)
        reads += [np.array(x, np.uint8) for x in r]
    if junk:
        for i in (5, 40, 41, 77):
            reads[i][3 + i % 20] = 0
    U = len(reads)
    allq = reads + [synth.revcomp(r) for r in reads]
    E = [budget(0.96, len(r)) for r in reads] * 2
    big = capi.Queries(allq, E, list(range(U)) * 2, [0] * U + [1] * U)
    big.flags = np.zeros(big.n, np.uint8)
    big.flags[np.array([len(r) < 12 for r in allq])] = capi.BHIP_Q_EXHAUSTIVE
    cuts = [0, 50, 51, 100, U]
    padded = np.concatenate([big.codes, np.zeros(2, np.uint8)])
    codes4 = (padded[0:len(big.codes) + 1:2][:(len(big.codes) + 1) // 2] & 15) | ((padded[1:len(big.codes) + 2:2][:(len(big.codes) + 1) // 2] & 15) << 4)
    # four symbols per byte (A/C/G/T only: code - 1) and 2-byte lengths: what batches without other symbols carry over PCIe
    pad4 = np.concatenate([big.codes, np.zeros(4, np.uint8)])
    nb2 = (len(big.codes) + 3) // 4
    two = ((pad4 - 1) & 3).astype(np.uint8)
    codes2 = (two[0::4][:nb2] | (two[1::4][:nb2] << 2) | (two[2::4][:nb2] << 4) | (two[3::4][:nb2] << 6)).astype(np.uint8)
    len16 = np.diff(big.off).astype(np.uint16)
    packed_upload = [False]
    def spans_of(u0, u1):
        out = []
        for base in (0, U):
            out.append(dict(codes=big.codes, off=big.off[base + u0:base + u1 + 1], emac=big.emac[base + u0:base + u1], rc=big.rc[base + u0:base + u1],
                            flags=big.flags[base + u0:base + u1], q_base=base + u0))
            if packed_upload[0] == 1:
                out[-1]["codes4"] = codes4        # two symbols per byte: what then crosses PCIe
            elif packed_upload[0] == 2:
                out[-1]["len"] = len16[base + u0:base + u1]
                if not junk:
                    out[-1]["codes2"] = codes2
                else:
                    out[-1]["codes4"] = codes4
        return out
    def expected(u0, u1, all_hits):
        sub = capi.Queries(reads[u0:u1] + allq[U + u0:U + u1], E[u0:u1] * 2, list(range(u1 - u0)) * 2, [0] * (u1 - u0) + [1] * (u1 - u0))
        exp = oracle_hits(packed, clump_len, tot, sub, lut, all_hits).copy()
        q = exp["q"].astype(np.int64)
        exp["q"] = np.where(q < u1 - u0, u0 + q, U + u0 + (q - (u1 - u0))).astype(np.uint32)
        return exp
    for host_routing in (0, 1):
        dev.set_option("host_routing", host_routing)
        for all_hits in (False, True):
            packed_upload[0] = (2 if all_hits else 1) if not host_routing else (0 if all_hits else 2)
            # two batches ahead, as bh_align does: the seed lookups and profiles of batch k+1 run while batch k is aligned
            dev.stage_spans(spans_of(cuts[0], cuts[1]), cuts[1] - cuts[0], 150)
            dev.stage_spans(spans_of(cuts[1], cuts[2]), cuts[2] - cuts[1], 0)
            total = 0
            for k in range(len(cuts) - 1):
                if k + 3 < len(cuts):
                    dev.stage_spans(spans_of(cuts[k + 2], cuts[k + 3]), cuts[k + 3] - cuts[k + 2], 0 if k % 2 else 150)
                got, _ = dev.align_staged(all_hits)
                exp = expected(cuts[k], cuts[k + 1], all_hits)
                assert got.tobytes() == exp.tobytes(), (host_routing, all_hits, k)
                total += len(got)
            assert total > 100
    # three staging slots (one batch aligned, one staged with its seed lookups running ahead, one being staged): a fourth batch
    # cannot be staged before one has been aligned
    dev.stage_spans(spans_of(0, 10), 10)
    dev.stage_spans(spans_of(10, 20), 10)
    dev.stage_spans(spans_of(20, 30), 10)
    with pytest.raises(capi.BurstHipError):
        dev.stage_spans(spans_of(30, 40), 10)
    dev.set_option("discard_staged", 1)
    dev.close()


def test_asynchronous_record_handover():
    """option async_d2h: the count is final at return, the bytes after sync_hits(); two alternating host buffers; the
    device-resident copy (bhip_copy_hits_device) refers to the last call"""
    from burst_amd import capi
    seqs = family_db(161, 8, 12, 500)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lens, entries, offs = dbutil.build_acx(seqs, 12)
    lut = ol.score_lut(1)
    dev = capi.Device(packed, clump_len, tot, lut, acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=12)
    q, _ = make_queries(seqs, 80, 100, [0, 1, 2, 3, 5], 163, thres=0.97)
    q.flags = np.zeros(q.n, np.uint8)
    exp = oracle_hits(packed, clump_len, tot, q, lut, False)
    dev.stage(q)
    dev.set_option("async_d2h", 1)
    bufs = [None, None]
    views = []
    for k in range(5):
        h, bufs[k & 1] = dev.align_staged(False, bufs[k & 1])
        assert len(h) == len(exp)
        views.append(h)
    dev.sync_hits()
    assert views[-1].tobytes() == exp.tobytes() and views[-2].tobytes() == exp.tobytes()
    dev.set_option("async_d2h", 0)
    h, _ = dev.align_staged(False)
    assert h.tobytes() == exp.tobytes()
    dev.close()


@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("all_hits", [False, True])
def test_query_symbols_outside_the_alphabet(accel, all_hits):
    """A query symbol of code 0 (anything the reference's character table does not know, burst.c:1288-1307) costs 255 against
    every reference symbol (burst.c:170-190): it can only face a gap.  The device searches such queries without those
    symbols and adds their number back before re-scoring; records must equal the oracle's full-cost DP -- near the start, in
    the middle and near the end of a read, several per read, more than the budget, on both strands."""
    from burst_amd import capi, synth
    seqs = family_db(171, 6, 10, 600)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    kw = {}
    if accel:
        lens, entries, offs = dbutil.build_acx(seqs, 12)
        kw = dict(acx_lens=lens, acx_lists=dbutil.pack_acx_lists(lens, entries, 0), acx_fmt=0, K=12)
    reads, _ = synth.make_reads(seqs, 90, 100, [0, 1, 2, 3], 173, rc_frac=0.5)
    rng = np.random.default_rng(7)
    for i, r in enumerate(reads):
        r = np.array(r, np.uint8)
        k = i % 6                                   # 0 = untouched, 1..4 symbols of code 0, 5 = more than any budget
        # (never the first symbol of either strand: there the reference's re-scorer cannot follow its own search, see the next test)
        pos = {0: [], 1: [1], 2: [len(r) - 2], 3: [int(rng.integers(1, len(r) - 1))]}.get(k)
        if pos is None:
            pos = list(1 + rng.choice(len(r) - 2, size=(2 if k == 4 else 9), replace=False))
        r[pos] = 0
        reads[i] = r
    n = len(reads)
    allq = reads + [synth.revcomp(r) for r in reads]
    q = capi.Queries(allq, [budget(0.95, len(r)) for r in reads] * 2, list(range(n)) * 2, [0] * n + [1] * n)
    if accel:
        q.flags = np.zeros(q.n, np.uint8)
    dev = capi.Device(packed, clump_len, tot, lut, **kw)
    exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
    got = dev.align_batch(q, all_hits=all_hits)
    touched = np.array([(np.asarray(allq[e]) == 0).any() for e in exp["q"]])
    assert touched.sum() > 20 and (~touched).sum() > 10
    assert got.tobytes() == exp.tobytes()
    for opts in ({"two_stage": 0}, {"prune": 0, "rescore_reg": 0}, {"lanes": 3, "lane_min_entries": 4}):
        for k_, v in opts.items():
            dev.set_option(k_, v)
        assert dev.align_batch(q, all_hits=all_hits).tobytes() == exp.tobytes(), opts
    dev.close()


def test_first_symbol_outside_the_alphabet_stops_like_the_reference():
    """Row 1 of reScoreM takes the substitution cost alone (burst.c:722-739), so a query whose FIRST symbol has code 0 cannot
    be re-scored although the search finds it (by gapping that symbol): the reference prints "CRITICAL ERROR: Truncation
    within known good path" and exits (burst.c:812-816); the library returns BHIP_E_RESCORE."""
    from burst_amd import capi, synth
    seqs = family_db(181, 3, 6, 400)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    reads, _ = synth.make_reads(seqs, 8, 80, [0, 1], 183)
    reads = [np.array(r, np.uint8) for r in reads]
    reads[3][0] = 0
    q = capi.Queries(reads, [budget(0.95, len(r)) for r in reads])
    dev = capi.Device(packed, clump_len, tot, ol.score_lut(1))
    with pytest.raises(capi.BurstHipError) as e:
        dev.align_batch(q, all_hits=False)
    assert e.value.code == capi.BHIP_E_RESCORE
    dev.close()


# ---- the redo paths of a batch call (bhip_align_staged): a chain that outgrows its buffers is run again, bands beyond the LDS plan go
# through the global-scratch re-scorer.  The library says so under BHIP_DEBUG ("[bhip] redo: ...", "... n_wide N hits ...") ----
def staged_call(dev, mode, buf):
    """ONE bhip_align_staged call on the staged batch, no retry on the caller's side: (return code, record count)"""
    from burst_amd import capi
    n = capi.C.c_uint64()
    rc = capi.lib().bhip_align_staged(dev._h, mode, capi._ptr(buf), len(buf), capi.C.byref(n))
    return rc, int(n.value)


def with_debug_lines(capfd, monkeypatch, fn):
    """fn() under BHIP_DEBUG: (its result, the library's debug lines)"""
    monkeypatch.setenv("BHIP_DEBUG", "1")
    capfd.readouterr()
    try:
        res = fn()
    finally:
        err = capfd.readouterr().err
        monkeypatch.delenv("BHIP_DEBUG")
    return res, [ln for ln in err.splitlines() if ln.startswith("[bhip]")]


def redo_inputs(n_reads=17000):
    """64 references within one substitution of one 300-symbol sequence (4 clumps), reads of 100 symbols cut from it with 0 - 1 edits and
    a budget of 3: every reference is a hit for every read -- 64 x 17 000 = 1 088 000 raw hits and records"""
    rng = np.random.default_rng(4101)
    base = rng.integers(1, 5, size=300, dtype=np.uint8)
    seqs = []
    for i in range(64):
        v = base.copy()
        if i:
            p = int(rng.integers(0, len(v)))
            v[p] = v[p] % 4 + 1
        seqs.append(v)
    reads, _ = synth.make_reads([base], n_reads, 100, [0, 1], 4102)
    return seqs, reads


def wide_band_inputs(rep=150):
    """A read of "AC" x rep with ONE substitution in the middle (without it every alignment to a repeat is an exact match, and exact matches
    leave in k_rescore_classify: nothing would be re-scored), the plain repeat beside it, and ordinary 100-symbol reads; 24 references of
    600 symbols, every third one "AC" x 300, the others random.  The substituted read meets a repeat with one edit at every second end
    column over hundreds of columns: a band of > 48 (BHIP_RESCORE_WMAX) diagonals."""
    rng = np.random.default_rng(4201)
    ac = np.tile(np.array([1, 2], np.uint8), 300)
    seqs = [ac.copy() if i % 3 == 0 else rng.integers(1, 5, size=600, dtype=np.uint8) for i in range(24)]
    plain = np.tile(np.array([1, 2], np.uint8), rep)
    edited = plain.copy()
    edited[rep] = 3
    ordinary, _ = synth.make_reads([s for i, s in enumerate(seqs) if i % 3], 14, 100, [0, 1, 2, 3], 4202)
    return seqs, ordinary[:7] + [edited, plain] + ordinary[7:]


def test_chain_redone_for_size_gives_the_same_records(capfd, monkeypatch):
    """Exhaustive route, all hits: 1 088 000 raw hits against Lane::raw_cap = 2^18 and as many records against Handle::out_cap = 2^20, so
    the first call runs the chain three times (raw grows, then out).  The redo changes nothing: the second call on the same handle redoes
    nothing and returns the same bytes, so does a fresh handle that gets the reads in eight batches below every limit, and the first
    100 reads' records are the oracle's.  A caller's buffer one record too small gets BHIP_E_CAPACITY and the count; the next call
    delivers the resident records without running the chain."""
    from burst_amd import capi
    seqs, reads = redo_inputs()
    n_r = len(reads)
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    E = [budget(0.97, 100)] * n_r
    assert E[0] == 3
    q = capi.Queries(reads, E, list(range(n_r)), [0] * n_r)
    dev = capi.Device(packed, clump_len, tot, lut)
    dev.stage(q)
    buf = np.zeros(64 * n_r + 16, dtype=capi.HIT_DTYPE)
    (rc, n), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, 1, buf))
    redo = [ln for ln in lines if "redo:" in ln]
    print("first call: rc", rc, "records", n, redo)
    assert rc == capi.BHIP_OK and n > 2 ** 20
    assert any(" raw " in ln for ln in redo) and any(" out " in ln for ln in redo), lines
    first = buf[:n].copy()
    # the same batch again: every buffer is large enough now
    buf[:] = 0
    (rc, n2), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, 1, buf))
    assert rc == capi.BHIP_OK and n2 == n and not [ln for ln in lines if "redo:" in ln], lines
    assert any("list records" in ln for ln in lines)                     # (the chain did run)
    assert buf[:n].tobytes() == first.tobytes()
    # a caller's buffer one record too small, then one that is large enough: the resident records, no chain
    small = np.zeros(n - 1, dtype=capi.HIT_DTYPE)
    rc, n3 = staged_call(dev, 1, small)
    assert rc == capi.BHIP_E_CAPACITY and n3 == n
    buf[:] = 0
    (rc, n4), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, 1, buf))
    assert rc == capi.BHIP_OK and n4 == n and not [ln for ln in lines if "redo:" in ln or "list records" in ln], lines
    assert buf[:n].tobytes() == first.tobytes()
    dev.close()
    # the first 100 reads against the oracle
    q100 = capi.Queries(reads[:100], E[:100], list(range(100)), [0] * 100)
    exp = oracle_hits(packed, clump_len, tot, q100, lut, True)
    assert len(exp) == 6400
    assert_hits_equal(first[first["q"] < 100], exp)
    # a fresh handle, eight batches none of which reaches a limit
    dev = capi.Device(packed, clump_len, tot, lut)
    parts = []
    step = n_r // 8
    assert step * 8 == n_r

    def eight():
        for k in range(8):
            qk = capi.Queries(reads[k * step:(k + 1) * step], E[:step], list(range(step)), [0] * step)
            got = dev.align_batch(qk, all_hits=True, cap=64 * step + 16)
            got["q"] += k * step
            parts.append(got)
    _, lines = with_debug_lines(capfd, monkeypatch, eight)
    assert not [ln for ln in lines if "redo:" in ln], lines
    assert np.concatenate(parts).tobytes() == first.tobytes()
    dev.close()


@pytest.mark.parametrize("all_hits", [False, True])
def test_bands_beyond_the_lds_plan_are_rescored_through_global_scratch(all_hits, capfd, monkeypatch):
    """k_rescore<true>: the hits of wide_band_inputs() (repeat length used: "AC" x 150, with one substitution) have bands of hundreds of
    diagonals and leave the LDS plan of at most BHIP_RESCORE_WMAX = 48; ordinary reads run their narrow bands in the same batch.  Records
    against the oracle, the path taken from the library's debug line."""
    from burst_amd import capi
    seqs, reads = wide_band_inputs()
    packed, clump_len, tot = dbutil.pack_clumps(seqs)
    lut = ol.score_lut(1)
    q = capi.Queries(reads, [budget(0.97, len(r)) for r in reads], list(range(len(reads))), [0] * len(reads))
    exp = oracle_hits(packed, clump_len, tot, q, lut, all_hits)
    assert (exp["q"] == 7).sum() == 8 and (exp["ed"][exp["q"] == 7] == 1).all()       # the edited repeat: one edit against each of the 8 repeats
    assert (exp["q"] == 8).sum() == 8 and len(set(exp["q"].tolist())) > 10
    dev = capi.Device(packed, clump_len, tot, lut)
    dev.stage(q)
    buf = np.zeros(1 << 12, dtype=capi.HIT_DTYPE)
    (rc, n), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, int(all_hits), buf))
    wide = [int(ln.split("n_wide ")[1].split()[0]) for ln in lines if "n_wide " in ln]
    print("n_wide", wide, [ln for ln in lines if "redo:" in ln])
    assert rc == capi.BHIP_OK and wide and wide[0] > 0, lines
    assert_hits_equal(buf[:n].copy(), exp)
    buf[:] = 0
    (rc, n2), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, int(all_hits), buf))
    assert rc == capi.BHIP_OK and not [ln for ln in lines if "redo:" in ln], lines
    assert_hits_equal(buf[:n2].copy(), exp)
    dev.close()
