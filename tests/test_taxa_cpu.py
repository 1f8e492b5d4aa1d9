"""--taxa without a device: the tree builder, bh_taxa_host and bh_taxa_rollup_host (the definition in plain C) against the Python model
(tests/taxalib.py) and the hand case (tests/taxacases.py), the golden .b6 files against the reference's embalmulate table and the model,
the table writer behind solvers of the test's, the refusals of the command lines, and csrc/host/bh_taxa.c as a stand-alone program under
the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import taxacases as tc
import taxalib as tl
from burst_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burst_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BURST_HIP = os.path.join(ROOT, "burst_amd", "burst_hip")
TAX = os.path.join(GOLDEN, "tax.txt")
AGREES = [501, 667, 750, 1000]


def both(parent, header_node, gw, lines, agree):
    """bh_taxa_host and the model on one input: they agree in group_node, own, clade and info[0..4]; returns the model's"""
    gn, own, clade, info = host.taxa_host(parent, header_node, gw, lines, agree)
    want = tl.taxa(parent, header_node, gw, lines, agree)
    assert (gn.tolist(), own.tolist(), clade.tolist(), info[:5].tolist()) == want
    assert info[5:].tolist() == [0, 0, 0]
    return want


# ---- the tree builder ----
def build(tmp_path, strings, ncbi=False, heads=None):
    heads = heads or ["h%d" % i for i in range(len(strings))]
    m = tmp_path / "map.txt"
    m.write_bytes(b"".join(h.encode() + b"\t" + s.encode() + b"\n" for h, s in zip(heads, strings)))
    return host.taxa_tree(heads, str(m), ncbi)


def test_tree_of_the_hand_case(tmp_path):
    names, parent, depth, hn = build(tmp_path, tc.STRINGS)
    assert [n.decode() for n in names] == tc.NAMES and parent.tolist() == tc.PARENT and depth.tolist() == tc.DEPTH and hn.tolist() == tc.HEADER_NODE
    assert tl.tree_of(tc.STRINGS) == (tc.NAMES, tc.PARENT, tc.DEPTH, tc.HEADER_NODE)


def test_tree_edges(tmp_path):
    """trailing ';' removed, an empty inner level is a level, a leading blank stays part of its level, `Unassigned` and the empty string are
    the root, a level that sorts below ';' does not break the preorder property, a header the map lacks is at the root"""
    strings = ["k;p;", "k;p", "k;;s", "k; p", "Unassigned", "", "k;p;;;", "k!x", "k;p;Unassigned", ";"]
    heads = ["h%d" % i for i in range(len(strings))]
    m = tmp_path / "map.txt"
    m.write_bytes(b"".join(h.encode() + b"\t" + s.encode() + b"\n" for h, s in zip(heads, strings)))
    names, parent, depth, hn = host.taxa_tree(heads + ["absent"], str(m))
    names = [n.decode() for n in names]
    assert sorted(names) == sorted(["Unassigned", "k", "k;p", "k;", "k;;s", "k; p", "k!x", "k;p;Unassigned"])
    assert tl.is_preorder(parent.tolist()) and depth.tolist() == tl.depths(parent.tolist())
    at = [names[v] for v in hn]
    assert at == ["k;p", "k;p", "k;;s", "k; p", "Unassigned", "Unassigned", "k;p", "k!x", "k;p;Unassigned", "Unassigned", "Unassigned"]
    for v in range(1, len(names)):      # a node's parent is the name without its last level; its depth the number of levels
        assert names[parent[v]] == (names[v].rsplit(";", 1)[0] if ";" in names[v] else "Unassigned") and depth[v] == names[v].count(";") + 1
    # the model builds the same tree up to the order of siblings
    mn, mp, md, mh = tl.tree_of(strings + [""])
    assert sorted(zip(mn, [mn[p] for p in mp], md)) == sorted(zip(names, [names[p] for p in parent], depth.tolist())) and [mn[v] for v in mh] == at


def test_tree_depth_limit_names_the_header(tmp_path):
    ok = ";".join("l%d" % i for i in range(64))
    names, parent, depth, hn = build(tmp_path, [ok, "a"])
    assert len(names) == 66 and depth.max() == 64 and names[hn[0]].decode() == ok
    with pytest.raises(host.HostError, match="error -1.*'deep one'.*65 levels"):
        build(tmp_path, ["a", ok + ";x"], heads=["fine", "deep one"])


def test_tree_of_a_map_without_lines():
    """a map that holds nothing sends every header to the root (bh_tax_lookup's answer for it): a tree of the root alone"""
    tax, tree = host.BhTax(), host.BhTaxaTree()
    arr = (C.c_char_p * 2)(b"h0", b"h1")
    assert host.lib().bh_taxa_tree(2, arr, C.byref(tax), 0, C.byref(tree)) == 0
    assert (tree.n_nodes, tree.n_headers, tree.name[0], tree.header_node[0], tree.header_node[1]) == (1, 2, b"Unassigned", 0, 0)
    host.lib().bh_taxa_tree_free(C.byref(tree))


def test_tree_honours_ncbi_lookup(tmp_path):
    m = tmp_path / "map.txt"
    m.write_text("ACC1\ta;b\nACC2\ta;c\n")
    heads = [">gi|ACC1.2 x", ">gi|ACC2"]
    assert [n.decode() for n in host.taxa_tree(heads, str(m), True)[0]] == ["Unassigned", "a", "a;b", "a;c"]
    assert [n.decode() for n in host.taxa_tree(heads, str(m), False)[0]] == ["Unassigned"]


# ---- bh_taxa_host against the model ----
@pytest.mark.parametrize("agree", sorted(tc.EXPECT))
def test_hand_case(agree):
    assert both(tc.PARENT, tc.HEADER_NODE, tc.GROUP_W, tc.LINES, agree) == tc.EXPECT[agree]


@pytest.fixture(scope="module")
def random_cases():
    out = []
    for seed in (1, 2, 3):
        raw, hraw, gw, lines = tl.random_case(seed, n_nodes=[200, 60, 9][seed - 1])
        out.append((raw, hraw, gw, lines, tl.preorder(raw), tl.preorder(raw, reverse=True)))
    return out


@pytest.mark.parametrize("agree", AGREES)
def test_random_trees_in_two_sibling_orders(random_cases, agree):
    deep = 0
    for raw, hraw, gw, lines, (pa, na), (pb, nb) in random_cases:
        assert pa != pb and tl.is_preorder(pa) and tl.is_preorder(pb)
        ga, oa, ca, ia = both(pa, [na[v] for v in hraw], gw, lines, agree)
        gb, ob, cb, ib = both(pb, [nb[v] for v in hraw], gw, lines, agree)
        # the same result in terms of the raw nodes
        assert ia == ib and [oa[na[v]] for v in range(len(raw))] == [ob[nb[v]] for v in range(len(raw))] and [ca[na[v]] for v in range(len(raw))] == [cb[nb[v]] for v in range(len(raw))]
        back = {na[v]: v for v in range(len(raw))}, {nb[v]: v for v in range(len(raw))}
        assert [back[0].get(x, x) for x in ga] == [back[1].get(x, x) for x in gb]
        assert ca[0] == ia[2] and ga.count(tl.NONE) >= 6
        deep = max(deep, ia[4])
    assert deep >= 3      # (the cases reach below the first levels)


def test_host_refusals():
    P, H, W, L = tc.PARENT, tc.HEADER_NODE, tc.GROUP_W, tc.LINES
    for args in (([1, 0], [0], W, L), ([0, 0, 2], [0] * 6, W, L), ([0, 0, 0, 1], [0] * 6, W, L), (P, [7] + H[1:], W, L), (P, H, W, [(7, 0)]), (P, H, W, [(0, 6)]),
                 ([0] + list(range(65)), [0] * 6, W, L)):
        with pytest.raises(host.HostError, match="error -1"):
            host.taxa_host(*args)
    for agree in (0, 500, 1001):
        with pytest.raises(host.HostError, match="error -1.*agree"):
            host.taxa_host(P, H, W, L, agree)
    gn, own, clade, info = host.taxa_host([0] + list(range(64)), [64], [2], [(0, 0)])      # a chain of 64 levels is the limit
    assert gn.tolist() == [64] and own[64] == 2 and clade.tolist() == [2] * 65 and info[:5].tolist() == [1, 1, 2, 0, 64]
    gn, own, clade, info = host.taxa_host(P, H, W, [])
    assert gn.tolist() == [tl.NONE] * 7 and not own.any() and not clade.any() and not info.any()


def test_rollup_against_the_model(random_cases):
    rng = np.random.default_rng(5)
    for raw, hraw, gw, lines, (pa, na), _ in random_cases:
        hn = [na[v] for v in hraw]
        counts = [int(x) for x in rng.integers(0, 1 << 62, size=len(hn), dtype=np.uint64)]
        own, clade = host.taxa_rollup_host(pa, hn, counts)
        assert (own.tolist(), clade.tolist()) == tl.rollup(pa, hn, counts)
    own, clade = host.taxa_rollup_host(tc.PARENT, tc.HEADER_NODE, [5, 7, 11, 13, 17, 1 << 62])
    assert own.tolist() == [17, 0, 0, (1 << 62) + 5, 7, 11, 13] and clade.tolist() == [(1 << 62) + 53, (1 << 62) + 23, (1 << 62) + 12, (1 << 62) + 5, 7, 11, 13]
    with pytest.raises(host.HostError, match="error -1"):
        host.taxa_rollup_host([0, 0, 0, 1], [0], [1])


# ---- the table object (bh_taxa.c) ----
class Table:
    """bh_taxa.c's tables over any headers and a map file; solvers: None = bh_taxa_host and bh_taxa_rollup_host, or run(parent, header_node,
    group_w, lines, agree) -> (own, clade) or an int = its error"""

    def __init__(self, prefix, heads, tax_file, agree=1000, run=None):
        self.h, self.tax, self.calls = C.c_void_p(), host.BhTax(), []
        assert host.lib().bh_tax_load(tax_file.encode(), C.byref(self.tax)) == 0
        arr = (C.c_char_p * len(heads))(*[x.encode() for x in heads])
        rc = host.lib().bh_taxa_open_heads(prefix.encode(), len(heads), arr, C.byref(self.tax), 0, agree, C.byref(self.h))
        assert rc == 0, host.lib().bh_last_error()
        if run is None:
            host.lib().bh_taxa_set_solver(self.h, C.cast(host.lib().bh_taxa_host, C.c_void_p), C.cast(host.lib().bh_taxa_rollup_host, C.c_void_p), None)
            return

        def _run(ctx, nn, parent, nh, hnode, ng, gw, lines, n, agree_, gnode, own, clade, info):
            p = np.frombuffer((C.c_uint8 * (4 * nn)).from_address(parent), np.uint32).copy()
            hn = np.frombuffer((C.c_uint8 * (4 * nh)).from_address(hnode), np.uint32).copy()
            g = np.frombuffer((C.c_uint8 * (4 * ng)).from_address(gw), np.uint32).copy() if ng else np.zeros(0, np.uint32)
            ln = np.frombuffer((C.c_uint8 * (8 * n)).from_address(lines), capi.EM_LINE_DTYPE).copy() if n else np.zeros(0, capi.EM_LINE_DTYPE)
            self.calls.append((p, hn, g, ln, int(agree_)))
            r = run(p.tolist(), hn.tolist(), g.tolist(), list(zip(ln["group"].tolist(), ln["ref"].tolist())), int(agree_))
            if isinstance(r, int):
                return r
            for dst, src in ((own, r[0]), (clade, r[1])):
                a = np.asarray(src, np.uint64)
                C.memmove(dst, a.ctypes.data, 8 * nn)
            return 0

        def _rollup(ctx, nn, parent, nh, hnode, counts, own, clade):
            p = np.frombuffer((C.c_uint8 * (4 * nn)).from_address(parent), np.uint32).tolist()
            hn = np.frombuffer((C.c_uint8 * (4 * nh)).from_address(hnode), np.uint32).tolist()
            c = np.frombuffer((C.c_uint8 * (8 * nh)).from_address(counts), np.uint64).tolist()
            for dst, src in zip((own, clade), tl.rollup(p, hn, c)):
                a = np.asarray(src, np.uint64)
                C.memmove(dst, a.ctypes.data, 8 * nn)
            return 0
        self.cb = host.TAXA_RUN_FN(_run), host.TAXA_ROLLUP_FN(_rollup)
        host.lib().bh_taxa_set_solver(self.h, C.cast(self.cb[0], C.c_void_p), C.cast(self.cb[1], C.c_void_p), None)

    def sample(self, name, reads, refs, weights, em=None):
        reads = np.asarray(reads, np.uint32)
        pl = np.zeros(len(refs), capi.COV_LINE_DTYPE)
        pl["ref"], pl["st"], pl["ed"], pl["w"] = refs, 1, 50, weights
        em = np.asarray(em, np.uint64) if em is not None else None
        return host.lib().bh_taxa_sample(self.h, None, name.encode(), reads.ctypes.data, pl.ctypes.data, len(pl), em.ctypes.data if em is not None else None)

    def stats(self):
        nc, nn = C.c_uint32(), C.c_uint32()
        host.lib().bh_taxa_dims(self.h, C.byref(nc), C.byref(nn))
        cols = np.zeros((4, nc.value, nn.value), np.uint64)
        assert host.lib().bh_taxa_stats(self.h, cols.ctypes.data) == 0
        return cols

    def write(self):
        nl, nel = C.c_uint32(), C.c_uint32()
        rc = host.lib().bh_taxa_write(self.h, C.byref(nl), C.byref(nel))
        return rc, nl.value, nel.value

    def close(self):
        host.lib().bh_taxa_close(self.h)
        host.lib().bh_tax_free(C.byref(self.tax))


def model_run(parent, hn, gw, lines, agree):
    return tl.taxa(parent, hn, gw, lines, agree)[1:3]


def files_of(tmp_path, prefix):
    return {f[len(prefix):]: open(os.path.join(str(tmp_path), f)).read() for f in sorted(os.listdir(str(tmp_path))) if f.startswith(prefix)}


@pytest.fixture()
def hand_map(tmp_path):
    m = tmp_path / "hand_map.txt"
    m.write_text("".join("h%d\t%s\n" % (i, s) for i, s in enumerate(tc.STRINGS)))
    return str(m)


def test_writer_rows_levels_and_dataset(tmp_path, hand_map):
    """rows in strcmp order of the name, none for a node whose Dataset is zero, level files up to the deepest level with a clade count, the
    abundance level files from the rolled-up counts, a failed sample as a zero column, Dataset = the sum of the sample columns"""
    out = tmp_path / "out"
    out.mkdir()
    prefix = str(out / "st_")
    t = Table(prefix, ["h%d" % i for i in range(6)], hand_map, 1000, model_run)
    uq = [g for g, _ in tc.LINES]
    assert t.sample("/x/y/first.b6", uq, [h for _, h in tc.LINES], [tc.GROUP_W[g] | (0x80000000 if g == 0 else 0) for g in uq], em=[3 << 30, 1 << 29, 0, 0, 1 << 30, 5]) == 0
    assert host.lib().bh_taxa_sample_failed(t.h, b"broken.sample.b6") == 0
    assert t.sample("third", [4, 4, 1], [2, 2, 3], [2, 2, 5]) == 0      # two reads at a;e, five at f: no third level in this sample
    p, hn, g, ln, agree = t.calls[0]
    assert p.tolist() == tc.PARENT and hn.tolist() == tc.HEADER_NODE and agree == 1000 and g.tolist() == tc.GROUP_W[:6]
    assert sorted(zip(ln["group"].tolist(), ln["ref"].tolist())) == sorted(tc.LINES)
    cols = t.stats()
    own1, clade1 = tc.EXPECT[1000][1:3]
    assert cols[0][1].tolist() == own1 and cols[1][1].tolist() == clade1 and not cols[:, 2].any()
    assert cols[0][3].tolist() == [0, 0, 0, 0, 0, 2, 5] and cols[1][3].tolist() == [7, 2, 0, 0, 0, 2, 5]
    assert (cols[:, 0] == cols[:, 1] + cols[:, 2] + cols[:, 3]).all()
    assert cols[3][1].tolist() == [(9 << 29) + 5, (7 << 29) + 5, (7 << 29) + 5, (3 << 30) + 5, 1 << 29, 0, 0] and not cols[2:, 3].any()
    assert t.write() == (0, 3, 3)
    t.close()
    got = files_of(out, "st_")
    assert sorted(got) == ["taxa.txt", "taxa_L1.txt", "taxa_L2.txt", "taxa_L3.txt", "taxa_abundance_L1.txt", "taxa_abundance_L2.txt", "taxa_abundance_L3.txt"]
    H = "#OTU ID\tDataset\tfirst\tbroken.sample\tthird\n"
    assert got["taxa.txt"] == H + "Unassigned\t2\t2\t0\t0\na;b\t2\t2\t0\t0\na;b;c\t4\t4\t0\t0\na;e\t2\t0\t0\t2\nf\t5\t0\t0\t5\n"
    assert got["taxa_L1.txt"] == H + "a\t8\t6\t0\t2\nf\t5\t0\t0\t5\n"
    assert got["taxa_L2.txt"] == H + "a;b\t6\t6\t0\t0\na;e\t2\t0\t0\t2\n"
    assert got["taxa_L3.txt"] == H + "a;b;c\t4\t4\t0\t0\n"
    assert got["taxa_abundance_L1.txt"] == H + "a\t3.5000\t3.5000\t0.0000\t0.0000\nf\t0.0000\t0.0000\t0.0000\t0.0000\n"
    assert got["taxa_abundance_L2.txt"] == H + "a;b\t3.5000\t3.5000\t0.0000\t0.0000\na;e\t0.0000\t0.0000\t0.0000\t0.0000\n"      # (the rows of taxa_L2.txt)
    assert got["taxa_abundance_L3.txt"] == H + "a;b;c\t3.0000\t3.0000\t0.0000\t0.0000\n"      # (a;b;d has no clade count: no row)
    names = ["first", "broken.sample", "third"]
    assert got == tl.tables(tc.NAMES, tc.DEPTH, names, [c.tolist() for c in cols[0][1:]], [c.tolist() for c in cols[1][1:]], [c.tolist() for c in cols[3][1:]])


def test_writer_without_abundance_has_no_abundance_files(tmp_path, hand_map):
    out = tmp_path / "out"
    out.mkdir()
    t = Table(str(out / "n_"), ["h%d" % i for i in range(6)], hand_map, 600)      # (the plain-C solvers)
    uq = [g for g, _ in tc.LINES]
    assert t.sample("s.b6", uq, [h for _, h in tc.LINES], [tc.GROUP_W[g] for g in uq]) == 0
    assert t.write() == (0, 3, 0)
    info = np.zeros(8, np.uint64)
    host.lib().bh_taxa_last_info(t.h, info.ctypes.data)
    assert info[:5].tolist() == tc.EXPECT[600][3]
    t.close()
    own, clade = tc.EXPECT[600][1:3]
    assert files_of(out, "n_") == tl.tables(tc.NAMES, tc.DEPTH, ["s"], [own], [clade])


def test_nothing_written_after_abort_or_solver_error(tmp_path, hand_map):
    out = tmp_path / "out"
    out.mkdir()
    prefix, heads = str(out / "ab_"), ["h%d" % i for i in range(6)]
    t = Table(prefix, heads, hand_map, 1000, model_run)
    assert t.sample("s.b6", [0], [0], [1]) == 0
    host.lib().bh_taxa_abort(t.h)
    assert t.write()[0] == host.E_DEVICE and t.sample("s2.b6", [0], [0], [1]) == host.E_DEVICE
    t.close()
    t = Table(prefix, heads, hand_map, 1000, lambda *a: host.E_DEVICE)
    assert t.sample("s.b6", [0], [0], [1]) == host.E_DEVICE and t.write()[0] == host.E_DEVICE      # (a solver's error is final)
    t.close()
    # without a solver and without a device handle: an error, not a table from somewhere else
    t = Table(prefix, heads, hand_map, 1000, model_run)
    host.lib().bh_taxa_set_solver(t.h, None, None, None)
    assert t.sample("s.b6", [0], [0], [1]) == host.E_DEVICE
    t.close()
    assert os.listdir(str(out)) == []


# ---- the golden .b6 files ----
def golden_tables(tmp_path, b6, agree, em=None):
    """the golden lines through bh_taxa.c with the plain-C solvers: (files, model's groups)"""
    headers, strings, gw, lines, reads = tl.b6_groups(open(os.path.join(GOLDEN, b6)).read(), tl.read_map(open(TAX).read()))
    out = tmp_path / ("g%d" % agree)
    out.mkdir()
    t = Table(str(out / "g_"), headers, TAX, agree)
    assert t.sample("out/golden.b6", [g for g, _ in lines], [h for _, h in lines], [1] * len(lines), em=em) == 0
    assert t.write()[0] == 0
    t.close()
    return files_of(out, "g_"), (headers, strings, gw, lines)


def test_best_golden_equals_the_reference_table(tmp_path):
    """BEST output has one line per read: the own table is the count of column 13, which is what embalmulate writes"""
    ref = {}
    for ln in open(os.path.join(GOLDEN, "taxa", "dna_q100_best_tax_fr_taxa.txt")).read().split("\n")[1:]:
        if "\t" in ln:      # (the row of the empty taxon starts with the tab)
            name, n = ln.split("\t")
            ref[name or "Unassigned"] = int(n)
    assert len(ref) == 41 and sum(ref.values()) == 497 and ref["Unassigned"] == 33
    files, _ = golden_tables(tmp_path, "dna_q100_best_tax_fr.b6", 1000)
    rows = [ln.split("\t") for ln in files["taxa.txt"].splitlines()[1:]]
    assert {(r[0], int(r[1])) for r in rows} == set(ref.items()) and all(r[1] == r[2] for r in rows) and len(rows) == 41


@pytest.mark.parametrize("agree", [1000, 600])
def test_allpaths_golden_equals_the_model(tmp_path, agree):
    files, (headers, strings, gw, lines) = golden_tables(tmp_path, "dna_q100_allpaths_tax_fr.b6", agree)
    names, parent, depth, hn = tl.tree_of(strings)
    # what makes it a test: reads on several headers, whose lowest common ancestors lie at several levels
    cand = {}
    for g, h in lines:
        cand.setdefault(g, set()).add(h)
    lca = [depth[tl.taxon(parent, depth, [hn[h] for h in hs], 1000)] for hs in cand.values() if len(hs) >= 2]
    assert len(lines) == 588 and len(cand) == 497 and {k: lca.count(k) for k in set(lca)} == {0: 18, 6: 30, 4: 2, 7: 20}
    gnode, own, clade, info = tl.taxa(parent, hn, gw, lines, agree)
    assert files == tl.tables(names, depth, ["golden"], [own], [clade]) and "taxa_L7.txt" in files and clade[0] == 497


# ---- the command lines ----
REFUSALS = [
    (["-b", TAX, "-x"], "-x"),
    (["-b", TAX, "-d", "DNA"], "-d"),
    (["-b", TAX, "--make-acx", "x.acx"], "--make-acx"),
    (["-b", TAX, "--gpus", "1", "--shards", "2"], "--shards"),
    (["-b", TAX, "--mates", os.path.join(GOLDEN, "q292.fa")], "mates"),
    (["-b", TAX, "-m", "FORAGE", "--cluster", "C"], "--cluster"),
    (["-b", TAX, "-m", "FORAGE", "--chimeras", "C"], "--chimeras"),
    ([], "-b"),
    (["-b", TAX, "--taxa-agree", "500"], "501 .. 1000"),
    (["-b", TAX, "--taxa-agree", "1001"], "501 .. 1000"),
    (["-b", TAX, "--taxa-agree", "x"], "501 .. 1000"),
]


@pytest.mark.parametrize("extra,word", REFUSALS, ids=[w + str(i) for i, (_, w) in enumerate(REFUSALS)])
@pytest.mark.parametrize("samples", [False, True], ids=["single", "samples"])
def test_refusals_before_a_device_is_touched(tmp_path, extra, word, samples):
    """usage errors, exit code 1, with nothing read, no device opened (this machine may have none) and no file left"""
    out = tmp_path / "o.b6"
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\n")
    base = ["--samples", str(lst)] if samples else ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", str(out)]
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "--taxa", str(tmp_path / "P")] + base + extra, capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 1, r.stdout + r.stderr
    if samples and word in ("--cluster", "--chimeras"):      # (neither goes with --samples at all: that older rule answers first)
        assert "ERROR: " + word in r.stdout, r.stdout
    else:
        assert "ERROR: --" in r.stdout and "taxa" in r.stdout and word in r.stdout, r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["list.txt"]


def test_mates_line_in_a_sample_list_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\tb.fa\n")
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-m", "ALLPATHS", "-fr", "-b", TAX, "--taxa", str(tmp_path / "P"), "--samples", str(lst)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: --taxa" in r.stdout and "mates" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["list.txt"]


@pytest.mark.parametrize("extra,text", [(["--taxa-agree", "800"], "ERROR: --taxa-agree goes with --taxa <prefix>"), (["--taxa"], "--taxa requires an argument")],
                         ids=["agree-alone", "no-prefix"])
@pytest.mark.parametrize("samples", [False, True], ids=["single", "samples"])
def test_option_errors(tmp_path, extra, text, samples):
    """the refusals' own texts: the parser of a build without the flag answers `Unrecognized command-line option` with the same exit code"""
    out = tmp_path / "o.b6"
    lst = tmp_path / "list.txt"
    lst.write_text("a.fa\ta.b6\n")
    base = ["--samples", str(lst)] if samples else ["-q", os.path.join(GOLDEN, "q100.fa"), "-o", str(out)]
    r = subprocess.run([BURST_HIP, "-r", os.path.join(GOLDEN, "quick.edx"), "-b", TAX] + base + extra, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and text in r.stdout and "Unrecognized" not in r.stdout, r.stdout + r.stderr
    assert os.listdir(str(tmp_path)) == ["list.txt"]


def test_launcher_refuses_the_flag():
    r = subprocess.run([sys.executable, "-m", "burst_amd.run", "-r", "x.edx", "-q", "q.fa", "-o", "o.b6", "--taxa", "P"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--taxa is not available" in r.stdout and "burst_hip" in r.stdout


def test_help_names_the_flags():
    r = subprocess.run([BURST_HIP, "-h"], capture_output=True, text=True)
    assert "--taxa <prefix>" in r.stdout and "--taxa-agree" in r.stdout


def test_host_file_under_sanitizers(tmp_path, hand_map):
    """csrc/host/bh_taxa.c as a stand-alone program (tests/csrc/taxa_host_main.c), built with the address and the undefined-behaviour
    sanitizer: the tree builder, the hand case, the refusals, the roll-up, the tables with a failed sample"""
    exe, prefix = str(tmp_path / "taxa_host_main"), str(tmp_path / "t_")
    m = tmp_path / "m.txt"
    m.write_text("h0\ta;b;c\nh1\ta;b;d;\nh2\ta;e\nh3\tf\nh4\tUnassigned\nh5\ta;b;c\n")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(CSRC, "host"),
                           os.path.join(ROOT, "tests", "csrc", "taxa_host_main.c"), os.path.join(CSRC, "host", "bh_taxa.c"), os.path.join(CSRC, "host", "bh_tax.c"),
                           os.path.join(CSRC, "host", "bh_tables.c"), "-o", exe])
    r = subprocess.run([exe, str(m), prefix], capture_output=True, text=True)      # (the sanitizers' runtimes are linked into the program)
    assert r.returncode == 0 and "taxa_host_main ok" in r.stdout, r.stdout + r.stderr
    H = "#OTU ID\tDataset\tone\ttwo\tthree\n"
    assert open(prefix + "taxa.txt").read() == H + "Unassigned\t2\t2\t0\t0\na;b\t2\t2\t0\t0\na;b;c\t6\t4\t0\t2\n"
    assert open(prefix + "taxa_L1.txt").read() == H + "a\t8\t6\t0\t2\n"
    assert open(prefix + "taxa_abundance_L3.txt").read() == H + "a;b;c\t3.0000\t3.0000\t0.0000\t0.0000\n"


def test_exports():
    assert "bhip_taxa_run" in capi.EXPORTS and "bhip_taxa_rollup" in capi.EXPORTS and capi.lib().bhip_abi_version() == 8
