"""bhip_taxa_run and bhip_taxa_rollup on the MI355X against the Python model (tests/taxalib.py): bit-equal group_node, own, clade and
info[0..4] on the hand case, random trees, one shape either side of the thread / wave split, a window that spans two subtrees, a chain of
64 levels, everything at the root, and every refusal."""
import numpy as np
import pytest

import taxacases as tc
import taxalib as tl

pytestmark = pytest.mark.gpu
_dev = {}


def small_device():
    """a handle on a small database: the call needs a handle, not its references"""
    if "d" not in _dev:
        import dbutil
        import oraclelib as ol
        from burst_amd import capi
        rng = np.random.default_rng(5)
        seqs = [rng.integers(1, 5, size=int(n), dtype=np.uint8) for n in rng.integers(90, 400, size=40)]
        packed, clump_len, tot = dbutil.pack_clumps(seqs)
        _dev["d"] = capi.Device(packed, clump_len, tot, ol.score_lut(1))
    return _dev["d"]


def check(parent, header_node, gw, lines, agree, want=None):
    """the device on one input against the model (or the answer written out before)"""
    gn, own, clade, info = small_device().taxa_run(parent, header_node, gw, lines, agree)
    print("pairs %d, groups %d, reads %d, at the root %d, deepest %d, device %d us, peak %d bytes" % tuple(int(x) for x in info[:7]))
    want = want if want is not None else tl.taxa(parent, header_node, gw, lines, agree)
    assert (gn.tolist(), own.tolist(), clade.tolist(), info[:5].tolist()) == tuple(want) and int(info[7]) == 0
    return want


@pytest.mark.parametrize("agree", sorted(tc.EXPECT))
def test_hand_case(agree):
    check(tc.PARENT, tc.HEADER_NODE, tc.GROUP_W, tc.LINES, agree, tc.EXPECT[agree])


@pytest.mark.parametrize("agree", [501, 667, 750, 1000])
def test_random_trees(agree):
    for seed, n_nodes in ((1, 200), (2, 60), (3, 9)):
        raw, hraw, gw, lines = tl.random_case(seed, n_nodes=n_nodes)
        for rev in (False, True):
            parent, new = tl.preorder(raw, reverse=rev)
            check(parent, [new[v] for v in hraw], gw, lines, agree)


def family_tree(n_leaves, fan=7):
    """root -> two halves -> `fan` families each -> leaves: leaf k is under half k % 2, family (k // 2) % fan.  Returns (parent, the leaves'
    nodes) in a numbering that is no preorder yet (taxalib.preorder)"""
    parent, leaves = [0], [0] * n_leaves
    for half in range(2):
        parent.append(0)
        h = len(parent) - 1
        fams = []
        for _ in range(fan):
            parent.append(h)
            fams.append(len(parent) - 1)
        for k in range(half, n_leaves, 2):
            parent.append(fams[(k // 2) % fan])
            leaves[k] = len(parent) - 1
    return parent, leaves


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("agree", [501, 750, 1000])
def test_candidate_counts_either_side_of_the_split(n, agree):
    """groups of exactly n candidates (a thread takes up to 64, a wave the longer ones) beside groups of one, inside one family, one half
    and across both halves; some lines twice"""
    raw, leaves = family_tree(140)
    parent, new = tl.preorder(raw)
    hn = [new[v] for v in leaves] + [0]
    rng = np.random.default_rng(n)
    gw, lines = [], []
    for g in range(12):
        gw.append(g % 4)
        pool = {0: np.arange(0, 140, 2), 1: np.arange(140)}[g % 2]      # (even headers: one half; all: both halves)
        if g >= 8:
            pool = np.arange(0, 140, 14)[:max(n, 1)] if n <= 10 else pool      # (one family while it has enough leaves)
        k = min(n, len(pool)) if g != 11 else 1
        lines += [(g, int(h)) for h in rng.choice(pool, size=k, replace=False)]
    lines += [lines[int(i)] for i in rng.choice(len(lines), size=len(lines) // 4, replace=False)]
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    check(parent, hn, gw, lines, agree)


def test_window_spans_two_subtrees():
    """one group of 5000 candidates, 2400 under one half and 2600 under the other: at 501 .. 520 permille the larger half holds enough of
    them, at 521 and above only the root does -- and a window of t neighbours then always spans both halves"""
    parent = [0, 0] + [1] * 2400 + [0] + [2402] * 2600
    assert tl.is_preorder(parent)
    hn = list(range(2, 2402)) + list(range(2403, 5003))
    rng = np.random.default_rng(3)
    lines = [(1, int(h)) for h in rng.permutation(5000)] + [(0, 7), (2, 4000), (2, 4001)]
    for agree, node in ((501, 2402), (520, 2402), (521, 0), (1000, 0)):
        gn, own, clade, info = check(parent, hn, [1, 6, 2], lines, agree)
        assert gn == [9, node, 2402] and own[node] >= 6 and info[:3] == [5003, 3, 9]


def test_chain_of_64_levels():
    parent = [0] + list(range(64))
    hn = list(range(65))
    lines = [(0, 64), (1, 64), (1, 10), (2, 30), (2, 31), (2, 64), (3, 0), (3, 64)]
    want = check(parent, hn, [1, 2, 3, 4], lines, 1000)
    assert want[0] == [64, 10, 30, 0] and want[3][4] == 64
    assert check(parent, hn, [1, 2, 3, 4], lines, 600)[0] == [64, 10, 31, 0]
    with pytest.raises(Exception, match="64|levels"):
        small_device().taxa_run([0] + list(range(65)), [0], [1], [(0, 0)])


def test_all_headers_at_the_root_and_no_lines():
    want = check(tc.PARENT, [0] * 6, tc.GROUP_W, tc.LINES, 750)
    assert want[1] == [8, 0, 0, 0, 0, 0, 0] and want[3] == [12, 6, 8, 8, 0]
    want = check(tc.PARENT, tc.HEADER_NODE, tc.GROUP_W, [], 1000)
    assert want[0] == [tl.NONE] * 7 and want[3] == [0] * 5
    check([0], [0, 0], [5], [(0, 1), (0, 0)], 1000, ([0], [5], [5], [2, 1, 5, 5, 0]))      # a tree of the root alone


def test_refusals_leave_the_handle_usable():
    from burst_amd import capi
    d = small_device()
    P, H, W, L = tc.PARENT, tc.HEADER_NODE, tc.GROUP_W, tc.LINES
    bad = [([1, 0], [0], W, L, 1000),                  # parent[0] != 0
           ([0, 0, 2], [0] * 6, W, L, 1000),           # parent[v] >= v
           ([0, 0, 0, 1], [0] * 6, W, L, 1000),        # not a preorder numbering
           ([0] + list(range(65)), [0] * 6, W, L, 1000),      # 65 levels
           (P, [7] + H[1:], W, L, 1000),               # a header's node beyond the tree
           (P, H, W, L + [(0, 6)], 1000),              # a line's header beyond the table
           (P, H, W, L + [(7, 0)], 1000),              # a line's group beyond the table
           (P, H, W, L, 500), (P, H, W, L, 1001)]
    for args in bad:
        with pytest.raises(capi.BurstHipError) as e:
            d.taxa_run(*args)
        assert e.value.code == capi.BHIP_E_ARG, str(e.value)
        check(P, H, W, L, 1000, tc.EXPECT[1000])
    lines = capi.em_lines(L)
    p, h, w = (np.asarray(x, np.uint32) for x in (P, H, W))
    own, clade = np.zeros(7, np.uint64), np.zeros(7, np.uint64)
    rc = capi.lib().bhip_taxa_run(d._h, 7, capi._ptr(p), 6, capi._ptr(h), 7, capi._ptr(w), capi._ptr(lines), 1 << 31, 1000, None, capi._ptr(own), capi._ptr(clade), None)
    assert rc == capi.BHIP_E_ARG
    with pytest.raises(capi.BurstHipError):
        d.taxa_rollup([0, 0, 0, 1], [0], [1])
    check(P, H, W, L, 667, tc.EXPECT[667])


def test_rollup_against_the_model():
    d = small_device()
    rng = np.random.default_rng(11)
    for seed, n_nodes in ((1, 200), (3, 9)):
        raw, hraw, _, _ = tl.random_case(seed, n_nodes=n_nodes)
        parent, new = tl.preorder(raw)
        hn = [new[v] for v in hraw]
        counts = [int(x) for x in rng.integers((1 << 62) - (1 << 20), 1 << 62, size=len(hn), dtype=np.uint64)]
        counts[::7] = [0] * len(counts[::7])
        own, clade = d.taxa_rollup(parent, hn, counts)
        assert (own.tolist(), clade.tolist()) == tl.rollup(parent, hn, counts)
    own, clade = d.taxa_rollup(tc.PARENT, tc.HEADER_NODE, [5, 7, 11, 13, 17, 1 << 62])
    assert own.tolist() == [17, 0, 0, (1 << 62) + 5, 7, 11, 13] and clade.tolist() == [(1 << 62) + 53, (1 << 62) + 23, (1 << 62) + 12, (1 << 62) + 5, 7, 11, 13]
