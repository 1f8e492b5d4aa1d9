"""bhip_consensus_pairs against the dictionary model of conspairslib, byte for byte, pairs and info: sample counts on either side of the
tile edge, union lengths across the word boundaries and the wave's word loop, the segment shapes and letters written by hand, every
min_compared, the three budgets (default, several groups, one header in slabs), a relabelling of two samples, both capacities, every
refusal with its text and a good call behind it, and a bhip_consensus_run on the same handle afterwards."""
import numpy as np
import pytest

import conspairscases as cc
import conspairslib as cl
import dbutil
import oraclelib as ol

pytestmark = pytest.mark.gpu

DEFAULT_BUDGET = 1 << 30


@pytest.fixture(scope="module")
def dev():
    from burst_amd import capi
    rng = np.random.default_rng(2)
    packed, clump_len, tot = dbutil.pack_clumps([rng.integers(1, 5, size=200, dtype=np.uint8) for _ in range(4)])
    d = capi.Device(packed, clump_len, tot, ol.score_lut(1), device=0)
    yield d
    d.close()


def same_as_model(dev, case, min_compared=1):
    n, segs, letters = case
    rows = cl.rows_of_segs(segs, letters)
    want = cl.pairs(rows, min_compared)
    got = dev.consensus_pairs(n, segs, letters, min_compared, pair_cap=max(len(want), 1))
    assert got.tobytes() == cl.pairs_array(want).tobytes()
    info = dev.consensus_pairs_info()
    figures = (info["segments"], info["headers"], info["union_positions"], info["examined"], info["pairs"])
    assert figures == cl.info(rows, len(segs), len(want))
    if figures[1]:
        assert info["device_us"] > 0 and info["peak_bytes"] > 0
    return want


@pytest.mark.parametrize("n_samples", [1, 2, 3, 15, 16, 17, 33, 65])
def test_sample_counts_on_one_header(dev, n_samples):
    want = same_as_model(dev, cc.one_header(n_samples, 300, 40 + n_samples))
    if n_samples >= 15:
        assert len(want) > n_samples and any(c != s for _, _, _, c, s in want)


@pytest.mark.parametrize("union", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4160])
def test_union_lengths(dev, union):
    for n_samples, seed in ((2, union), (2, union + 1), (5, union)):      # abutting and overlapping halves; five samples
        same_as_model(dev, cc.one_header(n_samples, union, seed))


@pytest.mark.parametrize("m", [1, 2, 13, 71])
def test_shapes_and_letters_written_by_hand(dev, m):
    want = same_as_model(dev, cc.shapes(), m)
    by = {(h, a, b): (c, s) for h, a, b, c, s in want}
    if m == 1:
        assert by[(3, 0, 1)] == (9, 7) and by[(4, 0, 3)] == (4, 3) and (40, 1, 3) not in by and (40, 2, 3) not in by and (5, 2, 2) not in by
        assert {h for h, _, _ in by} == {3, 4, 40}
    if m == 71:      # above every count
        assert want == []


@pytest.mark.parametrize("seed", range(4))
def test_random_studies(dev, seed):
    want = same_as_model(dev, cc.random_case(seed, n_samples=9 + 10 * seed, n_headers=30))
    assert want


def test_a_segment_longer_than_a_wave_of_words(dev):
    """k_cp_planes gives a segment one wave and a word per lane: 9 000 positions are 141 words, three passes of the lanes"""
    case = cc.long_segment()
    assert max(int(g["len"]) for g in case[1]) == 9000
    want = same_as_model(dev, case)
    by = {(h, a, b): (c, s) for h, a, b, c, s in want}
    # (sample 1's 4 160 positions from 5 000 lie on words 62 .. 127 of the axis, its last 60 on word 140: most of what is compared is
    # behind the first pass of the lanes)
    assert by[(9, 0, 1)][0] > 2000 and by[(9, 0, 1)][0] > by[(9, 0, 1)][1] > 0 and (10, 0, 2) in by


@pytest.mark.parametrize("budget", [DEFAULT_BUDGET, 3 * 24 * 300, 3 * 24 * 100, 3 * 24 * 256], ids=["default", "slabs of 300 words", "slabs of 100 words", "slabs of 256 words"])
def test_a_header_wider_than_a_workgroups_words(dev, budget):
    """40 000 positions are 625 words: k_cp_pairs splits them over three workgroups per tile, which add into one cell; in slabs wider
    than, narrower than and equal to the 256 words of a workgroup as well"""
    case = cc.wide_header()
    try:
        dev.set_option("conspairs_bytes", budget)
        want = same_as_model(dev, case)
    finally:
        dev.set_option("conspairs_bytes", DEFAULT_BUDGET)
    by = {(h, a, b): (c, s) for h, a, b, c, s in want}
    assert dev.consensus_pairs_info()["union_positions"] == 40000 + 287 + 193
    assert by[(7, 0, 2)][0] > 20000 and by[(7, 0, 1)][0] > by[(7, 0, 1)][1] > 0 and {(2, 0, 1), (8, 1, 2)} <= set(by)


def test_the_budget_changes_no_byte(dev):
    case = cc.random_case(11, n_samples=20, n_headers=25, max_len=3000)
    n, segs, letters = case
    rows = cl.rows_of_segs(segs, letters)
    want = cl.pairs_array(cl.pairs(rows)).tobytes()
    by_header = {}
    for (s, h), row in rows.items():
        by_header.setdefault(h, []).append(row)
    need = {h: 24 * len(r) * ((len(set().union(*map(set, r))) + 63) // 64) for h, r in by_header.items() if len(r) >= 2}      # plane bytes of a header
    largest = max(need.values())
    assert largest * 3 < sum(need.values()) and largest > 24 * 20 * 4
    try:
        outs = []
        for budget in (DEFAULT_BUDGET, largest, 24 * 20 * 3, 1):      # one group; several groups; the large headers in slabs of three words; of one word
            dev.set_option("conspairs_bytes", budget)
            outs.append(dev.consensus_pairs(n, segs, letters, 1, pair_cap=1 << 16).tobytes())
            info = dev.consensus_pairs_info()
            assert (info["segments"], info["headers"], info["examined"]) == (len(segs), len(need), sum(len(r) * (len(r) - 1) // 2 for r in by_header.values()))
    finally:
        dev.set_option("conspairs_bytes", DEFAULT_BUDGET)
    assert all(o == want for o in outs)
    from burst_amd import capi
    with pytest.raises(capi.BurstHipError):
        dev.set_option("conspairs_bytes", 0)


def test_relabelling_two_samples(dev):
    case = cc.random_case(5, n_samples=18, n_headers=10)
    a = same_as_model(dev, case)
    b = same_as_model(dev, cc.relabel(case, 2, 17))
    swap = lambda s: 17 if s == 2 else 2 if s == 17 else s
    assert sorted((h, min(swap(x), swap(y)), max(swap(x), swap(y)), c, s) for h, x, y, c, s in a) == b


def test_both_capacities_and_nothing_to_pair(dev):
    from burst_amd import capi
    n, segs, letters = case = cc.random_case(3)
    want = same_as_model(dev, case)
    with pytest.raises(capi.BurstHipError) as e:
        dev.consensus_pairs(n, segs, letters, 1, pair_cap=len(want) - 1, retry=False)
    assert e.value.code == capi.BHIP_E_CAPACITY and dev.pairs_wanted == len(want) and not dev.pairs_buffer.tobytes().strip(b"\0")      # nothing is written
    assert dev.consensus_pairs(n, segs, letters, 1, pair_cap=len(want), retry=False).tobytes() == cl.pairs_array(want).tobytes()      # the handle stays usable
    assert dev.consensus_pairs(n, segs, letters, 1, pair_cap=0).tobytes() == cl.pairs_array(want).tobytes()      # (asked again with the number wanted)
    for n_samples in (0, 1):
        few = segs[segs["sample"] < n_samples]
        assert len(dev.consensus_pairs(n_samples, few, letters)) == 0
        info = dev.consensus_pairs_info()
        assert (info["segments"], info["headers"], info["union_positions"], info["examined"], info["pairs"], info["device_us"]) == (len(few), 0, 0, 0, 0, 0)
    assert len(dev.consensus_pairs(5, None, b"")) == 0 and dev.consensus_pairs_info()["segments"] == 0


@pytest.mark.parametrize("what,n_samples,rows,letters,m,text", cc.bad_arguments(), ids=[b[0] for b in cc.bad_arguments()])
def test_refusals_leave_the_handle_usable(dev, what, n_samples, rows, letters, m, text):
    from burst_amd import capi
    with pytest.raises(capi.BurstHipError) as e:
        dev.consensus_pairs(n_samples, cc.seg_rows(rows), letters, m)
    assert e.value.code == capi.BHIP_E_ARG and text in str(e.value)
    same_as_model(dev, cc.shapes())


def test_a_consensus_run_on_the_same_handle_afterwards(tmp_path_factory):
    """two samples' bhip_consensus_run segments go into the pairs as they come back; a bhip_consensus_run on the same handle behind the pairs
    still gives its own model's bytes"""
    import cigarlib as cg
    import test_gpu_consensus as tg
    from burst_amd import capi
    pool = tg.Pool(cg.restate(tmp_path_factory.mktemp("cigar")), 1)
    try:
        idx = list(range(len(pool.cases)))
        spec_segs, letters = [], b""
        for sample, part in enumerate((idx[0::2], idx[1::2], idx)):
            segs, let = pool.check(part)
            for g in segs:
                spec_segs.append((sample, int(g["header"]), int(g["pos"]), int(g["len"]), len(letters) + int(g["off"])))
            letters += let.encode()
        segs = cc.seg_rows(spec_segs)
        want = same_as_model(pool.dev, (3, segs, letters))
        assert want and all(c >= s > 0 for _, _, _, c, s in want)
        pool.check(idx)
        pool.check(idx[0::3], 2)
        assert pool.dev.consensus_pairs_info()["pairs"] == len(want)
    finally:
        pool.dev.close()
