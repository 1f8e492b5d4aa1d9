"""bhip_cluster_run on the MI355X against bh_cluster_host (the definition in plain sequential C, itself checked against the Python model in
tests/test_cluster_cpu.py): exact array equality on the smallest shapes at which each step can go wrong (tests/clustercases.py)."""
import numpy as np
import pytest

import clustercases as cc

pytestmark = pytest.mark.gpu
_dev = {}


def small_device():
    """a handle on a small database: the clustering call needs a handle, not its references"""
    if "d" not in _dev:
        import dbutil
        import oraclelib as ol
        from burst_amd import capi
        rng = np.random.default_rng(5)
        seqs = [rng.integers(1, 5, size=int(n), dtype=np.uint8) for n in rng.integers(90, 400, size=40)]
        packed, clump_len, tot = dbutil.pack_clumps(seqs)
        _dev["d"] = capi.Device(packed, clump_len, tot, ol.score_lut(1))
    return _dev["d"]


_want = {}


def yardstick(name, case):
    """bh_cluster_host's answer, computed once per case"""
    from burst_amd import host
    if name not in _want:
        _want[name] = host.cluster_host(*case)
    return _want[name]


def check(name, case, dev=None):
    dev = dev or small_device()
    weights, edges = case
    centroid, edits = dev.cluster_run(weights, edges)
    info = dev.cluster_info()
    want_c, want_e, want_info = yardstick(name, case)
    print("%s: rounds %d, edges kept %d, centroids %d, device %d us" % (name, info["rounds"], info["edges_kept"], info["centroids"], info["device_us"]))
    assert centroid.dtype == np.uint32 and edits.dtype == np.uint32
    assert np.array_equal(centroid, want_c) and np.array_equal(edits, want_e)
    assert (info["edges_kept"], info["centroids"], info["edges"], info["nodes"]) == tuple(int(want_info[k]) for k in (1, 2, 5, 6))
    return centroid, edits, info


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case(name):
    _, _, info = check(name, cc.CASES[name])
    if not cc.CASES[name][1]:
        assert info["rounds"] == 0 and info["device_us"] == 0      # no edges: nothing is launched


def test_chain_takes_a_round_per_node():
    """i -> i - 1: roles alternate and node i waits for node i - 1; the rounds are counted, not capped"""
    centroid, _, info = check("chain300", cc.CASES["chain300"])
    assert centroid[:6].tolist() == [0, 0, 2, 2, 4, 4]
    assert 150 <= info["rounds"] <= 300
    centroid, _, info = check("chain300_reversed", cc.CASES["chain300_reversed"])
    assert centroid[-4:].tolist() == [297, 297, 299, 299]
    assert 150 <= info["rounds"] <= 300


@pytest.mark.parametrize("deg", [63, 64, 65, 1000])
def test_star_roles(deg):
    """the run of node 0 is walked by a thread below 64 targets and by a wave from 64 on: the only centroid last, first, absent"""
    assert check("star%d_last" % deg, cc.CASES["star%d_last" % deg])[0][0] == deg + 1
    assert check("star%d_first" % deg, cc.CASES["star%d_first" % deg])[0][0] == 2
    c, e, info = check("star%d_absent" % deg, cc.CASES["star%d_absent" % deg])
    assert c[0] == 0 and e[0] == 0 and info["edges_kept"] == 2 * deg


@pytest.mark.parametrize("seed", cc.RANDOM_SEEDS)
def test_random_graph(seed):
    centroid, _, info = check("random%d" % seed, cc.random_graph(seed))
    assert 1 < info["centroids"] < 2000 and info["centroids"] == int((centroid == np.arange(2000)).sum())
    assert info["edges"] == 20000 and info["edges_kept"] < 18000      # self edges, edges towards lower priority and duplicates are gone


def test_smaller_then_larger_on_one_handle():
    """grow-only buffers and stale state: a large input, a small one, a larger one, and the first again"""
    big, small, bigger = cc.random_graph(1), cc.CASES["weight_ties_by_number"], cc.random_graph(4, n=3000, m=40000)
    check("random1", big)
    check("weight_ties_by_number", small)
    check("random4_3000", bigger)
    check("no_edges", cc.CASES["no_edges"])
    check("random1", big)


def test_node_out_of_range_is_refused_without_a_launch():
    from burst_amd import capi
    dev = small_device()
    check("directed", cc.CASES["directed"])
    before = dev.cluster_info()
    for bad in ([(0, 3, 0)], [(3, 0, 0)], [(0, 1, 0), (1, 2, 0), (2, 3, 1)]):
        with pytest.raises(capi.BurstHipError) as ei:
            dev.cluster_run([1, 1, 1], bad)
        assert ei.value.code == capi.BHIP_E_ARG and "names node" in str(ei.value)
    assert dev.cluster_info() == before      # (nothing ran: the figures are the last call's)
    check("directed", cc.CASES["directed"])      # the handle stays usable
