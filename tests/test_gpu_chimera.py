"""bhip_chimera_run on the MI355X against bh_chimera_host (the definition in plain sequential C, itself checked against the Python model in
tests/test_chimera_cpu.py): exact array equality on the smallest shapes at which each step can go wrong (tests/chimeracases.py)."""
import numpy as np
import pytest

import chimeracases as cc

pytestmark = pytest.mark.gpu
_dev = {}


def small_device():
    """a handle on a small database: the chimera call needs a handle, not its references"""
    if "d" not in _dev:
        import dbutil
        import oraclelib as ol
        from burst_amd import capi
        rng = np.random.default_rng(5)
        seqs = [rng.integers(1, 5, size=int(n), dtype=np.uint8) for n in rng.integers(90, 400, size=40)]
        packed, clump_len, tot = dbutil.pack_clumps(seqs)
        _dev["d"] = capi.Device(packed, clump_len, tot, ol.score_lut(1))
    return _dev["d"]


@pytest.fixture(scope="module", autouse=True)
def _close_device():
    """the module's handle goes with the module: the tests that follow in the same process find no streams or buffers of this one"""
    yield
    d = _dev.pop("d", None)
    if d is not None:
        d.close()


_want = {}


def yardstick(name, case):
    """bh_chimera_host's answer, computed once per case"""
    from burst_amd import host
    if name not in _want:
        w, lens, lines, ops, par = case
        _want[name] = host.chimera_host(w, lens, lines, ops, **par)
    return _want[name]


def check(name, case, dev=None):
    dev = dev or small_device()
    w, lens, lines, ops, par = case
    rows = dev.chimera_run(w, lens, lines, ops, **par)
    info = dev.chimera_info()
    want, want_info = yardstick(name, case)
    print("%s: pairs kept %d, evaluated %d, chimeric %d, device %d us" % (name, info["pairs_kept"], info["evaluated"], info["chimeric"], info["device_us"]))
    assert rows.dtype == want.dtype and np.array_equal(rows, want)
    assert (info["pairs_kept"], info["evaluated"], info["chimeric"], info["lines"], info["nodes"]) == tuple(int(want_info[k]) for k in (0, 1, 2, 5, 6))
    return rows, info


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case(name):
    rows, info = check(name, cc.CASES[name])
    if not cc.CASES[name][2]:
        assert info["device_us"] == 0 and not rows["role"].any()      # no lines: nothing is launched


def test_hand_values():
    """a few rows spelled out (the rest in tests/test_chimera_cpu.py): role, single, model, cut, a, ea, b, eb of read 0"""
    assert check("baseline_reverse", cc.CASES["baseline_reverse"])[0][0].tolist() == (2, 3, 0, 16, 1, 0, 2, 0)
    assert check("d_at_the_cut_reverse", cc.CASES["d_at_the_cut_reverse"])[0][0].tolist() == (2, 1, 0, 16, 2, 0, 1, 0)
    assert check("edits254", cc.CASES["edits254"])[0][0].tolist() == (2, 254, 0, 254, 2, 0, 1, 0)
    assert check("len_4095", cc.CASES["len_4095"])[0][0].tolist()[:3] == (2, 3, 0)
    assert check("wide_product", cc.CASES["wide_product"])[0]["role"].tolist() == [2, 0, 0, 0]


@pytest.mark.parametrize("seed", cc.RANDOM_SEEDS)
def test_random_case(seed):
    rows, info = check("random%d" % seed, cc.random_case(seed))
    assert 0 < info["chimeric"] < info["evaluated"] < 2000
    assert info["lines"] == 20000 and info["pairs_kept"] < 20000      # self lines, lines towards non-candidates and repeated (q, r) are gone


@pytest.mark.parametrize("name", ["lines_65", "lines_1500", "skew_edge"])
def test_permuted_lines(name):
    """no repeated (q, r) in these: the output does not depend on the order the lines are given in"""
    w, lens, lines, ops, par = cc.CASES[name]
    assert len(set((q, r) for q, r, _, _, _ in lines)) == len(lines)
    perm = np.random.default_rng(3).permutation(len(lines))
    check(name, (w, lens, [lines[i] for i in perm], ops, par))


def test_larger_then_smaller_on_one_handle():
    """grow-only scratch buffers and stale contents: a large input, a small one, a larger one, none at all, and the first again"""
    check("random1", cc.random_case(1))
    check("five_times", cc.CASES["five_times"])
    check("random4_3000", cc.random_case(4, n=3000, lines=40000))
    check("no_lines", cc.CASES["no_lines"])
    check("random1", cc.random_case(1))


def test_bad_arguments_are_refused_without_a_launch():
    from burst_amd import capi
    dev = small_device()
    check("baseline", cc.CASES["baseline"])
    before = dev.chimera_info()
    w, lens, eq8 = [1, 2, 2], [8, 8, 8], [8 << 4 | 7]
    for lines, ops, par, word in (([(0, 3, 0, 1, 0)], eq8, {}, "names node"), ([(0, 1, 0, 2, 0)], eq8, {}, "leave"), ([(0, 1, 0, 1, 0)], [8 << 4 | 3], {}, "no run of"),
                                  ([(0, 1, 0, 1, 0)], [7 << 4 | 7], {}, "consume"), ([(0, 1, 0, 2, 0)], eq8 + [255 << 4 | 2], {}, "edits"),
                                  ([(0, 1, 0, 1, 0)], eq8, {"min_seg": 0}, "at least 1")):
        with pytest.raises(capi.BurstHipError) as ei:
            dev.chimera_run(w, lens, lines, ops, **par)
        assert ei.value.code == capi.BHIP_E_ARG and word in str(ei.value)
    with pytest.raises(capi.BurstHipError, match="symbols"):
        dev.chimera_run(w, [4096, 8, 8], [(0, 1, 0, 1, 0)], [4096 << 4 | 7])
    assert dev.chimera_info() == before      # (nothing ran: the figures are the last call's)
    check("baseline", cc.CASES["baseline"])      # the handle stays usable
