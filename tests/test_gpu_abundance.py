"""bhip_em_run on the MI355X against the Python model (tests/emlib.py): bit-equal counts and info[0..4] on the hand cases of the
definition, the random case, one shape per kernel path and per threshold between two paths, the weak hash, and the errors."""
import ctypes as C

import numpy as np
import pytest

import emlib as em

pytestmark = pytest.mark.gpu
ONE = em.ONE
_dev = {}


def small_device():
    """a handle on a small database: the abundance call needs a handle, not its references"""
    if "d" not in _dev:
        import dbutil
        import oraclelib as ol
        from burst_amd import capi
        rng = np.random.default_rng(5)
        seqs = [rng.integers(1, 5, size=int(n), dtype=np.uint8) for n in rng.integers(90, 400, size=40)]
        packed, clump_len, tot = dbutil.pack_clumps(seqs)
        _dev["d"] = capi.Device(packed, clump_len, tot, ol.score_lut(1))
    return _dev["d"]


def check(case, max_iters, tol, want=None, classes_at_least=False):
    """the device on one input against the model (or the model's answer computed before)"""
    nh, gw, ln = case
    counts, info = small_device().em_run(nh, gw, ln, max_iters, tol)
    wc, wi = want if want is not None else em.em(nh, gw, ln, max_iters, tol)
    print("iterations %d, pairs %d, classes %d, delta %d, converged %d, device %d us, peak %d bytes" % tuple(int(x) for x in info[:7]))
    assert [int(x) for x in counts] == wc
    got = [int(x) for x in info[:5]]
    if classes_at_least:
        assert got[2] >= wi[2]
        got[2] = wi[2]
    assert got == wi and int(info[7]) == 0
    return counts, info


@pytest.mark.parametrize("max_iters,tol,counts,info", [
    (1, 0, [5368709120, 3221225472, 0], [1, 12, 3, 4294967296, 0]),
    (2, 0, [5905580032, 2684354560, 0], [2, 12, 3, 536870912, 0]),
    (3, 0, [6174015488, 2415919104, 0], [3, 12, 3, 268435456, 0]),
    (1000, 1024, [6442449920, 2147484672, 0], [21, 12, 3, 1024, 1]),
    (1000, 0, [6442450944, 2147483648, 0], [31, 12, 3, 0, 1]),
], ids=["t1", "t2", "t3", "tol1024", "tol0"])
def test_hand_case_1(max_iters, tol, counts, info):
    check(em.CASE1, max_iters, tol, (counts, info))


def test_hand_cases_2_3_4():
    check(em.CASE2, 1000, 1024, ([357913942, 357913941, 357913941], [2, 3, 1, 0, 1]))
    check(em.CASE3, 1000, 1024, ([0, 1789569710, 1789569705, 1789569705], [2, 3, 1, 0, 1]))
    check(em.CASE4, 1000, 1024, ([ONE, ONE], [1, 2, 2, 0, 1]))


@pytest.fixture(scope="module")
def random_case():
    """the model run once to its fixed point; the answer for (max_iters, tol) is read off its trace"""
    case = em.random_case(1)
    trace = []
    _, info = em.em(*case, max_iters=100000, tol=0, trace=trace)
    assert trace[-1][2] == 0 and len(trace) < 1000

    def answer(max_iters, tol):
        t = min(next(t for t, _, d in trace if d <= tol), max_iters)
        return trace[t - 1][1], [t, info[1], info[2], trace[t - 1][2], int(trace[t - 1][2] <= tol)]
    return case, answer


SETTINGS = [(1, 0), (7, 0), (1000, 1024), (100000, 0)]


@pytest.mark.parametrize("max_iters,tol", SETTINGS)
def test_random_case(random_case, max_iters, tol):
    case, answer = random_case
    check(case, max_iters, tol, answer(max_iters, tol))


@pytest.mark.parametrize("max_iters,tol", SETTINGS)
def test_weak_hash_changes_no_count(random_case, max_iters, tol):
    """with a 2-bit hash the element-by-element comparison decides which groups merge: the same counts and iterations; the classes may be
    more than the distinct sets (equal sets that are no neighbours stay apart), never fewer -- and without the option they are equal"""
    case, answer = random_case
    dev = small_device()
    dev.set_option("em_weak_hash", 1)
    try:
        _, info = check(case, max_iters, tol, answer(max_iters, tol), classes_at_least=True)
    finally:
        dev.set_option("em_weak_hash", 0)
    check(case, max_iters, tol, answer(max_iters, tol))


def big_set_case(size, n_headers, seed):
    """one group of `size` candidates (2 reads) beside single-candidate groups on the same headers, a second group with the same set, and a
    few small sets; some headers on no line"""
    rng = np.random.default_rng(seed)
    big = sorted(int(x) for x in rng.choice(n_headers - 3, size=size, replace=False))
    gw, lines = [2, 1], [(0, h) for h in big] + [(1, h) for h in reversed(big)]
    for k in range(40):      # single-candidate groups on the big set's headers: their counts differ, the shares are not all equal
        gw.append(1 + k % 3)
        lines.append((len(gw) - 1, big[(k * 7) % size]))
    for k in range(6):
        gw.append(1)
        lines += [(len(gw) - 1, big[k]), (len(gw) - 1, big[size - 1 - k])]
    order = rng.permutation(len(lines))
    return n_headers, gw, [lines[int(i)] for i in order]


@pytest.mark.parametrize("size,n_headers,opts", [
    (65, 80, {}),                              # one past a wave: the wave kernel's lanes stride twice
    (1100, 1200, {}),                          # past a block: the block kernel, four rounds of its 256 threads and a part of a fifth
    (1100, 1200, {"em_wave_max": 4096}),       # ... and the same set through the wave kernel: eighteen strides
    (9, 12, {}),                               # a thread walks nine candidates
    (9, 12, {"em_thread_max": 1}),             # ... and a wave with nine lanes at work
    (40, 60, {"em_thread_max": 64}),           # a thread's long walk
], ids=["65", "1100", "1100-wave", "9", "9-wave", "40-thread"])
def test_one_shape_per_kernel_path(size, n_headers, opts):
    case = big_set_case(size, n_headers, size)
    dev = small_device()
    for k, v in opts.items():
        dev.set_option(k, v)
    try:
        for max_iters, tol in ((1, 0), (9, 0), (1000, 1024)):
            check(case, max_iters, tol)      # (the classes too: the big set, listed twice, is one)
    finally:
        for k in opts:
            dev.set_option(k, 0)


def test_sizes_at_the_thresholds():
    """sets of 2, 16 | 17, 64 | 65, 1024 | 1025 candidates in one input: the last set a thread takes and the first a wave takes, a full wave and
    one more, the last set a wave takes and the first a block takes"""
    nh = 1100
    rng = np.random.default_rng(11)
    gw, lines = [], []
    for size in (2, 16, 17, 64, 65, 1024, 1025, 1, 1, 1):
        gw.append(int(rng.integers(1, 4)))
        lines += [(len(gw) - 1, int(h)) for h in rng.choice(nh - 10, size=size, replace=False)]
    case = (nh, gw, lines)
    for max_iters, tol in ((1, 0), (6, 0), (1000, 1024)):
        check(case, max_iters, tol)


def test_errors_leave_the_handle_usable():
    from burst_amd import capi
    dev = small_device()
    nh, gw, ln = em.CASE4
    good = ([ONE, ONE], [1, 2, 2, 0, 1])
    bad = [
        (dict(n_headers=nh, group_w=gw, lines=[(0, 0), (1, 2)]), "header"),
        (dict(n_headers=nh, group_w=gw, lines=[(0, 0), (2, 1)]), "group"),
        (dict(n_headers=nh, group_w=[0x7FFFFFFF, 1], lines=ln), "2^31 - 1"),
        (dict(n_headers=nh, group_w=gw, lines=ln, max_iters=0), "max_iters"),
    ]
    for kw, word in bad:
        with pytest.raises(capi.BurstHipError) as e:
            dev.em_run(**kw)
        assert e.value.code == capi.BHIP_E_ARG and word in str(e.value), str(e.value)
        check(em.CASE4, 1000, 1024, good)
    # n_lines >= 2^31 is refused before a line is read
    lines, gwa = capi.em_lines(ln), np.asarray(gw, np.uint32)
    counts, info = np.full(nh, 7, np.uint64), np.full(8, 7, np.uint64)
    rc = capi.lib().bhip_em_run(dev._h, nh, 2, gwa.ctypes.data_as(C.c_void_p), lines.ctypes.data_as(C.c_void_p), 1 << 31, 10, 0,
                                counts.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    assert rc == capi.BHIP_E_ARG and b"2^31 - 1" in capi.lib().bhip_last_error()
    check(em.CASE4, 1000, 1024, good)
    # the summed weight of the groups that take part is what is bounded: 2^31 - 1 is taken, a group of 2^31 reads without a line is not there
    c, _ = dev.em_run(nh, [0x7FFFFFFE, 1, 0x80000000], ln)
    assert [int(x) for x in c] == [0x7FFFFFFE * ONE, ONE]


def test_empty_inputs():
    dev = small_device()
    for gw, ln in (([], []), ([1, 2], []), ([0, 0], [(0, 1), (1, 2), (1, 2)])):
        counts, info = dev.em_run(3, gw, ln, 50, 0)
        assert not counts.any() and not info[:6].any()
    check(em.CASE4, 1000, 1024, ([ONE, ONE], [1, 2, 2, 0, 1]))


def test_golden_lines():
    import os
    import goldenlib as gl
    headers, gw, ln, reads = em.b6_groups(open(os.path.join(gl.G, "dna_q100_allpaths_fr.b6")).read())
    _, info = check((len(headers), gw, ln), 1000, 1024)
    assert [int(x) for x in info[:5]] == [10, 578, 94, 299, 1]
