"""bhip_md_tags against the Python model (tests/samlib.py), byte for byte (md, md_off, nm): cigarlib's pool of lanes and paths (21 lanes in
two clumps, lanes 0 and 15 of a clump, reads of 2 .. 1 100 symbols), planted paths on the dword and chunk boundaries of a lane, the batch
sizes at the scan's wave and block edges, capacity, arguments and the call's figures."""
import ctypes as C

import numpy as np
import pytest

import cigarlib as cg
import pilecases
import samlib

pytestmark = pytest.mark.gpu


class Pool(pilecases.PileCases):
    def __init__(self, L):
        from burst_amd import capi
        super().__init__(L, 1)
        self.dev = capi.Device(self.packed, self.clump_len, self.tot, self.lut, device=0)

    def arrays_of(self, paths):
        """paths: [(refIx, ref_first, op words)] -> (requests, ref_first, op_off, ops)"""
        from burst_amd import capi
        req = np.zeros(len(paths), capi.PATH_REQ_DTYPE)
        req["refIx"] = [p[0] for p in paths]
        first = np.array([p[1] for p in paths], np.uint32)
        off = np.zeros(len(paths) + 1, np.uint64)
        off[1:] = np.cumsum([len(p[2]) for p in paths])
        ops = np.concatenate([np.asarray(p[2], np.uint32) for p in paths]) if paths else np.zeros(0, np.uint32)
        return req, first, off, ops.astype(np.uint32)

    def check(self, paths, cap=None):
        req, first, off, ops = self.arrays_of(paths)
        md, md_off, nm = self.dev.md_tags(req, first, off, ops, cap=cap)
        e_md, e_off, e_nm = samlib.md_batch(self.seqs, req["refIx"], first, off, ops)
        assert md.tobytes() == e_md and md_off.tolist() == e_off and nm.tolist() == e_nm
        info = self.dev.md_info()
        assert info["requests"] == len(paths) and info["md_bytes"] == len(e_md)
        return e_md

    def case_paths(self, idx):
        return [(self.cases[i]["refIx"], self.cases[i]["ref_first"], self.cases[i]["ops"]) for i in idx]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return cg.restate(tmp_path_factory.mktemp("cigar"))


@pytest.fixture(scope="module")
def pool(L):
    p = Pool(L)
    yield p
    p.dev.close()


def test_whole_pool(pool):
    lanes = {c["refIx"] for c in pool.cases}
    assert len(pool.seqs) == 21 and {0, 16} <= lanes and max(lanes) >= 16      # (lane 15 of the first clump: the planted paths below)
    md = pool.check(pool.case_paths(range(len(pool.cases))))
    assert b"^" in md and len(md) > 1000
    info = pool.dev.md_info()
    assert info["device_us"] > 0 and info["peak_bytes"] > len(md)


def test_planted_boundaries(pool):
    """X and D on lane columns 7|8 and 31|32 (a dword and a chunk boundary), a path from column 1, one that ends on the lane's last column,
    a D run across a dword boundary, a one-symbol read"""
    W = lambda text: samlib.words(text)
    n0, n15 = len(pool.seqs[0]), len(pool.seqs[15])
    paths = [(0, 7, W("2X")), (0, 7, W("1=1D3=")), (0, 8, W("1D1X")), (0, 31, W("2X")), (0, 31, W("2D")), (0, 32, W("1X1D1X")), (15, 31, W("1=2D1X")),
             (0, 1, W("1X5=1D")), (15, 1, W("3D")), (0, n0, W("1X")), (15, n15 - 4, W("2=1I1D2X")), (0, 5, W("2=6D2=")), (16, 28, W("9D")), (0, 3, W("1=")), (15, 9, W("1X")),
             (0, 60, W("4I")), (16, 1, W("100=1X"))]
    md = pool.check(paths)
    assert md.count(b"^") == 10


@pytest.mark.parametrize("n", [0, 1, 64, 65, 256, 257])
def test_batch_sizes(pool, n):
    rng = np.random.default_rng(n + 1)
    pool.check(pool.case_paths([int(i) for i in rng.integers(0, len(pool.cases), size=n)]))
    if n == 0:
        assert pool.dev.md_info()["device_us"] == 0      # (nothing was launched)


def test_capacity_then_the_right_room(pool):
    from burst_amd import capi
    paths = pool.case_paths(range(0, len(pool.cases), 3))
    req, first, off, ops = pool.arrays_of(paths)
    e_md, e_off, e_nm = samlib.md_batch(pool.seqs, req["refIx"], first, off, ops)
    n = len(paths)
    lib, h = capi.lib(), pool.dev._h
    for cap in (len(e_md) - 1, len(e_md)):
        md, md_off, nm, info = np.full(len(e_md) + 8, 0x55, np.uint8), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32), np.zeros(8, np.uint64)
        rc = lib.bhip_md_tags(h, capi._ptr(req), capi._ptr(first), capi._ptr(off), capi._ptr(ops), n, capi._ptr(md), cap, capi._ptr(md_off), capi._ptr(nm), capi._ptr(info))
        assert md_off.tolist() == e_off and nm.tolist() == e_nm and int(info[2]) == len(e_md)
        if cap < len(e_md):
            assert rc == capi.BHIP_E_CAPACITY
        else:
            assert rc == 0 and md[:cap].tobytes() == e_md and (md[cap:] == 0x55).all()


def test_bad_arguments_leave_the_handle_usable(pool):
    from burst_amd import capi
    good = pool.case_paths([0, 1, 2])
    n0 = len(pool.seqs[0])
    clump0 = int(pool.clump_len[0])
    bad = [[(0, 1, [3 << 4 | 3])], [(0, 1, [7])], [(pool.tot, 1, [1 << 4 | 7])], [(16 * len(pool.clump_len), 1, [1 << 4 | 7])], [(0, 0, [1 << 4 | 7])],
           [(0, clump0, [2 << 4 | 7])], [(0, 2, [clump0 << 4 | 2])]]
    for paths in bad:
        req, first, off, ops = pool.arrays_of(good + paths)
        with pytest.raises(capi.BurstHipError) as e:
            pool.dev.md_tags(req, first, off, ops)
        assert e.value.code == capi.BHIP_E_ARG and "bhip_md_tags" in str(e.value)
        pool.check(good)
    req, first, off, ops = pool.arrays_of(good)
    off2 = off.copy()
    off2[1], off2[2] = off[2], off[1]      # not ascending
    with pytest.raises(capi.BurstHipError):
        pool.dev.md_tags(req, first, off2, ops)
    lib = capi.lib()
    assert lib.bhip_md_tags(pool.dev._h, None, None, None, None, 3, None, 0, None, None, None) == capi.BHIP_E_ARG
    pool.check(good)
    assert n0 <= clump0
