"""Every sweep variant against the oracle on constructed cells (sweeplib.CELLS): one cell per admissible (NW, NWP) at the top and at the
bottom of NWP's budget range, the one-stage cells, the cells of the long kernel -- records byte for byte, and the library's own counters
against the plain model of the prefix stage: WHICH prefix width ran, how many (entry, lane) windows it flagged, how many columns the
window stage swept.  test_sweep_cases_cpu.py shows from the reference side that these cells reach every variant, placement and band class.

What the counters count (bhip_align.hip, collect_stats): n_windows is the number of window records the prefix kernels wrote, one per
(entry, live lane) with a flagged group of 8 columns; n_window_columns sums, per window, the groups of 8 columns the window kernels
swept; n_columns adds ClumpLen once per (entry, CLUMP) pair of the clump-level sweeps -- not per lane, so with several flagged lanes per
clump the window columns may exceed it, and the bound asserted here is per window instead."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sweeplib as sl
from test_gpu_kernels import assert_hits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"band": 1, "two_stage": 1}
KEYS = list(sl.CLASS_NW) + ["long", "max"]


class Handles:
    """one handle per (length class, feeder), opened when first asked for"""

    def __init__(self):
        self.devs = {}

    def get(self, key, feeder):
        from burst_amd import capi
        if (key, feeder) not in self.devs:
            db = sl.class_db(key)
            self.devs[(key, feeder)] = capi.Device(db.packed, db.clump_len, db.tot, sl.lut(), **(db.acx() if feeder == "tasks" else {}))
        return self.devs[(key, feeder)]

    def close(self):
        for d in self.devs.values():
            d.close()
        self.devs = {}


@pytest.fixture(scope="module")
def handles():
    h = Handles()
    yield h
    h.close()


def run_cell(dev, cell, all_hits, band):
    """the cell's batch through bhip_align_batch under (band, the cell's own options): records, statistics; the defaults come back"""
    for k, v in {**DEFAULTS, **cell.options, "band": band}.items():
        dev.set_option(k, v)
    try:
        got = dev.align_batch(cell.batch(), all_hits=all_hits)
        return got, dev.stats()
    finally:
        for k, v in DEFAULTS.items():
            dev.set_option(k, v)


def check_cell(dev, cell, all_hits, band):
    db, b = sl.class_db(cell.key), cell.batch()
    exp = sl.expected(cell, all_hits)
    got, st = run_cell(dev, cell, all_hits, band)
    print(cell.name, "all_hits", all_hits, "band", band, {k: st[k] for k in ("prefix_words", "n_windows", "n_window_columns", "n_columns", "n_lane_tasks", "n_pairs", "n_raw_hits")}, len(got))
    assert len(exp) > 0
    assert_hits_equal(got, exp)
    assert st["prefix_words"] == cell.nwp
    if not cell.nwp:
        assert st["n_windows"] == 0 and st["n_window_columns"] == 0
        return
    cols_max = max(32 * ((int(L) + 31) // 32) for L in db.clump_len)
    assert 0 < st["n_window_columns"] <= st["n_windows"] * cols_max
    if cell.feeder == "pairs":
        g_first, g_last, _ = sl.model(cell)
        assert st["n_windows"] == int((g_first >= 0).sum())
        assert st["n_window_columns"] == sl.window_columns(db, b, cell.nwp, g_first, g_last)
        assert st["n_columns"] == b.n * int(db.clump_len.sum()) and st["n_pairs"] == b.n * len(db.clump_len) and st["n_lane_tasks"] == 0
    else:
        assert st["n_lane_tasks"] > 0
        g_first, _, _ = sl.model(cell)
        assert 0 < st["n_windows"] <= int((g_first >= 0).sum())        # tasks are a subset of the lanes, and flag what the model flags there


@pytest.mark.parametrize("band", [1, 0])
@pytest.mark.parametrize("all_hits", [False, True])
@pytest.mark.parametrize("cell", sl.CELLS, ids=[c.name for c in sl.CELLS])
def test_cell_equals_the_oracle(handles, cell, all_hits, band):
    """records, prefix width and window counters of one cell in one mode, banded and full-column window sweeps"""
    check_cell(handles.get(cell.key, cell.feeder), cell, all_hits, band)


@pytest.mark.parametrize("key", KEYS)
def test_class_cells_back_to_back_on_one_handle(key):
    """a length class's cells one after the other on a fresh handle: largest Emax first, then the smallest, then the one-stage cells --
    the profile buffers, the flags of the band classes seen and the window buffers of a wide variant are followed by a narrow one's"""
    from burst_amd import capi
    cells = [c for c in sl.CELLS if c.key == key and c.feeder == "pairs"]
    two = sorted((c for c in cells if c.nwp), key=lambda c: -c.emax)
    order = two[:1] + two[-1:] + two[1:-1] + [c for c in cells if not c.nwp]
    db = sl.class_db(key)
    dev = capi.Device(db.packed, db.clump_len, db.tot, sl.lut())
    try:
        for c in order:
            for all_hits in (True, False):
                check_cell(dev, c, all_hits, 1)
        if two:
            check_cell(dev, two[0], True, 0)
            check_cell(dev, two[-1], False, 1)
    finally:
        dev.close()


def test_cells_under_poisoned_allocations():
    """the cells of the 10-word and the 32-word class in a fresh process whose device buffers start as 0xA5 bytes (BHIP_POISON): a
    kernel that reads what nobody wrote -- a profile word beyond the band, a window record of the previous cell -- differs here"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweep_driver.py"), "10", "32"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, BHIP_POISON="165"))
    assert r.returncode == 0 and "sweep driver ok" in r.stdout, r.stdout[-3000:]
