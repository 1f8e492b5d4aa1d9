"""The re-scorer on constructed cases (rescorelib.build_cases): records bit for bit against the oracle, and WHICH variant ran
each hit -- the library's BHIP_DEBUG line "re-scorer bands ..." -- against the classification of the oracle's records by the
plain DP.  test_rescore_cases_cpu.py shows from the reference side that these cases reach every variant, edge and tie."""
import re

import numpy as np
import pytest

import oraclelib as ol
import rescorelib as rl
from test_gpu_kernels import assert_hits_equal, oracle_hits, staged_call, with_debug_lines

pytestmark = pytest.mark.gpu

DEFAULTS = {"band": 1, "two_stage": 1, "lanes": 1, "lane_min_entries": 32768, "rescore_reg": 1}
BANDS_LINE = re.compile(r"re-scorer bands " + " ".join("%s:(\\d+)" % b for b in rl.BUCKETS))


@pytest.fixture(scope="module")
def cs():
    return rl.build_cases()


@pytest.fixture(scope="module")
def devices(cs):
    """one handle per score table, no accelerator: every (read, clump) pair is swept"""
    from burst_amd import capi
    devs = {z: capi.Device(cs.packed, cs.clump_len, cs.tot, ol.score_lut(z)) for z in (1, 0)}
    yield devs
    for d in devs.values():
        d.close()


@pytest.fixture
def dev_for(devices):
    """devices[z] with options set for one test; the defaults come back afterwards"""
    def get(z=1, **opts):
        for k, v in {**DEFAULTS, **opts}.items():
            devices[z].set_option(k, v)
        return devices[z]
    yield get
    for d in devices.values():
        for k, v in DEFAULTS.items():
            d.set_option(k, v)


_expected = {}


def expected(cs, key, batch, z, all_hits):
    """the oracle's records of a batch (computed once per batch and mode, shared by the tests)"""
    k = (key, z, bool(all_hits))
    if k not in _expected:
        _expected[k] = oracle_hits(cs.packed, cs.clump_len, cs.tot, batch, ol.score_lut(z), all_hits)
    return _expected[k]


def run(dev, batch, all_hits, capfd, monkeypatch):
    """the staged batch through bhip_align_staged, twice at most: (records, variant histogram summed over the sub-pipelines, number of
    sub-pipelines that reported) of the call that redid nothing"""
    from burst_amd import capi
    dev.stage(batch)
    buf = np.zeros(1 << 17, dtype=capi.HIT_DTYPE)
    for _ in range(2):
        (rc, n), lines = with_debug_lines(capfd, monkeypatch, lambda: staged_call(dev, int(all_hits), buf))
        assert rc == capi.BHIP_OK, (rc, capi.lib().bhip_last_error(), lines)
        if not [ln for ln in lines if "redo:" in ln]:
            break
    else:
        raise AssertionError("the second call redid the chain again: %r" % lines)
    found = [BANDS_LINE.search(ln) for ln in lines]
    found = [m for m in found if m]
    assert found, lines
    hist = {b: sum(int(m.group(i + 1)) for m in found) for i, b in enumerate(rl.BUCKETS)}
    return buf[:n].copy(), hist, len(found)


@pytest.mark.parametrize("all_hits", [False, True])
@pytest.mark.parametrize("opts", [{}, {"band": 0}, {"two_stage": 0}, {"lanes": 3, "lane_min_entries": 8}], ids=["defaults", "band0", "one_stage", "lanes3"])
def test_every_variant_runs_and_agrees(cs, dev_for, opts, all_hits, capfd, monkeypatch):
    """the whole case set: records equal the oracle's, every hit ran in the variant its band width asks for -- under each of the
    sweeps that produce e_first / e_last (prefix + banded window, prefix + full-column window, one-stage sweep, three sub-pipelines)"""
    batch = cs.batch(cs.cases)
    exp = expected(cs, "all", batch, 1, all_hits)
    want = rl.expected_histogram(exp, batch, cs, cs.lut)
    got, hist, n_lanes = run(dev_for(1, **opts), batch, all_hits, capfd, monkeypatch)
    print(n_lanes, hist)
    assert n_lanes == opts.get("lanes", 1)
    assert_hits_equal(got, exp)
    assert hist == want
    assert hist["scratch"] > 0 and all(hist[str(w)] > 0 for w in rl.REG_LIMITS) and hist["lds"] == 0


def test_lds_band_agrees(cs, dev_for, capfd, monkeypatch):
    """rescore_reg = 0: k_rescore<false> takes every band the LDS plan holds -- with query and reference staged in LDS, with rows
    read from global memory (a 452-symbol read in the batch), and under a plan of 16 band rows (budgets capped at 3), where the
    by-span ladder's width 16 stays and 17 leaves for the scratch variant"""
    dev = dev_for(1, rescore_reg=0)
    for key, kw in (("all", {}), ("all+long", {"long_read": True}), ("cap3", {"cap": 3})):
        batch = cs.batch(cs.cases, **kw)
        band_rows = rl.band_rows_of(batch.emac.max())
        assert band_rows == (16 if key == "cap3" else 48)
        if key == "all+long":      # the long read is the batch's last entry and meets nothing: the other entries' records are the batch's
            assert len(batch.seqs[-1]) > 440 and len(expected(cs, "long", rl.Batch([cs.long_read], [batch.emac[-1]]), 1, True)) == 0
        for all_hits in (True, False):
            exp = expected(cs, "all" if key == "all+long" else key, batch, 1, all_hits)
            bands = rl.record_bands(exp, batch, cs, cs.lut)
            live = bands["ed"] > 0
            want = {b: 0 for b in rl.BUCKETS}
            want["lds"], want["scratch"] = int((live & (bands["Wd"] <= band_rows)).sum()), int((live & (bands["Wd"] > band_rows)).sum())
            assert want == rl.expected_histogram(exp, batch, cs, cs.lut, use_reg=False)
            assert want["lds"] > 100 and want["scratch"] > 0
            if key == "cap3":
                span = np.array([c.family == "ladder_span" for c in cs.cases])[exp["q"]]
                assert {16, 17} <= set(bands["Wd"][span].tolist())
            got, hist, _ = run(dev, batch, all_hits, capfd, monkeypatch)
            print(key, all_hits, hist)
            assert_hits_equal(got, exp)
            assert hist == want


def test_wave_fill(cs, dev_for, capfd, monkeypatch):
    """Waves of rescore_reg_one with few and with many live lanes.  The by-edits ladder without its width 41 leaves a handful of hits
    per variant and exactly one for the 48-wide one; both ladders replicated (every copy its own slot) put more than 64 hits and
    not a multiple of 64 into every variant: full waves, a partly live last wave, the ballot compaction of the records."""
    dev = dev_for(1)
    few = cs.batch([c for c in cs.select("ladder_edits") if c.want != 41])
    ladder = cs.select("ladder")
    base = rl.expected_histogram(expected(cs, "ladder", cs.batch(ladder), 1, True), cs.batch(ladder), cs, cs.lut)
    rep = next(n for n in range(33, 200) if all(base[b] * n > 64 and (base[b] * n) % 64 for b in rl.BUCKETS if b != "lds"))
    many = cs.batch(ladder, rep=rep)
    for key, batch in (("few", few), ("many%d" % rep, many)):
        for all_hits in (True, False):
            exp = expected(cs, key, batch, 1, all_hits)
            want = rl.expected_histogram(exp, batch, cs, cs.lut)
            if key == "few":
                assert want["48"] == 1 and max(want.values()) <= 8
            else:
                assert all(want[b] > 64 and want[b] % 64 for b in rl.BUCKETS if b != "lds"), want
            got, hist, _ = run(dev, batch, all_hits, capfd, monkeypatch)
            print(key, all_hits, hist)
            assert_hits_equal(got, exp)
            assert hist == want


@pytest.mark.parametrize("z", [1, 0])
def test_both_score_tables(cs, dev_for, z, capfd, monkeypatch):
    """the phase and tie families under score_lut(1) (N costs 1 against everything) and score_lut(0) (N matches everything)"""
    batch = cs.batch(cs.select("phase", "tie"))
    lut = ol.score_lut(z)
    dev = dev_for(z)
    for all_hits in (True, False):
        exp = expected(cs, "phase+tie", batch, z, all_hits)
        assert len(exp) > 300
        got, hist, _ = run(dev, batch, all_hits, capfd, monkeypatch)
        print(z, all_hits, hist)
        assert_hits_equal(got, exp)
        assert hist == rl.expected_histogram(exp, batch, cs, lut)
