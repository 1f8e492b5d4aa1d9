"""Coverage on the MI355X beyond tests/test_gpu_coverage.py: a failed bhip_cov_add (csrc/bhip_cov.hip) leaves no events on the handle."""
import numpy as np
import pytest

from test_gpu_coverage import lines_of, small_device

pytestmark = pytest.mark.gpu


def test_failed_add_leaves_no_events():
    """two good lines on header 0 and one that names a header beyond bhip_cov_begin's: the call fails (BHIP_E_ARG); the next sample's
    column and Dataset hold that sample alone.  By hand: one line of weight 2 over [0, 10) of header 1: tot 20, cov 10, sq 40, lines 2"""
    from burst_amd import capi
    dev = small_device()
    dev.cov_begin([100, 50], 0)
    try:
        with pytest.raises(capi.BurstHipError) as e:
            dev.cov_add(0, lines_of([0, 0, 5], [1, 10, 1], [20, 30, 5], [1, 1, 1], [1, 1, 1]))
        assert e.value.code == capi.BHIP_E_ARG
        dev.cov_add(1, lines_of([1], [1], [11], [2], [1]))
        want = np.array([[0, 0, 0, 0], [20, 10, 40, 2]], np.uint64)
        for gs, gu in (dev.cov_stats(1), dev.cov_stats(None)):
            assert np.array_equal(gs, want) and np.array_equal(gu, want)
        assert not dev.cov_stats(0)[0].any()
    finally:
        dev.cov_end()

