"""bhip_pf_group (burst_amd/csrc/bhip_pf_select.h) on the host: how many lanes a query gets in k_prefilter_cq's first pass -- 8 (eight
queries per wave) only for that kernel in slot mode 0, a short expected stream and a lane whose last chain was not strain-rich; 16 anywhere
else.  No device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CF, MASK = 0, 1        # option prefilter_algo


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pf_group") / "pf_group_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "burst_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "pf_group_host.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def group(ask, rows):
    return [int(x) for x in ask(["group %d %d %d %d %r %r" % r for r in rows])]


def test_limits_are_positive_and_eight_lanes_need_both(ask):
    X, S = (float(v) for v in ask(["limits"])[0].split())
    assert 0.0 < X <= 128.0          # two resident rows of 64 records: nothing longer can be meant for 8 lanes
    assert 0.0 < S <= 16.0           # the 16-slot exact table: a mean query beyond it would overflow
    # (prefilter_group, algo, prefilter_cw, W16, expect, survivors per query of the last chain)
    rows = [(0, CF, 2, 8, X, -1.0), (0, CF, 2, 8, X * 1.01, -1.0),             # expect on both sides of X, first batch of a lane
            (0, CF, 2, 8, X, S), (0, CF, 2, 8, X, S * 1.01),                   # the guard on both sides of its limit
            (0, CF, 2, 8, X * 1.01, 0.0), (0, CF, 2, 8, 1.0, 0.0), (0, CF, 2, 8, 1.0, 1e9)]
    assert group(ask, rows) == [8, 16, 8, 16, 16, 8, 16]


def test_every_kind_slot_mode_and_option_value(ask):
    X, S = (float(v) for v in ask(["limits"])[0].split())
    short, calm = X / 2, S / 2
    for grp in (0, 8, 16):
        eight = 16 if grp == 16 else 8
        rows, want = [], []
        # kinds: k_prefilter_cq (prefilter_cw 2), k_prefilter_cw (1), k_prefilter_cf (0), the exact table (algo 1)
        for w16, mode in ((4, 0), (8, 0), (16, 1), (32, 2)):
            rows.append((grp, CF, 2, w16, short, calm)); want.append(eight if mode == 0 else 16)          # slot mode 2 is k_prefilter_cw<2>
            rows.append((grp, CF, 1, w16, short, calm)); want.append(16)
            rows.append((grp, CF, 0, w16, short, calm)); want.append(16)
            for cw in (0, 1, 2):
                rows.append((grp, MASK, cw, w16, short, calm)); want.append(16)
        assert group(ask, rows) == want, grp
    # a forced 8 ignores the stream and the guard where the kernel has the instance, and only there
    assert group(ask, [(8, CF, 2, 8, X * 100, S * 100), (8, CF, 2, 16, short, calm), (8, CF, 2, 9, short, calm), (16, CF, 2, 8, short, calm)]) == [8, 16, 16, 16]
