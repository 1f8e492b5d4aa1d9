"""The rules of option "fetch_once" (burst_amd/csrc/bhip_fetch_plan.h), compiled for the host: where a re-scored hit's packed query is kept is
a pure function of the class word count, the kernels' registers and LDS, and the option.  No device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DWORD, LDS, CHUNK = 0, 1, 2
# (registers, static LDS bytes) of k_rescore_reg<SET, FORM> for FORM = dword, lds, chunk as the compiler gives them for gfx950 today ...
RESCORE_SETS = {0: ((71, 64), (71, 64), (90, 64)), 3: ((91, 64), (80, 64), (101, 64)), 1: ((130, 64), (130, 64), (140, 64)), 2: ((153, 64), (153, 64), (163, 64))}
# ... and a sweep of figures around them: the rule must hold whatever the compiler does next (the lds / chunk kernel with as many, fewer and more registers)
SWEEP_SETS = {"r%d%+d%+d" % (r, d1, d2): ((r, 64), (r + d1, 64), (r + d2, 64)) for r in range(40, 201, 8) for d1 in (0, -8, 8) for d2 in (0, 16)}
QWS = list(range(1, 129)) + [160, 255, 256, 257, 1000]


def resident_blocks(threads, regs, static_lds, dyn_lds):
    """the rule of bhip_resident_blocks restated: 512 registers per SIMD lane in steps of 8, 8 waves per SIMD, 148 KB of LDS in steps of 512 B"""
    waves = (threads + 63) // 64
    by_reg = 4 * min(8, 512 // max(8, (regs + 7) // 8 * 8)) // waves
    lds = static_lds + dyn_lds
    by_lds = (148 * 1024) // max(512, (lds + 511) // 512 * 512) if lds else 64
    return max(1, min(by_reg, by_lds))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fetch_plan") / "fetch_plan_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "burst_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "fetch_plan_host.cpp"), "-o", exe])

    def ask_(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in ln.split()] for ln in out]
    return ask_


def test_resident_blocks_follow_registers_and_lds(ask):
    cases = [(t, r, s, d) for t in (64, 256) for r in (1, 8, 64, 71, 72, 73, 80, 96, 128, 129, 256, 512) for s in (0, 64, 2048) for d in (0, 1, 448, 449, 4096, 13144 - 64, 14168 - 64, 65536)]
    got = ask(["blocks %d %d %d %d" % c for c in cases])
    assert [g[0] for g in got] == [resident_blocks(*c) for c in cases]
    # the two measurements the LDS figure comes from: 11 blocks of 13 144 B fit a CU and 10 of 14 168 B
    assert ask(["blocks 64 32 13144 0", "blocks 64 32 14168 0"]) == [[11], [10]]


def test_query_fetch_never_costs_a_resident_block(ask):
    """every class word count 1 .. 128 (and beyond) in every register set: the chosen form keeps the blocks per CU that the same arithmetic
    gives the dword form without dynamic LDS, the LDS area is the class's qw dwords per thread, and the form is the first of lds, chunk,
    dword that keeps them"""
    sets = dict(RESCORE_SETS, **SWEEP_SETS)
    keys = [(name, qw) for name in sets for qw in QWS]
    got = ask(["query %d 1 %d %d %d %d %d %d" % ((qw,) + sum(sets[name], ())) for name, qw in keys])
    n_form = [0, 0, 0]
    for (name, qw), (form, lds, blocks, tail) in zip(keys, got):
        k = sets[name]
        base = resident_blocks(64, k[DWORD][0], k[DWORD][1], 0)
        assert blocks == resident_blocks(64, k[form][0], k[form][1], lds) >= base, (name, qw)
        assert lds == (qw * 256 if form == LDS else 0), (name, qw)
        fits_lds = qw * 256 <= 65536 and resident_blocks(64, k[LDS][0], k[LDS][1], qw * 256) >= base
        fits_chunk = resident_blocks(64, k[CHUNK][0], k[CHUNK][1], 0) >= base
        assert form == (LDS if fits_lds else CHUNK if fits_chunk else DWORD), (name, qw)
        # rows that are no multiple of four dwords start anywhere in a 16-byte chunk and end inside one: flagged for the chunk form
        assert tail == (1 if form == CHUNK and qw % 4 else 0), (name, qw)
        n_form[form] += 1
    assert min(n_form) > 100, n_form


def test_query_fetch_of_the_register_sets(ask):
    """set 0 (bands of 4 .. 8 diagonals, 7 waves per SIMD): reads of up to 128 symbols = 16 dwords take the LDS form; longer classes whatever
    the arithmetic says, here: the LDS form while 28 blocks of qw * 256 + 64 bytes fit 148 KB, then the dword form, because the chunk
    form's registers would cost two waves.  The wide sets (3 waves) have room for both."""
    k = RESCORE_SETS[0]
    rows = ask(["query %d 1 %d %d %d %d %d %d" % ((qw,) + sum(k, ())) for qw in (1, 13, 16, 17, 19, 20, 75)])
    assert rows[:3] == [[LDS, 256, 28, 0], [LDS, 13 * 256, 28, 0], [LDS, 4096, 28, 0]]
    base = resident_blocks(64, 71, 64, 0)
    for qw, row in zip((17, 19, 20, 75), rows[3:]):
        want = LDS if resident_blocks(64, 71, 64, qw * 256) >= base else CHUNK if resident_blocks(64, 90, 64, 0) >= base else DWORD
        assert row[0] == want, (qw, row)
    k = RESCORE_SETS[2]
    rows = ask(["query %d 1 %d %d %d %d %d %d" % ((qw,) + sum(k, ())) for qw in (13, 48, 49, 75, 128, 257)])
    assert [r[0] for r in rows] == [LDS if resident_blocks(64, 153, 64, qw * 256) >= 12 else CHUNK for qw in (13, 48, 49, 75, 128, 257)]
    assert rows[0][0] == LDS and rows[-1] == [CHUNK, 0, 12, 1] and rows[-2] == [CHUNK, 0, 12, 0]


def test_fetch_once_off_is_the_dword_form(ask):
    for name, k in RESCORE_SETS.items():
        rows = ask(["query %d 0 %d %d %d %d %d %d" % ((qw,) + sum(k, ())) for qw in QWS])
        assert all(r == [DWORD, 0, resident_blocks(64, k[0][0], k[0][1], 0), 0] for r in rows), name
