"""bhip_stage_spans with packed uploads at every phase.  A span's symbols arrive four per byte (codes2 -> k_unpack2) or two per byte
(codes4 -> k_unpack4) at the phase its first symbol has in the CALLER's array, and are unpacked to wherever the batch's symbols so
far end: source phase (off[0] & 3, or the nibble parity) and destination residue (offset & 3 of the span inside the batch) are
independent, and the kernels take another path for each -- the funnel shift over two source dwords, the byte tails of the first and the
last destination dword.  test_pipelined_spans_equal_one_call_batches stages spans whose offsets and sizes are all multiples of 4; here
the cuts are chosen so that all 16 (source phase, destination residue) pairs of k_unpack2 and all 8 of k_unpack4 occur for a span that
is not the first of its batch, with reads of 20 .. 70 symbols whose budgets equal their planted edits: one wrong symbol loses a record."""
import numpy as np
import pytest

import sweeplib as sl
from test_gpu_kernels import oracle_hits

pytestmark = pytest.mark.gpu

SEED = 20261022
U = 48                         # reads in the caller's array: forward entries 0 .. U - 1, their reverse complements U .. 2 U - 1
TINY = (20, 33)                # reads of 3 symbols: a batch of one of them is two spans of byte tails only
IUPAC_READ = U - 1             # the read that holds an IUPAC symbol: its batch cannot go four symbols per byte


def build_reads():
    """reads of 20 .. 70 symbols (every residue modulo 4 many times over) cut from the lanes of the 2-word class's database, with 0 .. 2
    substitutions and that budget; two reads of 3 symbols; a compatible IUPAC code in the last read"""
    from burst_amd import synth
    rng = np.random.default_rng(SEED)
    db = sl.class_db(2)
    lens = rng.permutation(np.arange(20, 71))[:U]
    reads, emac = [], []
    for i in range(U):
        m = 3 if i in TINY else int(lens[i])
        lane = int(rng.integers(0, db.tot))
        st = int(rng.integers(0, db.lens[lane] - m))
        q = db.seqs[lane][st:st + m].copy()
        k = 0 if i in TINY else i % 3
        for p in rng.choice(np.arange(2, m - 2), size=k, replace=False) if k else ():
            q[p] = q[p] % 4 + 1
        if i == IUPAC_READ:
            q[7] = synth.COMPAT[int(q[7])][0]
        reads.append(q if i % 2 == 0 else synth.revcomp(q))
        emac.append(k)
    return db, reads, emac


def phases(off, u0, u1, packed):
    """of the batch [u0, u1): (source phase of the first span, of the second, destination residue of the second, destination end & 3 of both).
    The first span goes to offset 0 of the batch, the second behind the forward entries' symbols."""
    mask = 3 if packed == "codes2" else 1
    n_fwd = int(off[u1] - off[u0])
    return int(off[u0]) & mask, int(off[U + u0]) & mask, n_fwd & 3, (n_fwd & 3, (2 * n_fwd) & 3)


def choose_cuts(off, packed):
    """batches of 3 .. 10 consecutive reads, taken greedily until every (source phase, destination residue) pair of a second span has
    occurred; then the batch of one 3-symbol read, and for codes4 a batch around the read with the IUPAC symbol"""
    want = {(s, d) for s in range(4 if packed == "codes2" else 2) for d in range(4)}
    last = U - 1 if packed == "codes2" else U                # (four per byte: never the read with the IUPAC symbol)
    cuts, seen = [], set()
    sized = [(u0, 3 + (5 * u0) % 8) for u0 in range(last)]      # a first pass with sizes that cycle through 3 .. 10, then whatever is missing
    for u0, n in sized + [(u0, n) for n in range(3, 11) for u0 in range(last)]:
        if u0 + n > last or seen == want:
            continue
        _, s2, d2, _ = phases(off, u0, u0 + n, packed)
        if (s2, d2) not in seen:
            seen.add((s2, d2)); cuts.append((u0, u0 + n))
    t = TINY[0] if packed == "codes2" else TINY[1]
    cuts.append((t, t + 1))
    if packed == "codes4":
        cuts.append((U - 5, U))
    return cuts


@pytest.fixture(scope="module")
def setup():
    from burst_amd import capi, synth
    db, reads, emac = build_reads()
    allq = reads + [synth.revcomp(r) for r in reads]
    big = capi.Queries(allq, emac * 2, list(range(U)) * 2, [0] * U + [1] * U)
    n = len(big.codes)
    pad = np.concatenate([big.codes, np.zeros(4, np.uint8)])
    nb4, nb2 = (n + 1) // 2, (n + 3) // 4
    codes4 = ((pad[0::2][:nb4] & 15) | ((pad[1::2][:nb4] & 15) << 4)).astype(np.uint8)
    two = ((pad - 1) & 3).astype(np.uint8)
    codes2 = (two[0::4][:nb2] | (two[1::4][:nb2] << 2) | (two[2::4][:nb2] << 4) | (two[3::4][:nb2] << 6)).astype(np.uint8)
    # what the spans carry as plain `codes`: every symbol WRONG (1 -> 2 -> 3 -> 4 -> 1, the IUPAC code a base).  With a packed array in every
    # span the library uploads and unpacks that one and never reads `codes` (stage_enqueue), so the records can only come out right
    # through k_unpack2 / k_unpack4; if the packed arrays stopped being forwarded, every read would change and the test fail
    decoy = (big.codes % 4 + 1).astype(np.uint8)
    assert (decoy != big.codes).all() and decoy.min() >= 1 and decoy.max() <= 4
    return dict(db=db, reads=reads, allq=allq, emac=emac, big=big, codes4=codes4, codes2=codes2, len16=np.diff(big.off).astype(np.uint16), decoy=decoy)


def check_coverage(off, cuts, packed):
    """plain Python, before any device work: the cut table covers what this test is for"""
    ph = [phases(off, u0, u1, packed) for u0, u1 in cuts]
    n_src = 4 if packed == "codes2" else 2
    assert {(s2, d2) for _, s2, d2, _ in ph} == {(s, d) for s in range(n_src) for d in range(4)}      # 16 pairs (codes2), 8 (codes4)
    assert {s1 for s1, _, _, _ in ph} == set(range(n_src))
    assert all(1 <= u1 - u0 <= 10 for u0, u1 in cuts) and sum(u1 - u0 >= 3 for u0, u1 in cuts) >= len(cuts) - 1
    sizes = [int(off[u1] - off[u0]) for u0, u1 in cuts]
    assert any(s < 4 for s in sizes)                          # spans of byte tails only
    ends = {e for _, _, _, both in ph for e in both}
    assert 0 in ends and len(ends) == 4                      # a span that ends exactly on a dword, and every other residue
    assert len(cuts) <= 24


@pytest.mark.parametrize("packed", ["codes2", "codes4"])
def test_cut_table_covers_every_phase(setup, packed):
    off = setup["big"].off
    cuts = choose_cuts(off, packed)
    check_coverage(off, cuts, packed)
    has_iupac = [u0 <= IUPAC_READ < u1 for u0, u1 in cuts]
    assert any(has_iupac) == (packed == "codes4")
    assert (setup["big"].codes > 4).sum() == 2 and all(((r >= 1) & (r <= 4)).all() for r in setup["reads"][:IUPAC_READ])
    lens = np.diff(off)[:U]
    assert {int(x) & 3 for x in lens} == {0, 1, 2, 3} and 20 <= lens[lens > 3].min() and lens.max() <= 70


@pytest.mark.parametrize("all_hits", [False, True])
@pytest.mark.parametrize("packed", ["codes2", "codes4"])
def test_packed_spans_at_every_phase_equal_the_oracle(setup, packed, all_hits):
    """every batch of the cut table, staged two ahead as two spans of one caller array with `len` given: the oracle's records for that
    batch with the caller's query numbers (as test_pipelined_spans_equal_one_call_batches computes them).  The spans' plain `codes` are
    a decoy with every symbol wrong: only the packed upload can give these records."""
    from burst_amd import capi
    db, big, reads, allq, emac = setup["db"], setup["big"], setup["reads"], setup["allq"], setup["emac"]
    cuts = choose_cuts(big.off, packed)
    check_coverage(big.off, cuts, packed)

    def spans_of(u0, u1):
        out = []
        for base in (0, U):
            sp = dict(codes=setup["decoy"], off=big.off[base + u0:base + u1 + 1], emac=big.emac[base + u0:base + u1], rc=big.rc[base + u0:base + u1],
                      q_base=base + u0, len=setup["len16"][base + u0:base + u1])
            sp[packed] = setup[packed]
            out.append(sp)
        return out

    def expected(u0, u1):
        n = u1 - u0
        sub = capi.Queries(reads[u0:u1] + allq[U + u0:U + u1], emac[u0:u1] * 2, list(range(n)) * 2, [0] * n + [1] * n)
        exp = oracle_hits(db.packed, db.clump_len, db.tot, sub, sl.lut(), all_hits).copy()
        q = exp["q"].astype(np.int64)
        exp["q"] = np.where(q < n, u0 + q, U + u0 + (q - n)).astype(np.uint32)
        return exp

    exps = [expected(u0, u1) for u0, u1 in cuts]
    assert all(len(e) >= u1 - u0 for e, (u0, u1) in zip(exps, cuts))          # every read hits
    dev = capi.Device(db.packed, db.clump_len, db.tot, sl.lut())
    try:
        for k in range(min(2, len(cuts))):
            dev.stage_spans(spans_of(*cuts[k]), cuts[k][1] - cuts[k][0], 70 if k % 2 else 0)
        for k in range(len(cuts)):
            if k + 2 < len(cuts):
                dev.stage_spans(spans_of(*cuts[k + 2]), cuts[k + 2][1] - cuts[k + 2][0], 70 if k % 2 else 0)
            got, _ = dev.align_staged(all_hits)
            assert got.tobytes() == exps[k].tobytes(), (packed, all_hits, k, cuts[k], phases(big.off, *cuts[k], packed), len(got), len(exps[k]))
    finally:
        dev.set_option("discard_staged", 1)
        dev.close()
