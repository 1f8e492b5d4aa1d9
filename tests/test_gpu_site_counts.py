"""bhip_site_counts against bh_site_counts_host, the definition in plain sequential C, byte for byte: every pairing of the range and record
counts at which the launch shapes change, the ranges written by hand for every edge of the definition, 3000 ranges piled on one position,
a real sample of the variants pool, permutations of the ranges and of the records, no records and no ranges, and every refusal with its
text and a good call behind it."""
import numpy as np
import pytest

import cigarlib as cg
import dbutil
import oraclelib as ol
import pilecases
import vcfstudycases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from burst_amd import capi
    rng = np.random.default_rng(2)
    packed, clump_len, tot = dbutil.pack_clumps([rng.integers(1, 5, size=200, dtype=np.uint8) for _ in range(4)])
    d = capi.Device(packed, clump_len, tot, ol.score_lut(1), device=0)
    yield d
    d.close()


def same(dev, r, s, a, q):
    from burst_amd import host
    got, want = dev.site_counts(r, s, a, q), host.site_counts_host(r, s, a, q)
    assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("n_records", [1, 257, 5000])
@pytest.mark.parametrize("n_ranges", [1, 63, 64, 65, 5000])
def test_sizes(dev, n_ranges, n_records):
    r, s, a, q = vc.random_case(n_ranges, n_records, 100 * n_ranges + n_records)
    got = same(dev, r, s, a, q)
    info = dev.site_counts_info()
    assert (info["ranges"], info["records"]) == (n_ranges, n_records) and info["device_us"] > 0 and info["peak_bytes"] > 0
    if n_ranges >= 63 and n_records >= 257:      # every kind of cell is among them
        site = q["allele"] == 0
        assert got["depth"].max() > 1 and (got["depth"] == 0).any() and got["count"][~site].max() > 0 and (got["count"][~site] == 0).any()
        assert (got["n"][site].sum(1) == got["depth"][site]).any() and (got["n"][site].sum(1) != got["depth"][site]).any()


def test_ranges_written_by_hand(dev):
    ranges, sites, alleles, records, want = vc.hand()
    got = same(dev, *vc.to_arrays(ranges, sites, alleles, records))
    assert vc.cells_as_tuples(got) == want


def test_3000_ranges_piled_on_one_position(dev):
    from burst_amd import capi
    r = np.zeros(3000, capi.COUNT_RANGE_DTYPE)
    r["header"], r["pos"], r["span"], r["w"] = 2, 1000 - np.arange(3000) % 40, 41 + np.arange(3000) % 7, 1 + np.arange(3000) % 3      # all hold 1000 .. 1001
    s, a, q = vc.to_arrays([], [(2, 1000, 3, 0, (5, 6, 7, 8, 0, 0), 0)], [(2, 1000, 4, 1, 0, 2999)], [(2, 1000, 0, 3), (2, 1001, 0, 3), (2, 1000, 4, 0), (2, 960, 0, 1), (2, 1048, 0, 1)])[1:]
    got = vc.cells_as_tuples(same(dev, r, s, a, q))
    total = int(r["w"].sum())
    assert got[0] == (total, (5, 6, 7, 8), 0) and got[1] == (total, (0, 0, total, 0), 0) and got[2] == (total, (0, 0, 0, 0), 2999) and got[3][0] == 0 and got[4][0] == 0


def test_a_sample_of_the_pool(dev, tmp_path_factory):
    L = cg.restate(tmp_path_factory.mktemp("cigar"))
    pool = pilecases.PileCases(L, 1)
    arrays, want = vc.sample_case(pool.model_lines(list(range(len(pool.cases)))), np.random.default_rng(4))
    assert vc.cells_as_tuples(same(dev, *arrays)) == want


def test_a_permutation_of_ranges_and_records_changes_nothing(dev):
    r, s, a, q = vc.random_case(3000, 2000, 8)
    rng = np.random.default_rng(9)
    base = same(dev, r, s, a, q)
    pr, pq = rng.permutation(len(r)), rng.permutation(len(q))
    assert dev.site_counts(r[pr], s, a, q).tobytes() == base.tobytes()
    assert dev.site_counts(r, s, a, q[pq]).tobytes() == base[pq].tobytes()


def test_no_records_and_no_ranges_launch_nothing(dev):
    r, s, a, q = vc.random_case(100, 300, 3)
    same(dev, r, s, a, q)
    assert dev.site_counts_info()["device_us"] > 0
    assert len(dev.site_counts(r, s, a, q[:0])) == 0
    info = dev.site_counts_info()
    assert (info["ranges"], info["records"], info["device_us"]) == (100, 0, 0)
    got = same(dev, r[:0], s, a, q)      # no read anywhere: depth 0, the look-ups stand
    info = dev.site_counts_info()
    assert (info["ranges"], info["records"], info["device_us"]) == (0, 300, 0) and not got["depth"].any() and got["count"].max() > 0


BAD = [("range 1: position 0", lambda r, s, a, q: r["pos"].__setitem__(1, 0)), ("range 1 has weight 0", lambda r, s, a, q: r["w"].__setitem__(1, 0)),
       ("range 1: position 4294967290 + span 6", lambda r, s, a, q: (r["pos"].__setitem__(1, vc.TOP - 5), r["span"].__setitem__(1, 6))),
       ("more than 2^31 - 1 reads", lambda r, s, a, q: r["w"].__setitem__(slice(0, 2), 1 << 30)),
       ("sites not strictly ascending", lambda r, s, a, q: s.__setitem__(1, s[0])), ("alleles not strictly ascending", lambda r, s, a, q: a.__setitem__(1, a[0])),
       ("record 2 has position 0", lambda r, s, a, q: q["pos"].__setitem__(2, 0)),
       ("site record 0 has ref 5", lambda r, s, a, q: (q["allele"].__setitem__(0, 0), q["ref"].__setitem__(0, 5))),
       ("site record 0 has ref 0", lambda r, s, a, q: (q["allele"].__setitem__(0, 0), q["ref"].__setitem__(0, 0)))]


@pytest.mark.parametrize("text,spoil", BAD, ids=[b[0] for b in BAD])
def test_every_refusal_names_its_case_and_leaves_the_handle_usable(dev, text, spoil):
    from burst_amd import capi
    r, s, a, q = vc.random_case(20, 20, 1)
    good = tuple(x.copy() for x in (r, s, a, q))
    spoil(r, s, a, q)
    with pytest.raises(capi.BurstHipError) as e:
        dev.site_counts(r, s, a, q)
    assert e.value.code == capi.BHIP_E_ARG and text in str(e.value)
    same(dev, *good)


def test_a_count_of_2_to_the_32_is_refused_before_anything_is_read(dev):
    from burst_amd import capi
    r, s, a, q = vc.random_case(20, 20, 1)
    cells, info = np.zeros(20, capi.COUNT_CELL_DTYPE), np.zeros(8, np.uint64)
    for k in range(4):
        n = [len(r), len(s), len(a), len(q)]
        n[k] = 1 << 32
        rc = capi.lib().bhip_site_counts(dev._h, capi._ptr(r), n[0], capi._ptr(s), n[1], capi._ptr(a), n[2], capi._ptr(q), n[3], capi._ptr(cells), capi._ptr(info))
        assert rc == capi.BHIP_E_ARG and b"2^32 or more" in capi.lib().bhip_last_error()
    same(dev, r, s, a, q)
