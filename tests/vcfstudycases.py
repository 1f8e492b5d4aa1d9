"""The inputs the study-VCF tests share: ranges, sites, alleles and records written by hand for every edge of bhip_site_counts with the
cells they must give, random inputs of a given size, and the arrays of a vcfstudylib sample.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import vcfstudylib

TOP = (1 << 32) - 1
INS_AC = 2 << 60 | 1 << 56 | 2 << 52      # Ins(A C)


def to_arrays(ranges, sites, alleles, records):
    from burst_amd import capi
    r = np.array([tuple(x) for x in ranges], capi.COUNT_RANGE_DTYPE) if ranges else np.zeros(0, capi.COUNT_RANGE_DTYPE)
    s = np.zeros(len(sites), capi.PILE_SITE_DTYPE)
    for i, (h, p, ref, depth, n, ins) in enumerate(sites):
        s[i] = (h, p, ref, depth, tuple(n), ins)
    a = np.zeros(len(alleles), capi.ALLELE_DTYPE)
    for i, (h, p, word, ref, depth, count) in enumerate(alleles):
        a[i] = (h, p, word, ref, depth, count, 0, 0)
    q = np.zeros(len(records), capi.COUNT_RECORD_DTYPE)
    for i, (h, p, word, ref) in enumerate(records):
        q[i] = (h, p, word, ref, 0)
    return r, s, a, q


def cells_as_tuples(cells):
    return [(int(c["depth"]), tuple(int(x) for x in c["n"]), int(c["count"])) for c in cells]


def hand():
    """(ranges, sites, alleles, records, expected cells): every edge the definition names"""
    ranges = [(3, 10, 11, 2),            # covers 10 .. 20 of header 3, whose last position is 20 ...
              (4, 1, 5, 7),              # ... and header 4 begins at position 1
              (3, 15, 0, 5),             # span 0: contributes nothing
              (3, 12, 3, 4),             # 12 .. 14
              (5, TOP - 100, 100, 3),    # pos + span = 2^32 - 1: covers up to 2^32 - 2
              (9, 1, 1, 1)]
    sites = [(3, 12, 2, 6, (1, 5, 0, 0, 0, 0), 0), (3, 20, 4, 2, (0, 0, 0, 1, 1, 0), 0)]
    alleles = [(3, 14, 2, 1, 6, 1), (3, 14, INS_AC, 1, 6, 2), (4, 2, 1, 3, 7, 7)]
    records = [(3, 20, 0, 4), (4, 1, 0, 1), (3, 21, 0, 1), (3, 9, 0, 2),      # the last position of 3 (site present), position 1 of 4, behind and before the range
               (3, 15, 0, 3), (3, 12, 0, 2), (3, 13, 0, 3),                   # the span-0 range adds nothing; site present; site absent: all on ref
               (5, TOP - 1, 0, 1), (5, TOP, 0, 1), (5, TOP - 101, 0, 1),      # the last covered position, the one behind it, the one before the range
               (7, 5, 0, 1), (7, 5, 9, 0), (2, 12, 0, 2),                     # records no range holds (a site and an allele), another header at a covered position
               (3, 14, 2, 0), (3, 14, INS_AC, 0), (3, 14, 3, 0), (3, 13, 2, 0),   # two words on one anchor, an absent word there, an absent anchor
               (4, 2, 1, 0), (4, 2, 0, 3), (3, 14, 2, 0)]                     # an allele and a site record at one position; a record twice
    cells = [(2, (0, 0, 0, 1), 0), (7, (7, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0),
             (2, (0, 0, 2, 0), 0), (6, (1, 5, 0, 0), 0), (6, (0, 0, 6, 0), 0),
             (3, (3, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0),
             (0, (0, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0),
             (6, (0, 0, 0, 0), 1), (6, (0, 0, 0, 0), 2), (6, (0, 0, 0, 0), 0), (6, (0, 0, 0, 0), 0),
             (7, (0, 0, 0, 0), 7), (7, (0, 0, 7, 0), 0), (6, (0, 0, 0, 0), 1)]
    return ranges, sites, alleles, records, cells


def random_case(n_ranges, n_records, seed):
    """arrays of a given size: ranges that overlap on a few headers (spans 0 .. 60), sorted sites and alleles at some of the positions, records
    at positions with and without a site / an allele, in no order.  Each cell stands alone, so the lists need not be one sample's"""
    from burst_amd import capi
    rng = np.random.default_rng(seed)
    width = max(50, 4 * n_ranges)
    r = np.zeros(n_ranges, capi.COUNT_RANGE_DTYPE)
    r["header"], r["pos"] = rng.integers(0, 5, n_ranges) * 3, rng.integers(1, width, n_ranges)
    r["span"], r["w"] = rng.integers(0, 61, n_ranges), rng.integers(1, 5, n_ranges)
    n_pos = min(2000, 5 * width)
    keys = np.unique(rng.integers(0, 5, n_pos).astype(np.uint64) * 3 << np.uint64(32) | rng.integers(1, width + 70, n_pos).astype(np.uint64))
    s = np.zeros(len(keys), capi.PILE_SITE_DTYPE)
    s["header"], s["pos"], s["ref"] = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF), rng.integers(1, 5, len(keys))
    s["n"] = rng.integers(0, 9, (len(keys), 6))
    words = np.array([1, 2, 7, 1 << 60 | 3 << 56, INS_AC, 15 << 60 | 0x123456789ABCDEF], np.uint64)
    ak = np.unique(np.stack([rng.choice(keys, len(keys)), rng.choice(words, len(keys))], 1), axis=0)      # (rows sorted by key, then by word)
    a = np.zeros(len(ak), capi.ALLELE_DTYPE)
    a["header"], a["pos"], a["allele"], a["count"] = ak[:, 0] >> np.uint64(32), ak[:, 0] & np.uint64(0xFFFFFFFF), ak[:, 1], rng.integers(1, 9, len(ak))
    q = np.zeros(n_records, capi.COUNT_RECORD_DTYPE)
    q["header"], q["pos"] = rng.integers(0, 6, n_records) * 3, rng.integers(1, width + 80, n_records)
    pick = rng.integers(0, 4, n_records)      # 0: any position; 1: a site's; 2: an allele's with its word; 3: an allele's position with any word
    at_site, at_al = rng.integers(0, len(s), n_records), rng.integers(0, len(a), n_records)
    for f in ("header", "pos"):
        q[f] = np.where(pick == 1, s[f][at_site], np.where(pick >= 2, a[f][at_al], q[f]))
    q["allele"] = np.where(pick == 2, a["allele"][at_al], np.where(pick == 3, rng.choice(words, n_records), 0))
    q["ref"] = np.where(q["allele"] == 0, rng.integers(1, 5, n_records), 0)
    return r, s, a, q


def sample_case(lines, rng, n_extra=300):
    """one vcfstudylib sample (pilelib lines) as arrays, with records at every position it observes on an A/C/G/T column (a subset of at most
    3000), at positions nobody observes, at every allele and at words and anchors it does not carry; and the cells of the dictionaries"""
    c, ranges, sites, alleles = vcfstudylib.arrays(lines)
    spots = [(h, p, 0, s["ref"]) for (h, p), s in c.sites.items() if 1 <= s["ref"] <= 4]
    event_spots = [x for x in spots if c.sites[(x[0], x[1])]["events"]]
    if len(spots) > 3000:
        spots = [spots[i] for i in rng.choice(len(spots), 3000, replace=False)] + event_spots
    records = spots + [(h, p + 5000000, 0, 1 + int(rng.integers(0, 4))) for h, p, _, _ in spots[:n_extra]]
    for h, p, word, ref, depth, cnt in alleles:
        records += [(h, p, word, 0), (h, p, word + 1, 0), (h, p + 5000000, word, 0)]
    order = rng.permutation(len(records))
    records = [records[i] for i in order]
    return to_arrays(ranges, sites, alleles, records), [vcfstudylib.cell(c, r) for r in records]
