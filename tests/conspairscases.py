"""Inputs of bhip_consensus_pairs / bh_consensus_pairs_host for the tests: a case is (n_samples, segs, letters) with segs a
capi.PAIR_SEG_DTYPE array in the order the primitive asks for and letters the bytes the offsets point into."""
import numpy as np

ALPHABET = b"ACGT-NRYACGTACGT"      # every byte class; mostly bases, so that pairs agree and differ


def build(spec):
    """spec: {(sample, header): [(pos, letters bytes), ...]} -> (segs, letters), the segments ascending by (sample, header, pos)"""
    from burst_amd import capi
    flat = sorted((s, h, p, t) for (s, h), lst in spec.items() for p, t in lst)
    segs, letters = np.zeros(len(flat), capi.PAIR_SEG_DTYPE), bytearray()
    for i, (s, h, p, t) in enumerate(flat):
        segs[i] = (s, h, p, len(t), len(letters))
        letters += t
    return segs, bytes(letters)


def rand_letters(rng, n):
    return bytes(ALPHABET[k] for k in rng.integers(0, len(ALPHABET), size=n))


def rand_segments(rng, lo, hi, max_segs=3):
    """up to max_segs disjoint segments inside [lo, hi), ascending; two of them may abut"""
    cuts = sorted(set(int(x) for x in rng.integers(lo, hi + 1, size=2 * int(rng.integers(1, max_segs + 1)))))
    return [(a, b) for a, b in zip(cuts[0::2], cuts[1::2]) if b > a]


def one_header(n_samples, union_len, seed, header=5, base=1000):
    """n_samples samples on one header whose union is exactly [base, base + union_len): sample 0 covers its head and the last sample its
    tail (abutting for an even seed, overlapping else); the others lie anywhere inside"""
    rng = np.random.default_rng(seed)
    spec = {}
    if n_samples == 1:
        spec[(0, header)] = [(base, rand_letters(rng, union_len))]
    else:
        c = int(rng.integers(1, union_len)) if union_len > 1 else 1
        c2 = c if seed % 2 == 0 or union_len == 1 else int(rng.integers(0, c + 1))
        if union_len == 1:
            c2 = 0
        spec[(0, header)] = [(base, rand_letters(rng, c))]
        spec[(n_samples - 1, header)] = [(base + c2, rand_letters(rng, union_len - c2))]
        for s in range(1, n_samples - 1):
            lst = [(a, rand_letters(rng, b - a)) for a, b in rand_segments(rng, base, base + union_len)]
            if lst:
                spec[(s, header)] = lst
    return (n_samples,) + build(spec)


def random_case(seed, n_samples=9, n_headers=12, max_len=700):
    """headers with gaps in their numbers, some with one sample only, union lengths up to max_len"""
    rng = np.random.default_rng(seed)
    spec = {}
    header = 0
    for _ in range(n_headers):
        header += int(rng.integers(1, 4))
        lo = int(rng.integers(1, 5000))
        hi = lo + int(rng.integers(1, max_len + 1))
        for s in rng.permutation(n_samples)[:int(rng.integers(1, n_samples + 1))]:
            lst = [(a, rand_letters(rng, b - a)) for a, b in rand_segments(rng, lo, hi)]
            if lst:
                spec[(int(s), header)] = lst
    return (n_samples,) + build(spec)


def shapes():
    """the segment shapes and letters written by hand (4 samples)"""
    spec = {
        # header 3: two union intervals, 10 and 12 positions, that share the first compressed word; the first is made only by abutting
        # segments of different samples (0: 100..104, 1: 105..109), which therefore share no position: Compared == 0 for (0, 1) there ...
        (0, 3): [(100, b"ACGTA"), (9000, b"ACGT-ACGTNNN")],
        (1, 3): [(105, b"CCCCC"), (9000, b"ACGA--CGTACG")],      # ... but 9000..9011: T/A differ, -/- equal, A/- differ, N never
        (2, 3): [(102, b"GTAC"), (9003, b"T")],
        # header 4, the next number: 5 positions; without the padding its planes would share header 3's last word
        (0, 4): [(1, b"ACGTR")],
        (3, 4): [(1, b"ACGAR")],      # R against R is not compared
        # header 5: one participant between two headers that have pairs
        (2, 5): [(50, b"ACGTACGT")],
        # header 40 (a gap in the numbers): segments that start and end mid-word, 130 positions from 7
        (1, 40): [(7, b"A" * 70), (90, b"C" * 47)],
        (2, 40): [(60, b"A" * 10 + b"-" * 10 + b"C" * 30)],
        (3, 40): [(77, b"N" * 60)],      # covers, is never comparable: Compared == 0 with both
    }
    return (4,) + build(spec)


def long_segment(seed=21):
    """one sample's ONE segment over 9 000 positions (141 words: a wave's lanes take three passes over it), starting mid-word on the
    compressed axis because another sample starts 37 positions before it; a third sample in pieces; a small header behind it"""
    rng = np.random.default_rng(seed)
    spec = {
        (0, 9): [(1037, rand_letters(rng, 9000))],
        (1, 9): [(1000, rand_letters(rng, 100)), (5000, rand_letters(rng, 4160)), (9990, rand_letters(rng, 60))],
        (2, 9): [(a, rand_letters(rng, b - a)) for a, b in rand_segments(rng, 1000, 10050, 6)],
        (0, 10): [(5, rand_letters(rng, 70))],
        (2, 10): [(9, rand_letters(rng, 70))],
    }
    return (3,) + build(spec)


def wide_header(seed=22, n=40000):
    """a header of n positions and more (over 256 words: several workgroups share a pair's cell) with mid-word ends, three samples, and
    a small header before and behind it"""
    rng = np.random.default_rng(seed)
    spec = {
        (0, 2): [(3, rand_letters(rng, 200))],
        (1, 2): [(90, rand_letters(rng, 200))],
        (0, 7): [(500, rand_letters(rng, n))],
        (1, 7): [(533, rand_letters(rng, n // 2 - 533)), (n // 2 + 11, rand_letters(rng, n // 2 + 389))],
        (2, 7): [(700, rand_letters(rng, n - 1700))],
        (1, 8): [(1, rand_letters(rng, 130))],
        (2, 8): [(64, rand_letters(rng, 130))],
    }
    return (3,) + build(spec)


def relabel(case, i, j):
    """the data of samples i and j exchanged"""
    n, segs, letters = case
    spec = {}
    for g in segs:
        s = int(g["sample"])
        s = j if s == i else i if s == j else s
        spec.setdefault((s, int(g["header"])), []).append((int(g["pos"]), letters[int(g["off"]):int(g["off"]) + int(g["len"])]))
    return (n,) + build(spec)


def bad_arguments():
    """(what, n_samples, rows of segs, letters, min_compared, a piece of the text)"""
    L = b"ACGTACGTACGT"
    return [
        ("sample order", 3, [(1, 2, 1, 4, 0), (0, 2, 1, 4, 4)], L, 1, "not ascending"),
        ("header order", 3, [(0, 3, 1, 4, 0), (0, 2, 1, 4, 4)], L, 1, "not ascending"),
        ("pos order", 3, [(0, 2, 9, 2, 0), (0, 2, 1, 4, 4)], L, 1, "segment 1"),
        ("overlap", 3, [(0, 2, 1, 4, 0), (0, 2, 4, 4, 4)], L, 1, "overlapping"),
        ("pos 0", 3, [(0, 2, 0, 4, 0)], L, 1, "position 0"),
        ("len 0", 3, [(0, 2, 1, 0, 0)], L, 1, "length 0"),
        ("beyond 2^32 - 1", 3, [(0, 2, 0xFFFFFFFC, 4, 0)], L, 1, "at most 2^32 - 1"),
        ("letters", 3, [(0, 2, 1, 4, 9)], L, 1, "owns letters"),
        ("letters offset", 3, [(0, 2, 1, 4, 13)], L, 1, "owns letters"),
        ("sample", 3, [(3, 2, 1, 4, 0)], L, 1, "names sample 3 of 3"),
        ("n_samples", 65536, [(0, 2, 1, 4, 0)], L, 1, "at most 65535"),
        ("min 0", 3, [(0, 2, 1, 4, 0)], L, 0, "min_compared"),
        ("min 2^31", 3, [(0, 2, 1, 4, 0)], L, 1 << 31, "min_compared"),
    ]


def seg_rows(rows):
    from burst_amd import capi
    a = np.zeros(len(rows), capi.PAIR_SEG_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a
