"""An independent model of burst_hip --sam: the MD string and NM of a path from the lane's codes and the ops, and a whole expected SAM file
from the text of a `.b6 --cigar` output, the query FASTA, the reference FASTA and the @SQ lengths.  Nothing here calls the project's code.
TEST INFRASTRUCTURE ONLY.

The model takes the reads' names as distinct (it asserts so): a read is then the run of consecutive lines with one column 1, whose first line
is the primary record."""
import re

MD_LETTERS = "NACGTNKMRYSWBVHD"       # the letter of a reference code under X and D: the pad code 0 prints N
SEQ_LETTERS = ".ACGTNKMRYSWBVHD"      # the letter of a query code in SEQ
OP_CHAR = {1: "I", 2: "D", 7: "=", 8: "X"}
OP_CODE = {c: k for k, c in OP_CHAR.items()}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "K": "M", "M": "K", "R": "Y", "Y": "R", "S": "S", "W": "W", "B": "V", "V": "B", "H": "D", "D": "H"}
WS = re.compile(r"[ \t\r\n\v\f]")


def words(text):
    """a CIGAR text in =XID as op words length << 4 | code"""
    return [int(n) << 4 | OP_CODE[c] for n, c in re.findall(r"(\d+)([=XID])", text)]


def md_walk(letter_at, col, items):
    """samtools calmd's walk: letter_at(col) = the reference letter of 0-based column col; items = [(length, op char)].  Returns (MD text, NM)"""
    out, u, nm = [], 0, 0
    for n, c in items:
        if c == "=":
            u += n
            col += n
        elif c == "X":
            for _ in range(n):
                out.append("%d%s" % (u, letter_at(col)))
                u = 0
                col += 1
            nm += n
        elif c == "D":
            out.append("%d^%s" % (u, "".join(letter_at(col + k) for k in range(n))))
            u = 0
            col += n
            nm += n
        elif c == "I":
            nm += n
        else:
            raise ValueError("not an op: %r" % (c,))
    out.append("%d" % u)
    return "".join(out), nm


def md_codes(lane, ref_first, ops):
    """(MD bytes, NM) of op words over a lane of codes; ref_first 1-based"""
    def letter(col):
        if not 0 <= col < len(lane):
            raise IndexError("column %d of a lane of %d" % (col + 1, len(lane)))
        return MD_LETTERS[int(lane[col]) & 15]
    text, nm = md_walk(letter, int(ref_first) - 1, [(int(w) >> 4, OP_CHAR[int(w) & 15]) for w in ops])
    return text.encode(), nm


def md_batch(lanes, requests_refix, ref_first, op_off, ops):
    """the model of a whole bhip_md_tags call: (md bytes, md_off list, nm list); lanes[refIx] = the lane's codes"""
    md, off, nms = [], [0], []
    for i, r in enumerate(requests_refix):
        t, nm = md_codes(lanes[int(r)], ref_first[i], ops[int(op_off[i]):int(op_off[i + 1])])
        md.append(t)
        off.append(off[-1] + len(t))
        nms.append(nm)
    return b"".join(md), off, nms


def fasta(path):
    """[(header line without '>', sequence as the loader codes it: upper case, U as T)] in file order"""
    out = []
    for ln in open(path):
        ln = ln.rstrip("\r\n")
        if ln.startswith(">"):
            out.append([ln[1:], []])
        elif out:
            out[-1][1].append(ln.upper().replace("U", "T"))
    return [(h, "".join(s)) for h, s in out]


def name_of(header):
    return WS.split(header, 1)[0]


def seq_text(seq):
    """SEQ of a read: letters outside the alphabet are what the loader reads them as"""
    return "".join(c if c in SEQ_LETTERS[1:] else "N" if c.isalpha() else "." for c in seq)


def revcomp(seq):
    return "".join(COMP.get(c, "N") for c in reversed(seq))


def header_lines(sq):
    """sq: [(reference header, length)] in the order of the database's header numbers"""
    return ["@HD\tVN:1.6\tSO:unknown\tGO:query"] + ["@SQ\tSN:%s\tLN:%d" % (name_of(h), n) for h, n in sq] + ["@PG\tID:burst_hip\tPN:burst_hip"]


def sq_of(refs, lengths=None):
    """the @SQ entries of a database made from the references `refs` (fasta()): its unique headers in the order of their numbers -- strcmp
    order of the whole header -- each with lengths[header] or, by default, the length of its sequence (the database's own extent)"""
    seqs = dict(refs)
    return [(h, int(lengths[h]) if lengths else len(seqs[h])) for h in sorted(seqs, key=lambda s: s.encode())]


def expected_sam(b6_cigar_text, queries, refs, sq, unmapped=False):
    """the whole file.  b6_cigar_text: the output of a run with --cigar (text); queries: fasta() of the query file; refs: fasta() of the
    references; sq as for header_lines"""
    qseq = dict(queries)
    assert len(qseq) == len(queries), "the model takes the reads' names as distinct"
    rseq = dict(refs)
    out = header_lines(sq)
    seen, prev = set(), None
    for ln in b6_cigar_text.split("\n"):
        if not ln:
            continue
        f = ln.split("\t")
        st, en, cigar, pos = int(f[8]), int(f[9]), f[-1], int(f[-2])
        items = [(int(n), c) for n, c in re.findall(r"(\d+)([=XID])", cigar)]
        flag = (0x10 if st > en else 0) | (0x100 if f[0] == prev else 0)
        assert f[0] == prev or f[0] not in seen, "the lines of a read are consecutive"
        prev = f[0]
        seen.add(f[0])
        seq = qseq[f[0]]
        if st > en:
            seq = revcomp(seq)
        ref = rseq[f[1]]
        md, nm = md_walk(lambda col: ref[col] if ref[col] in MD_LETTERS[1:] else "N", pos - 1, items)
        out.append("\t".join([name_of(f[0]), str(flag), name_of(f[1]), str(pos), "255", cigar, "*", "0", "0", seq_text(seq), "*", "NM:i:%d" % nm, "MD:Z:" + md]))
    if unmapped:
        for h, s in queries:
            if h not in seen:
                out.append("\t".join([name_of(h), "4", "*", "0", "0", "*", "*", "0", "0", seq_text(s), "*"]))
    return "\n".join(out) + "\n"


def records(sam_text):
    """the record lines of a SAM file as lists of fields"""
    return [ln.split("\t") for ln in sam_text.split("\n") if ln and not ln.startswith("@")]


def apply_md(seq, pos, cigar, md):
    """the reference letters a record claims, independent of md_walk: {0-based reference column: letter} at every X and D column, from
    walking CIGAR and MD together; also checks that the two agree in their lengths"""
    items = [(int(n), c) for n, c in re.findall(r"(\d+)([=XID])", cigar)]
    toks = re.findall(r"(\d+)|(\^[A-Z]+)|([A-Z])", md)
    # the MD as a per-reference-column list: None = match, a letter = the reference base under an X or a D
    cols = []
    for num, dele, sub in toks:
        if num:
            cols += [None] * int(num)
        elif dele:
            cols += [("D", c) for c in dele[1:]]
        else:
            cols.append(("X", sub))
    out, x, k = {}, pos - 1, 0
    for n, c in items:
        if c == "I":
            continue
        for _ in range(n):
            assert k < len(cols), "the MD string is shorter than the CIGAR's reference span"
            if c == "=":
                assert cols[k] is None
            else:
                assert cols[k] is not None and cols[k][0] == c, (cigar, md, k)
                out[x] = cols[k][1]
            x += 1
            k += 1
    assert k == len(cols), "the MD string is longer than the CIGAR's reference span"
    return out
