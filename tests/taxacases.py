"""The hand case of the taxon tables' definition (tests/test_taxa_cpu.py, tests/test_gpu_taxa.py), written out in full.

Strings a;b;c, a;b;d, a;e, f give the nodes (siblings in byte order)
    0 root   1 a   2 a;b   3 a;b;c   4 a;b;d   5 a;e   6 f
headers h0 a;b;c, h1 a;b;d, h2 a;e, h3 f, h4 none (root), h5 a;b;c
groups  g0 {h0} of 3 reads, g1 {h0, h1}, g2 {h0, h5, h1}, g3 {h0, h2, h3}, g4 {h0, h4}, g5 h0 on two lines, g6 no lines, 9 reads"""

STRINGS = ["a;b;c", "a;b;d", "a;e", "f", "", "a;b;c"]
NAMES = ["Unassigned", "a", "a;b", "a;b;c", "a;b;d", "a;e", "f"]
PARENT = [0, 0, 1, 2, 2, 1, 0]
DEPTH = [0, 1, 2, 3, 3, 2, 1]
HEADER_NODE = [3, 4, 5, 6, 0, 3]
GROUP_W = [3, 1, 1, 1, 1, 1, 9]
LINES = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 5), (2, 1), (3, 0), (3, 2), (3, 3), (4, 0), (4, 4), (5, 0), (5, 0)]
X = 0xFFFFFFFF

# agree -> (group_node, own, clade, info[0..4] = pairs, groups with lines, their reads, reads at the root, deepest level)
EXPECT = {
    #        g0 g1 g2 g3 g4 g5 g6       root a  a;b a;b;c a;b;d a;e f
    1000: ([3, 2, 2, 0, 0, 3, X], [2, 0, 2, 4, 0, 0, 0], [8, 6, 6, 4, 0, 0, 0], [12, 6, 8, 2, 3]),
    667:  ([3, 2, 2, 0, 0, 3, X], [2, 0, 2, 4, 0, 0, 0], [8, 6, 6, 4, 0, 0, 0], [12, 6, 8, 2, 3]),      # t = 3 of 3, 2 of 2
    666:  ([3, 2, 3, 1, 0, 3, X], [1, 1, 1, 5, 0, 0, 0], [8, 7, 6, 5, 0, 0, 0], [12, 6, 8, 1, 3]),      # t = 2 of 3: g2 at a;b;c, g3 at a
    600:  ([3, 2, 3, 1, 0, 3, X], [1, 1, 1, 5, 0, 0, 0], [8, 7, 6, 5, 0, 0, 0], [12, 6, 8, 1, 3]),
    501:  ([3, 2, 3, 1, 0, 3, X], [1, 1, 1, 5, 0, 0, 0], [8, 7, 6, 5, 0, 0, 0], [12, 6, 8, 1, 3]),      # g4 stays at the root: t = 2 of 2
}
