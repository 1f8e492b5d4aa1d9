"""The graphs the clustering tests share (tests/test_cluster_cpu.py against the model, tests/test_gpu_cluster.py against bh_cluster_host):
(weights, edges) with edges as rows (q, r, edits), the smallest shapes at which each step of bhip_cluster_run can go wrong."""
import numpy as np

WMAX = 2 ** 32 - 1


def chain(n, reverse=False):
    """i -> i - 1: roles alternate and every node waits for the one before it; reverse: the weights turn the priorities round, so that
    every edge points towards LOWER priority and all nodes are centroids -- with the edges i - 1 -> i added the chain runs the other way"""
    w = [1] * n if not reverse else [i + 1 for i in range(n)]
    e = [(i, i - 1, i % 3) for i in range(1, n)]
    if reverse:
        e += [(i - 1, i, i % 3) for i in range(1, n)]
    return w, e


def star(deg, where):
    """node 0 (lowest priority) has edges to `deg` targets, all of which are members of hub H except (where = 'last' / 'first') the one
    that is last / first in node 0's run, which is a centroid; 'absent': all targets are members, so node 0 is a centroid"""
    # nodes: 0 = the star's centre (weight 1), 1 = hub H (weight 4), 2 .. deg + 1 = targets
    n = deg + 2
    w = [1, 4] + [2] * deg
    e = [(0, t, 5) for t in range(2, n)]
    for t in range(2, n):
        e.append((t, 1, 1))                    # every target joins the hub ...
    lone = {"last": n - 1, "first": 2, "absent": None}[where]
    if lone is not None:
        e = [x for x in e if not (x[0] == lone and x[1] == 1)]      # ... but one, which stays a centroid
        if where == "first":
            w[lone] = 3                        # first in the run = highest priority among the targets
    return w, e


def random_graph(seed, n=2000, m=20000):
    """sparse random edges, 10 % of them repeated with other edits, weights 1 .. 4"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 5, size=n)
    base = m * 9 // 10
    q = rng.integers(0, n, size=base)
    r = (q + rng.integers(-3, 4, size=base)) % n      # neighbours in number: families
    far = rng.random(base) < 0.02
    r[far] = rng.integers(0, n, size=int(far.sum()))
    ed = rng.integers(0, 6, size=base)
    dup = rng.integers(0, base, size=m - base)
    q, r, ed = np.concatenate([q, q[dup]]), np.concatenate([r, r[dup]]), np.concatenate([ed, rng.integers(0, 6, size=m - base)])
    return [int(x) for x in w], list(zip(q.tolist(), r.tolist(), ed.tolist()))


RANDOM_SEEDS = (1, 2, 3)

CASES = {
    "no_edges": ([1, 1, 1, 1, 1], []),
    "one_node": ([1], []),
    "one_node_self": ([7], [(0, 0, 2)]),
    "self_only": ([1, 2, 3], [(0, 0, 1), (1, 1, 0), (2, 2, 4)]),
    "lower_priority_only": ([1, 1, 1, 1], [(0, 1, 0), (0, 3, 1), (1, 2, 0), (2, 3, 2)]),      # equal weights: a smaller number never joins a larger one
    "chain300": chain(300),
    "chain300_reversed": chain(300, reverse=True),
    "five_times": ([1, 1], [(1, 0, 4), (1, 0, 2), (1, 0, 9), (1, 0, 3), (1, 0, 2)]),
    "equal_edits_earlier_wins": ([1, 1, 1], [(2, 1, 3), (2, 0, 3)]),
    "nearer_later_wins": ([1, 1, 1], [(2, 0, 5), (2, 1, 1)]),
    "weight_ties_by_number": ([2, 2, 2, 1], [(0, 1, 0), (1, 0, 0), (2, 1, 1), (1, 2, 1), (3, 2, 0), (3, 0, 0)]),
    "weights_1_and_max": ([1, WMAX, 1, WMAX], [(0, 1, 1), (1, 0, 1), (3, 1, 2), (1, 3, 2), (2, 3, 0)]),
    "directed": ([1, 1, 1], [(0, 1, 0), (2, 1, 0)]),      # 0 -> 1 without 1 -> 0: 0 comes first and stays a centroid, 1 has no edge and is one, 2 joins 1
}
for _deg in (63, 64, 65, 1000):
    for _where in ("last", "first", "absent"):
        CASES["star%d_%s" % (_deg, _where)] = star(_deg, _where)
