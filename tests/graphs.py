"""Seed -> segment graph for the small-graph stages (FilterbyWeight .. MultiplyDisEdges): random graphs and hand-made ones.

A graph is a dict: nodes [(chr, pos, len, support, avgdepth)], edges [(ind1, head1, ind2, head2, weight)] sorted by Edge_t::operator<,
params {dp, di, w, a, r} (the -dp -di -w -a -r of the command line), `first` (the stage it enters at, 0 = FilterbyWeight .. 4 =
FurtherCompressNode) and `name`.  `SEEDS` is the committed list: random seeds (ints) and the names of the hand-made graphs; `graph(seed)`
makes either.  Only `random.Random(seed)` is used, so a seed gives the same graph everywhere.

Self-edges (ind1 == ind2): `edges_build.txt` of the oracle's dumps of C1 (54 edges), T2 (124 edges) and C5g (--records 200000 --tsv 400,
-w 1 -a 50; 4992 edges) holds none -- RawEdgesChim / RawEdgesOther skip i == j -- so the generator makes none either.
"""
import random

DEFAULT = {"dp": 50000, "di": 20, "w": 5, "a": 5, "r": 8}


def ctx_params(p):
    """keyword arguments of squid_amd.Context for the graph's parameters"""
    return {"concord_dist_pos": p["dp"], "concord_dist_idx": p["di"], "min_edge_weight": p["w"], "max_allowed_degree": p["a"], "discordant_ratio": float(p["r"])}


def oracle_flags(p):
    return ["-dp", str(p["dp"]), "-di", str(p["di"]), "-w", str(p["w"]), "-a", str(p["a"]), "-r", str(p["r"])]


def oracle_text(nodes, edges, keep=None):
    """stdin of `squid_oracle --graph-stages`; edges may carry a group weight (6th field); keep: the KeepEdge column"""
    out = [f"{len(nodes)} {len(edges)}"]
    out += [f"{n[0]} {n[1]} {n[2]} {n[3]} {float(n[4]).hex()}" for n in nodes]
    for i, e in enumerate(edges):
        row = list(e[:5]) + [e[5] if len(e) > 5 else 0] + ([int(bool(keep[i]))] if keep is not None else [])
        out.append(" ".join(str(int(x)) for x in row))
    return "\n".join(out) + "\n"


class _Edges:
    """edge set keyed like Edge_t (smaller node first, heads swapped along), equal keys summed (BuildEdges)"""

    def __init__(self):
        self.w = {}

    def add(self, a, ha, b, hb, w):
        if a == b:
            return
        if a > b:
            a, ha, b, hb = b, hb, a, ha
        k = (a, b, ha, hb)
        self.w[k] = self.w.get(k, 0) + w

    def rows(self):
        return [(a, ha, b, hb, w) for (a, b, ha, hb), w in sorted(self.w.items())]


def _tile(chroms, depth=lambda i: 10.0, support=lambda i: 1):
    """nodes that tile chromosomes: chroms = [(start position, [lengths])]"""
    nodes = []
    for c, (pos, lens) in enumerate(chroms):
        for ln in lens:
            nodes.append((c, pos, ln, support(len(nodes)), depth(len(nodes))))
            pos += ln
    return nodes


def _g(name, nodes, edges, first=0, **params):
    p = dict(DEFAULT)
    p.update(params)
    rows = edges.rows() if isinstance(edges, _Edges) else sorted(edges, key=lambda e: (e[0], e[2], e[1], e[3]))
    return {"name": name, "nodes": nodes, "edges": rows, "params": p, "first": first}


# ------------------------------------------------------------------------------------------------ random graphs
def random_graph(seed):
    rng = random.Random(seed)
    p = {"dp": rng.choice((50000, 1000)), "di": rng.choice((20, 3)), "w": rng.choice((1, 2, 5)), "a": rng.choice((5, 50)), "r": 8}
    r = rng.random()
    n = rng.randrange(40, 120) if r < 0.6 else rng.randrange(120, 300) if r < 0.9 else rng.randrange(300, 601)
    nchr = rng.choice((1, 2, rng.randrange(5, 9)))
    cuts = sorted(rng.sample(range(1, n), nchr - 1))
    chr_, pos, ln, sup, dep = [], [], [], [], []
    for c, (lo, hi) in enumerate(zip([0] + cuts, cuts + [n])):
        at = rng.choice((0, rng.randrange(0, 2000000), rng.randrange(200000000, 235000000)))  # (hg38: chr1 ends at 2.49e8)
        for _ in range(lo, hi):
            k = rng.random()
            length = rng.randrange(1, 301) if k < 0.45 else rng.randrange(300, 5001) if k < 0.9 else rng.randrange(20000, 60001)
            k = rng.random()
            prev = dep[-1] if dep else 7.0
            d = 0.0 if k < 0.08 else prev * 3.0 if k < 0.14 else prev * 50.0 if k < 0.18 else prev / 3.0 if k < 0.22 else rng.random() * 40
            chr_.append(c); pos.append(at); ln.append(length); sup.append(rng.randrange(0, 60)); dep.append(d if d < 1e6 else rng.random() * 40)
            at += length
    w = p["w"]

    def weight():
        if rng.random() < 0.65:
            return max(1, rng.choice((w - 2, w, w + 2)) + rng.randrange(-1, 2))
        return rng.randrange(6, 60)

    E = _Edges()
    holes = [(s, s + rng.randrange(2, 16)) for s in (rng.randrange(n) for _ in range(rng.randrange(0, 4)))]
    for i in range(n - 1):  # concordant backbone with gaps
        if chr_[i] == chr_[i + 1] and rng.random() < 0.85 and not any(lo <= i < hi for lo, hi in holes):
            E.add(i, 0, i + 1, 1, rng.randrange(1, 80))
    clamp = lambda v: min(max(v, 0), n - 1)
    planted = []
    for _ in range(rng.randrange(2, 4 + n // 15)):  # discordant clusters between two regions
        c1, c2 = rng.randrange(n), rng.randrange(n)
        pat = (rng.randrange(2), rng.randrange(2))
        for _ in range(rng.randrange(1, 9)):
            a, b = clamp(c1 + rng.randrange(-3, 4)), clamp(c2 + rng.randrange(-3, 4))
            k = rng.random()
            ha, hb = pat if k < 0.8 else (1 - pat[0], 1 - pat[1]) if k < 0.9 else (rng.randrange(2), rng.randrange(2))
            E.add(a, ha, b, hb, weight())
            planted.append((a, b))
    for a, b in rng.sample(planted, min(len(planted), rng.randrange(0, 5))):  # parallel edges of several head patterns
        for _ in range(rng.randrange(1, 4)):
            E.add(a, rng.randrange(2), b, rng.randrange(2), weight())
    for _ in range(rng.randrange(0, 3)):  # hubs: nodes with many neighbour groups (MaxAllowedDegree, GroupSelect)
        h, side = rng.randrange(n), rng.randrange(2)
        for _ in range(rng.randrange(2, 9)):
            b = rng.randrange(n)
            E.add(h, side if rng.random() < 0.8 else 1 - side, b, rng.randrange(2), rng.randrange(8, 40))
            planted.append((h, b))
    for a, b in planted:  # depths at the ends of some discordant edges: 0 / 0, the thresholds 3 and 50 exactly, just above, equal
        k = rng.random()
        if k < 0.06:
            dep[a] = dep[b] = 0.0
        elif k < 0.12:
            dep[b] = dep[a] * 3.0
        elif k < 0.16:
            dep[b] = dep[a] * 50.0
        elif k < 0.20:
            dep[b] = dep[a] * 3.0000000000000004
        elif k < 0.45:
            dep[b] = dep[a] * (0.5 + rng.random())
    nodes = list(zip(chr_, pos, ln, sup, dep))
    return _g(f"seed{seed}", nodes, E, **p)


# ------------------------------------------------------------------------------------------------ hand-made graphs
def _window_cut(gap, filler, conc=False, pats=((0, 0), (0, 0))):
    """two discordant clusters on chromosome 0 whose Ind1 nodes are `gap` bases apart (end of node 4 to start of the second cluster's first
    node), the partners side by side on chromosome 1; `filler` nodes in the gap, joined by concordant edges with conc"""
    dp = 1000
    fl = [gap // filler + (1 if k < gap % filler else 0) for k in range(filler)]
    nodes = _tile([(1000, [40, 40, 40, 40, 40] + fl + [40, 40, 40, 700]), (5000, [30] * 12)])
    n0 = 5 + filler + 4
    E = _Edges()
    for i, a in enumerate((2, 3, 4)):
        E.add(a, pats[0][0], n0 + 2 + i, pats[0][1], 2 + i)
    # (opposite patterns: the partners of the second cluster lie more than -di above the first one's, so only the UPWARD walk from the first
    # cluster can join the two -- its opposite class tests the seed's Ind2, ledger B14 -- and the group weights show whether it got across)
    far = 8 if pats[0] != pats[1] else 5
    for i, a in enumerate((5 + filler, 6 + filler)):
        E.add(a, pats[1][0], n0 + far + i, pats[1][1], 3 + i)
    if conc:
        for a in range(4, 5 + filler):
            E.add(a, 0, a + 1, 1, 9)
    return nodes, E, {"dp": dp, "di": 3, "w": 2, "a": 50}


def _window_cut_interleave(gap):
    """the same two clusters with heads chosen so that FilterbyInterleaving deletes all four edges exactly when its upward walk gets across
    the gap: only the joined group has Head and Tail partners on both sides whose index ranges overlap (:2264-2273), and the partner of the
    edge at node 4 lies too low for the downward walk from the second cluster to take it"""
    nodes = _tile([(1000, [40, 40, 40, 40, 40, gap, 40, 40, 40, 700]), (5000, [30] * 12)])
    E = _Edges()
    for a, ha, b, hb in ((3, 0, 18, 0), (4, 0, 11, 1), (6, 1, 16, 0), (7, 1, 17, 1)):
        E.add(a, ha, b, hb, 6)
    return nodes, E, {"dp": 1000, "di": 3, "w": 2, "a": 50}


def _chrom_edge():
    """a cluster that ends on the last node of chromosome 0, another that starts on the first node of chromosome 1"""
    nodes = _tile([(0, [50] * 8), (0, [50] * 8), (0, [50] * 10)])
    E = _Edges()
    for k, a in enumerate((5, 6, 7)):
        E.add(a, 0, 18 + k, 0, 3)
    for k, a in enumerate((8, 9, 10)):
        E.add(a, 0, 20 + k, 0, 4)
    return nodes, E, {"dp": 1000, "di": 3, "w": 2, "a": 50}


def _ballot(spaced, dense, di=3):
    """`spaced` discordant edges whose Ind1 nodes lie di + 2 apart (the upward walk of FilterbyWeight / FilterbyInterleaving stops on the
    index, the downward walk -- ledger B14 -- does not: each is collected by every later seed), then `dense` edges on consecutive nodes
    (one seed collects them all upwards).  The partners sit on chromosome 1, eight edges to a node, so no list passes FC_CAP."""
    step = di + 2
    n0 = spaced * step + dense + 2
    m = spaced + dense
    nodes = _tile([(0, [7] * n0), (100000, [11] * (m // 8 + 3))], depth=lambda i: 4.0 + (i % 5))
    E = _Edges()
    for k in range(m):
        a = k * step if k < spaced else spaced * step + (k - spaced)
        E.add(a, 0, n0 + k // 8, 0, 1 + k % 3)
    return nodes, E, {"dp": 50000, "di": di, "w": 2, "a": 50}


def _fc_cap(k, front):
    """enters at FurtherCompressNode: a hub whose Head and Tail lists together hold k discordant edges; front: the node in front of the hub
    has a discordant edge of its own, so the hub's list is also collected as that node's `next` list"""
    hub = 2
    nodes = _tile([(0, [100] * 6), (0, [100] * (k // 2 + 3))])
    E = _Edges()
    for j in range(k):
        E.add(hub, j % 2, 6 + j // 2, 0, 2)
    if front:
        E.add(hub - 1, 0, 6, 0, 2)
    return _g(f"fc_cap_{k}{'_front' if front else ''}", nodes, E, first=4)


def _sparse(n, seed, run=None):
    """n nodes, few edges: long runs of unlinked nodes for the run-head scans of the two compressions; run = (lo, hi): no edge touches
    the nodes lo .. hi - 1"""
    rng = random.Random(seed)
    lens = [rng.randrange(400, 1200) for _ in range(n)]
    half = n // 2 + rng.randrange(-3, 4)
    nodes = _tile([(0, lens[:half]), (0, lens[half:])], depth=lambda i: (i * 37 % 101) / 7.0, support=lambda i: i % 13)
    E = _Edges()
    free = lambda v: run is None or not run[0] <= v < run[1]
    for _ in range(max(8, n // 60)):
        a = rng.randrange(n - 1)
        k = rng.random()
        if k < 0.5:
            if nodes[a][0] == nodes[a + 1][0] and free(a) and free(a + 1):
                E.add(a, 0, a + 1, 1, rng.randrange(4, 30))
        else:
            b = rng.randrange(n)
            if free(a) and free(b):
                E.add(a, rng.randrange(2), b, rng.randrange(2), rng.randrange(4, 30))
    for v in (0, n - 2):  # the first and the last node carry an edge, the run in front of the last linked node is a whole tile long
        if free(v) and free(v + 1):
            E.add(v, 1, v + 1, 1, 9)
    return nodes, E, {"dp": 50000, "di": 20, "w": 2, "a": 50}


def _path(n, zigzag):
    """one component of n nodes, every edge discordant by its heads (enters at FurtherCompressNode, which merges none of them: -di 0, and the
    edges of neighbouring nodes differ in their heads); zigzag: the path runs 0, n-1, 1, n-2, ... so the unions of the component kernel join
    far-apart nodes, and the sorted edge list visits the path from both ends towards the middle"""
    nodes = _tile([(0, [300] * n)])
    E = _Edges()
    if zigzag:
        for i in range(n // 2):
            E.add(i, i % 2, n - 1 - i, i % 2, 3)
            if i + 1 < n - 1 - i:
                E.add(i + 1, (i + 1) % 2, n - 1 - i, (i + 1) % 2, 3)
    else:
        for i in range(n - 1):
            E.add(i, 1, i + 1, 1, 3)
    return _g(f"path_{n}{'_zigzag' if zigzag else ''}", nodes, E, first=4, di=0)


def _star(leaves):
    nodes = _tile([(0, [300] * 40), (0, [300] * (leaves + 5))])
    E = _Edges()
    for k in range(leaves):
        E.add(20, k % 2, 42 + k, 1, 2)
    return _g(f"star_{leaves}", nodes, E, first=4)


def _pairs(k):
    nodes = _tile([(0, [300] * (2 * k))])
    E = _Edges()
    for i in range(k):
        E.add(2 * i, 1, 2 * i + 1, 1, 2)
    return _g(f"pairs_{k}", nodes, E, first=4)


def _hand():
    H = {}

    def put(g):
        H[g["name"]] = g

    for gap in (999, 1000, 1001):
        for nm, kw in (("", {}), ("_mixed", {"pats": ((0, 0), (1, 1))}), ("_conc", {"conc": True}), ("_conc_mixed", {"conc": True, "pats": ((0, 0), (1, 1))})):
            nodes, E, p = _window_cut(gap, 2 if "conc" in nm else 1, **kw)
            put(_g(f"window_gap_{gap}{nm}", nodes, E, **p))
    for gap in (999, 1000, 1001):
        nodes, E, p = _window_cut_interleave(gap)
        put(_g(f"window_gap_{gap}_interleave", nodes, E, **p))
    nodes, E, p = _chrom_edge()
    put(_g("window_chromosome_edge", nodes, E, **p))
    for k in (63, 64, 65, 128, 129):
        nodes, E, p = _ballot(0, k)
        put(_g(f"ballot_window_{k}", nodes, E, **p))
    for spaced, dense in ((63, 70), (70, 1), (130, 131), (64, 64)):  # (63, 70): the collecting seed is the last edge of its 64-block
        nodes, E, p = _ballot(spaced, dense)
        put(_g(f"ballot_both_sides_{spaced}_{dense}", nodes, E, **p))
    for k in (255, 256, 257):
        put(_fc_cap(k, False))
        put(_fc_cap(k, True))
    for n in (2047, 2048, 2049, 4095, 4096, 4097):
        nodes, E, p = _sparse(n, n)
        put(_g(f"scan_{n}", nodes, E, **p))
    nodes, E, p = _sparse(4500, 7, run=(3800, 4400))
    put(_g("scan_run_across_4096", nodes, E, **p))
    nodes, E, p = _sparse(131073, 11)
    put(_g("scan_131073", nodes, E, **p))
    put(_path(5000, False))
    put(_path(5000, True))
    put(_star(200))
    put(_pairs(2000))
    # degenerate
    put(_g("one_node", _tile([(0, [500])]), []))  # (no edge can exist -- no self-edges: the reference's assert in front of CompressNode)
    rng = random.Random(5)  # (edges too light for -w 5: FilterbyWeight leaves nothing, the same assert)
    put(_g("all_edges_too_light", _tile([(0, [900] * 30)]), [(a, rng.randrange(2), a + rng.randrange(5, 9), rng.randrange(2), 1) for a in range(0, 20, 4)]))
    put(_g("two_nodes_one_edge", _tile([(0, [500, 500])]), [(0, 1, 1, 1, 9)], w=2))
    E = _Edges()
    for ha in (0, 1):
        for hb in (0, 1):
            E.add(3, ha, 9, hb, 6 + ha + 2 * hb)
    put(_g("one_node_pair", _tile([(0, [2000] * 12)], depth=lambda i: 5.0), E, dp=1000, di=3, w=2))
    E = _Edges()
    for a, b in ((1, 2), (2, 3), (0, 3), (13, 14), (12, 15), (1, 14)):
        E.add(a, a % 2, b, 1, 7)
    put(_g("chromosome_without_edges", _tile([(0, [900] * 5), (0, [900] * 6), (0, [900] * 5)], depth=lambda i: 5.0), E, w=2))
    E = _Edges()
    for a in range(12):
        for b in range(a + 1, 12):
            for pat in range(4):
                E.add(a, pat & 1, b, pat >> 1, 3 + (a * 7 + b * 3 + pat) % 9)
    put(_g("more_edges_than_nodes", _tile([(0, [3000] * 6), (0, [3000] * 6)], depth=lambda i: 5.0 + i), E, dp=1000, di=3, w=2, a=50))
    return H


_HAND = None


def hand_graph(name):
    global _HAND
    if _HAND is None:
        _HAND = _hand()
    g = _HAND[name]
    return dict(g, nodes=list(g["nodes"]), edges=list(g["edges"]), params=dict(g["params"]))


HAND_NAMES = (
    [f"window_gap_{gap}{nm}" for gap in (999, 1000, 1001) for nm in ("", "_mixed", "_conc", "_conc_mixed", "_interleave")] + ["window_chromosome_edge"]
    + [f"ballot_window_{k}" for k in (63, 64, 65, 128, 129)] + [f"ballot_both_sides_{s}_{d}" for s, d in ((63, 70), (70, 1), (130, 131), (64, 64))]
    + [f"fc_cap_{k}{f}" for k in (255, 256, 257) for f in ("", "_front")]
    + [f"scan_{n}" for n in (2047, 2048, 2049, 4095, 4096, 4097)] + ["scan_run_across_4096", "scan_131073"]
    + ["path_5000", "path_5000_zigzag", "star_200", "pairs_2000"]
    + ["one_node", "all_edges_too_light", "two_nodes_one_edge", "one_node_pair", "chromosome_without_edges", "more_edges_than_nodes"]
)
RANDOM_SEEDS = list(range(1000, 1200))
SEEDS = RANDOM_SEEDS + HAND_NAMES
BIG = {"scan_131073"}  # (the only graph the per-seed loops treat apart: see the tests)


def graph(seed):
    return random_graph(seed) if isinstance(seed, int) else hand_graph(seed)
