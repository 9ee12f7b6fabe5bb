"""FurtherCompressNode's walk cut at independent windows (sq_compress_windows_on_device, squid_amd/csrc/sq_compress_stage.inc) on the CPU.

The rule: node 0 and every first node of a chromosome start a window.  A node i behind them starts one exactly when
  * run(i) < i: no concordant edge of a node behind the last discordant node p in front of i (p itself left out; from the chromosome's first
    node when there is no p) touches i or a node behind i, and
  * not (p and the first discordant node q at or behind i both exist on this chromosome and q - p < 20).
What the route rests on: the reference's walk (SegmentGraph.cpp:2693-2892) arrives at such a node with curNode == MergeNode[i - 1] + 1,
rightmost == i and MergeNode[i] unset -- the state of a walk that starts there, up to the ids in front.  Checked here, in this file's own
words: a restatement of the walk over a node range that records the state on arrival at every node (`walk`), the rule (`rule`), the
state (1, 0, -1) at every cut, the windows' ids behind their offsets against the whole walk's, the whole walk against the literal of
test_literal_loops.py, and the cut kernels' source on the CPU (tools/fc_windows_emu.cpp) against `rule`, table for table.  The GPU file
(tests/test_fc_windows_gpu.py) takes graphs, rule and walk from here."""
import random
import subprocess

import pytest

import graphs
import oracle_util as ou
import test_literal_loops as ll

REACH = 20  # the literal `i + 20` of SegmentGraph.cpp:2750 (not Concord_Dist_Idx)
FCW_TILE = 1024  # fcw::TILE: the nodes of one wave of the cut kernels
SCAN_TILE = 4096  # the tile of the library's device scan (window count, id offsets)


# ------------------------------------------------------------------------------------------------ the graph as the stage reads it
class Lists:
    """per node: its discordant edges, Head list first, then Tail list, each in edge order; the farthest node its concordant edges touch"""

    def __init__(self, nodes, edges, dp, di):
        n = len(nodes)
        self.n, self.di = n, di
        self.chr = [v[0] for v in nodes]
        self.nodes = nodes
        head, tail = [[] for _ in range(n)], [[] for _ in range(n)]
        self.maxfar = [-1] * n
        for e in edges:
            a, ha, b, hb = e[:4]
            A, B = nodes[a], nodes[b]
            disc = A[0] != B[0] or (B[1] - A[1] - A[2] > dp and b - a > di) or ha != 0 or hb != 1  # IsDiscordant, :159-168
            if disc:
                (head if ha else tail)[a].append((a, ha, b, hb))
                (head if hb else tail)[b].append((a, ha, b, hb))
            else:
                self.maxfar[a] = max(self.maxfar[a], b)
                self.maxfar[b] = max(self.maxfar[b], b)
        self.disc = [head[v] + tail[v] for v in range(n)]
        self.hasdisc = [1 if d else 0 for d in self.disc]


def rule(L):
    """(flags, stats): flags[i] = 1 where a window starts; stats counts what the family must contain"""
    n = L.n
    first_at_or_behind = [None] * n
    nxt = None
    for v in range(n - 1, -1, -1):
        if L.hasdisc[v]:
            nxt = v
        first_at_or_behind[v] = nxt
        if v == 0 or L.chr[v] != L.chr[v - 1]:
            nxt = None
    flags = [0] * n
    stats = {"cuts": 0, "refused_19": 0, "granted_20": 0, "refused_by_reach": 0, "refused_by_pair": 0}
    p, run = None, -1
    for i in range(n):
        if i == 0 or L.chr[i] != L.chr[i - 1]:
            flags[i] = 1
            p, run = None, -1
        else:
            q = first_at_or_behind[i]
            pair = p is not None and q is not None
            if run >= i:
                stats["refused_by_reach"] += 1
            elif pair and q - p < REACH:
                stats["refused_by_pair"] += 1
                stats["refused_19"] += q - p == REACH - 1
            else:
                flags[i] = 1
                stats["cuts"] += 1
                stats["granted_20"] += pair and q - p == REACH
        if L.hasdisc[i]:
            p, run = i, -1
        else:
            run = max(run, L.maxfar[i])
    return flags, stats


def table(flags):
    return [i for i, f in enumerate(flags) if f] + [len(flags)]


def walk(L, lo, hi, merge, trace=None):
    """the reference's walk over the nodes lo .. hi - 1 from the state of a chromosome start, ids from 0, into merge[lo:hi] (all -1 on entry);
    trace[i] = (curNode - MergeNode[i - 1], rightmost - i, MergeNode[i]) on arrival at i.  Returns the ids used."""
    di, chr_ = L.di, L.chr
    near = lambda x, y: abs(x[0] - y[0]) <= di and abs(x[2] - y[2]) <= di and x[1] == y[1] and x[3] == y[3]
    chroms = lambda x, y: chr_[x[0]] == chr_[y[0]] and chr_[x[2]] == chr_[y[2]]

    def groups(V, anchor, needchr):  # one edge per run of neighbours in the list that continue each other
        out = V[:1]
        for x, y in zip(V, V[1:]):
            same = near(x, y) and (not needchr or chroms(x, y))
            if anchor is not None:
                same = same and ((x[0] == anchor and y[0] == anchor) or (x[2] == anchor and y[2] == anchor))
            if not same:
                out.append(y)
        return out

    def matched(A, B):  # every edge of A has a partner in B and the other way round
        a_ok, b_ok = [False] * len(A), [False] * len(B)
        for k, x in enumerate(A):
            for l, y in enumerate(B):
                if x[2] > y[0] and y[2] > x[0] and chroms(x, y) and near(x, y):
                    a_ok[k] = b_ok[l] = True
        return all(a_ok) and all(b_ok)

    cur, right = 0, lo
    for i in range(lo, hi):
        prev = merge[i - 1] if i > lo else -1
        if trace is not None:
            trace[i] = (cur - prev, right - i, merge[i])
        if i > lo and chr_[i] != chr_[i - 1] and cur == prev:
            cur += 1
        right = max(right, L.maxfar[i])
        mine = L.disc[i]
        if not mine:
            if merge[i] == -1:
                assert i <= right, "a node without discordant edges behind `rightmost` (the reference reads minDisInd2 unset there)"
                merge[i] = cur
                if i == right:
                    cur += 1
                    right += 1
            continue
        bound = min(e[2] if e[0] == i else i + REACH for e in mine)
        fresh = merge[i] == -1
        if fresh and i > lo and cur == prev:
            cur += 1
        j, ahead = i + 1, []
        while j < hi and j < i + REACH and j < bound and chr_[j] == chr_[i]:
            if L.disc[j]:
                ahead = L.disc[j]
                break
            j += 1
        mine = groups(mine, i, False)
        if fresh:
            same = bool(ahead) and matched(mine, groups(ahead, j, True))
        else:
            same = bool(ahead) and matched(groups(mine, None, True), groups(ahead, None, True))
        if same:
            for k in range(i, j + 1):
                merge[k] = cur
        elif fresh:
            merge[i] = cur
            cur += 1
        else:
            cur += 1
        right = i + 1
    return merge[hi - 1] + 1 if hi > lo else 0


def whole_walk(L, trace=None):
    merge = [-1] * L.n
    walk(L, 0, L.n, merge, trace)
    return merge


def windowed_walk(L, win):
    merge = [-1] * L.n
    off = 0
    for lo, hi in zip(win, win[1:]):
        used = walk(L, lo, hi, merge)
        for k in range(lo, hi):
            merge[k] += off
        off += used
    return merge


def merged_nodes(L, merge):
    """the output nodes of the stage: one per run of equal ids"""
    out, i = [], 0
    while i < L.n:
        j = i
        while j + 1 < L.n and merge[j + 1] == merge[i]:
            j += 1
        out.append((L.chr[i], L.nodes[i][1], L.nodes[j][1] + L.nodes[j][2] - L.nodes[i][1]))
        i = j + 1
    return out


def check_graph(g, literal=True):
    """every assertion the rule rests on, for one graph as it enters the stage; returns (window table, stats, merged-away nodes)"""
    p = g["params"]
    L = Lists(g["nodes"], g["edges"], p["dp"], p["di"])
    flags, stats = rule(L)
    trace = [None] * L.n
    merge = whole_walk(L, trace)
    for i in range(1, L.n):
        if flags[i] and L.chr[i] == L.chr[i - 1]:
            assert trace[i] == (1, 0, -1), (g["name"], i, trace[i])
    win = table(flags)
    assert windowed_walk(L, win) == merge, g["name"]
    if literal:
        assert merged_nodes(L, merge) == ll._further_compress_literal(g["nodes"], g["edges"], dist_pos=p["dp"], dist_idx=p["di"], ratio=p["r"])[0], g["name"]
    return win, stats, L.n - (merge[-1] + 1)


# ------------------------------------------------------------------------------------------------ graphs
def _nodes(chroms, ln=100):
    return graphs._tile([(0, [ln] * k) for k in chroms])


def _graph(name, chroms, conc=(), disc=(), **params):
    """enters at FurtherCompressNode.  conc: (a, b) tail -> head on one chromosome (concordant at the default -dp); disc: (a, head a, b, head b)"""
    E = graphs._Edges()
    for a, b in conc:
        E.add(a, 0, b, 1, 3)
    for a, ha, b, hb in disc:
        E.add(a, ha, b, hb, 2)
    return graphs._g(name, _nodes(chroms), E, first=4, **params)


def random_fc_graph(seed):
    """1-3 chromosomes of nodes 100 bases long, a concordant backbone with holes and a few longer concordant edges (discordant ones at the
    smaller -dp / -di), discordant edges with twins at the neighbours so that nodes merge, and in every fourth graph two discordant nodes
    exactly 19 or 20 apart with nothing between them"""
    rng = random.Random(seed)
    p = {"di": rng.choice((0, 2, 20)), "dp": rng.choice((0, 300, 50000))}
    chroms = [rng.randrange(8, 45) for _ in range(rng.randrange(1, 4))]
    n = sum(chroms)
    first = [sum(chroms[:k]) for k in range(len(chroms) + 1)]
    chrom_of = lambda v: max(k for k in range(len(chroms)) if first[k] <= v)
    E = graphs._Edges()
    quiet = None
    if seed % 4 == 0 and max(chroms) >= 24:  # a stretch [s, s + gap] that only its two ends' discordant edges touch
        c = chroms.index(max(chroms))
        gap = rng.choice((REACH - 1, REACH))
        s = first[c] + rng.randrange(0, chroms[c] - gap)
        quiet = (s, s + gap)
    free = lambda v: quiet is None or not quiet[0] <= v <= quiet[1]
    for v in range(n - 1):
        if chrom_of(v) == chrom_of(v + 1) and rng.random() < 0.6 and free(v) and free(v + 1):
            E.add(v, 0, v + 1, 1, rng.randrange(1, 9))
    for _ in range(rng.randrange(0, 4)):
        a = rng.randrange(n - 1)
        b = min(a + rng.randrange(2, 9), first[chrom_of(a) + 1] - 1)
        if b > a and free(a) and free(b) and not (quiet and a < quiet[0] and b > quiet[1]):
            E.add(a, 0, b, 1, 4)
    for _ in range(rng.randrange(1, 4 + n // 12)):
        a, b = sorted((rng.randrange(n), rng.randrange(n)))
        ha, hb = rng.choice(((1, 1), (0, 0), (1, 0), (0, 1)))
        if a == b or not (free(a) and free(b)) or ((ha, hb) == (0, 1) and chrom_of(a) == chrom_of(b)):
            continue
        E.add(a, ha, b, hb, 2)
        for _ in range(rng.randrange(0, 3)):  # twins at the neighbours
            da, db = rng.randrange(0, 3), rng.randrange(0, 3)
            if a + da < b and b + db < n and free(a + da) and free(b + db) and chrom_of(a + da) == chrom_of(a) and chrom_of(b + db) == chrom_of(b):
                E.add(a + da, ha, b + db, hb, 2)
    if quiet:
        for v in quiet:
            other = rng.choice([u for u in range(n) if not quiet[0] - 1 <= u <= quiet[1] + 1] or [0])
            a, b = sorted((v, other))
            if a != b:
                E.add(a, 1, b, 1, 2)
    return graphs._g(f"fc_seed{seed}", _nodes(chroms), E, first=4, r=8, **p)


RANDOM_FAMILY = range(5000, 7400)  # 2 400 graphs


def _hub_in_the_middle(k):
    """three windows on chromosome 0; the middle one holds a node with k discordant edges (FC_CAP = 256: one more hands the graph back)"""
    E = graphs._Edges()
    for a, b in ((0, 3), (6, 9), (12, 15)):
        for v in range(a, b):
            E.add(v, 0, v + 1, 1, 3)
    for j in range(k):
        E.add(7, j % 2, 20 + j // 2, 0, 2)
    return graphs._g(f"hub_{k}_in_a_middle_window", _nodes([20, k // 2 + 3]), E, first=4)


def hand_graphs():
    H = []
    far = lambda v, k=0: (v, 1, 60 + k, 1)  # a discordant edge of node v: its partner lies on chromosome 1 (nodes 60 ..)
    for d in (REACH - 1, REACH):
        H.append(_graph(f"discordant_nodes_{d}_apart", [60, 40], disc=[far(5), far(5 + d, 30)]))
        H.append(_graph(f"discordant_nodes_{d}_apart_chromosome_between", [15, 45, 40], disc=[far(5), far(5 + d, 30)]))
    H.append(_graph("concordant_edge_reaches_i_minus_1_and_i", [30], conc=[(2, 9)]))
    H.append(_graph("reach_of_a_discordant_node_is_dropped", [60, 40], conc=[(5, 12)], disc=[far(5)]))
    H.append(_graph("reach_from_in_front_of_a_discordant_node_is_dropped", [60, 40], conc=[(3, 12)], disc=[far(5)]))
    H.append(_graph("merged_range_then_a_cut", [60, 40], disc=[far(5), far(6, 1)]))
    H.append(_graph("chain_whose_second_step_does_not_merge", [60, 40], disc=[far(5), far(6, 1), (8, 0, 80, 0)]))
    H.append(_graph("windows_of_one_node", [7, 1, 5]))  # (and a chromosome of one node)
    H.append(_graph("first_and_last_node_discordant", [30, 30], disc=[(0, 1, 59, 1), (1, 1, 58, 1)]))
    H.append(_graph("window_starts_at_70", [120, 40], conc=[(v, v + 1) for v in range(69)] + [(70, 74)], disc=[(75, 1, 130, 1), (77, 1, 132, 1), (71, 0, 150, 0)]))
    for tile in (FCW_TILE, SCAN_TILE):
        for n in (tile - 1, tile, tile + 1):
            t = tile - 1
            H.append(_graph(f"nodes_{n}_at_tile_{tile}", [n - 40, 40], conc=[(t - 30, t - 2), (t - 2, t - 1), (t - 1, t), (t, t + 1)][: 4 if n - 40 > t + 1 else 2],
                            disc=[(t - 8, 1, n - 5, 1), (t - 40, 0, n - 9, 0)] + ([(t + 3, 1, n - 3, 1)] if n - 40 > t + 3 else [])))
    H.append(graphs._g("edgeless_131073", _nodes([131073]), [], first=4))
    H.append(_hub_in_the_middle(256))
    H.append(_hub_in_the_middle(257))
    return H


BIG = {"edgeless_131073"}
# what the hand-made graphs are there to show, worked out by hand: name -> (nodes that must start a window, nodes that must not)
EXPECT = {
    "discordant_nodes_19_apart": ([25, 26], list(range(6, 25))),
    "discordant_nodes_20_apart": (list(range(6, 27)), []),
    "discordant_nodes_19_apart_chromosome_between": ([6, 14, 15, 16, 24, 25], []),
    "concordant_edge_reaches_i_minus_1_and_i": ([1, 2, 10, 11], list(range(3, 10))),
    "reach_of_a_discordant_node_is_dropped": ([6, 7, 12, 13], []),
    "reach_from_in_front_of_a_discordant_node_is_dropped": ([3, 6, 7, 12, 13], [4, 5]),
    "merged_range_then_a_cut": ([7, 8], [6]),
    "chain_whose_second_step_does_not_merge": ([9, 10], [6, 7, 8]),
    "windows_of_one_node": (list(range(13)), []),
    "window_starts_at_70": ([70, 78], list(range(1, 70)) + [71, 72, 73, 74, 75, 76, 77]),
}


def stage4_input(built, tmp, seed):
    """a graph of tests/graphs.SEEDS in the form in which it enters FurtherCompressNode (None: the reference's assert ends it earlier)"""
    g = graphs.graph(seed)
    if g["first"] == 4:
        return g
    r = ou.graph_stages(built, graphs.oracle_text(g["nodes"], g["edges"]), tmp, graphs.oracle_flags(g["params"]), g["first"], 3)
    if "compress" not in r:
        return None
    nodes, edges = r["compress"]
    return dict(g, nodes=[tuple(v[:5]) for v in nodes], edges=[tuple(e[:6]) for e in edges], first=4)


@pytest.fixture(scope="module")
def seed_inputs(built, tmp_path_factory):
    """seed -> stage-4 form, computed once (the oracle runs once per graph)"""
    tmp = tmp_path_factory.mktemp("fc_stage4")
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = stage4_input(built, tmp / str(len(cache)), seed)
        return cache[seed]

    return get


@pytest.fixture(scope="module")
def fc_windows_emu(built):
    exe = built / "fc_windows_emu"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(built.parent), "build/fc_windows_emu"], stdout=subprocess.DEVNULL)
    return exe


def emulated_tables(exe, gs):
    """the cut kernels' source on the CPU: one process per (-dp, -di), the graphs one after the other (the processes side by side)"""
    from concurrent.futures import ThreadPoolExecutor

    out = [None] * len(gs)
    by_params = {}
    for k, g in enumerate(gs):
        by_params.setdefault((g["params"]["dp"], g["params"]["di"]), []).append(k)

    def run(item):
        (dp, di), ks = item
        text = "".join(graphs.oracle_text(gs[k]["nodes"], gs[k]["edges"]) for k in ks)
        return subprocess.run([str(exe), "-dp", str(dp), "-di", str(di)], input=text, capture_output=True, text=True, timeout=600)

    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(run, by_params.items()))
    for ks, r in zip(by_params.values(), results):
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(ks)
        for k, line in zip(ks, lines):
            out[k] = [int(x) for x in line.split()]
    return out


# ------------------------------------------------------------------------------------------------ tests
FLOORS = {"cuts": 20000, "merged": 1500, "refused_19": 1, "granted_20": 1, "refused_by_reach": 10000, "refused_by_pair": 3000}


def test_rule_state_and_emulated_kernels_on_the_random_family(fc_windows_emu):
    gs = [random_fc_graph(s) for s in RANDOM_FAMILY]
    total = dict.fromkeys(FLOORS, 0)
    graphs_19 = graphs_20 = 0
    want = []
    for g in gs:
        win, stats, merged = check_graph(g)
        want.append(win)
        for k, v in stats.items():
            total[k] += v
        total["merged"] += merged
        graphs_19 += stats["refused_19"] > 0
        graphs_20 += stats["granted_20"] > 0
    print(f"{len(gs)} graphs, {sum(len(g['nodes']) for g in gs)} nodes, {sum(len(w) - 1 for w in want)} windows: {total}; graphs with q - p == 19 refused: {graphs_19}, == 20 granted: {graphs_20}")
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total)
    assert graphs_19 >= 1 and graphs_20 >= 1
    got = emulated_tables(fc_windows_emu, gs)
    bad = [g["name"] for g, w, e in zip(gs, want, got) if w != e]
    assert not bad, bad[:10]


def test_either_half_of_the_rule_is_needed():
    """with a half of the rule taken away the windows' ids differ from the whole walk's on many graphs of the family: the check above is not vacuous"""
    broken = {"reach": 0, "pair": 0}
    for s in list(RANDOM_FAMILY)[:600]:
        g = random_fc_graph(s)
        L = Lists(g["nodes"], g["edges"], g["params"]["dp"], g["params"]["di"])
        merge = whole_walk(L)
        starts = [i == 0 or L.chr[i] != L.chr[i - 1] for i in range(L.n)]
        p, run, no_reach, no_pair = None, -1, [], []
        nxt, first_q = None, [None] * L.n
        for v in range(L.n - 1, -1, -1):
            nxt = v if L.hasdisc[v] else nxt
            first_q[v] = nxt
            if starts[v]:
                nxt = None
        for i in range(L.n):
            if starts[i]:
                p, run = None, -1
                no_reach.append(1); no_pair.append(1)
            else:
                pair = p is not None and first_q[i] is not None and first_q[i] - p < REACH
                no_reach.append(0 if pair else 1)
                no_pair.append(1 if run < i else 0)
            if L.hasdisc[i]:
                p, run = i, -1
            else:
                run = max(run, L.maxfar[i])
        for name, flags in (("reach", no_reach), ("pair", no_pair)):
            try:
                same = windowed_walk(L, table(flags)) == merge
            except AssertionError:
                same = False
            broken[name] += not same
    print(broken)
    assert broken["reach"] >= 100 and broken["pair"] >= 100, broken


def test_hand_made_graphs(fc_windows_emu):
    gs = hand_graphs()
    assert set(EXPECT) <= {g["name"] for g in gs}
    want = []
    for g in gs:
        win, _, _ = check_graph(g, literal=g["name"] not in BIG)
        want.append(win)
        if g["name"] in EXPECT:
            yes, no = EXPECT[g["name"]]
            assert set(yes) <= set(win) and not set(no) & set(win), (g["name"], win)
        if g["name"] == "edgeless_131073":
            assert win == list(range(131074))
    by_name = {g["name"]: w for g, w in zip(gs, want)}
    assert by_name["window_starts_at_70"][1] == 70  # (the second window starts at a node index that is no multiple of 64)
    assert 7 not in by_name["hub_257_in_a_middle_window"] and 6 in by_name["hub_257_in_a_middle_window"] and 10 in by_name["hub_257_in_a_middle_window"]
    assert emulated_tables(fc_windows_emu, gs) == want


def test_seed_list_graphs_as_they_enter_the_stage(fc_windows_emu, seed_inputs):
    gs = [g for g in (seed_inputs(s) for s in graphs.SEEDS) if g is not None]
    assert len(gs) >= len(graphs.SEEDS) * 8 // 10
    want = []
    cuts = 0
    for g in gs:
        win, stats, _ = check_graph(g)
        cuts += stats["cuts"]
        want.append(win)
    print(f"{len(gs)} graphs of the seed list enter the stage, {cuts} in-chromosome cuts")
    assert cuts >= 1000
    assert emulated_tables(fc_windows_emu, gs) == want
