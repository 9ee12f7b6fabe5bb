"""The small-graph stages (FilterbyWeight, FilterbyInterleaving, FilterEdges, CompressNode, FurtherCompressNode, the component labels,
MultiplyDisEdges) on the graphs of tests/graphs.py, by four routes: the Python literals of test_literal_loops.py, the oracle
(`squid_oracle --graph-stages`), the library's host functions and its kernels (`Context.debug_graph_stages`, route 0 / 1).

CPU: oracle == literals on every seed, stage by stage, and the seed list's coverage counted from those two alone.  GPU: kernels == host
functions == literals; the depth-bounds box rule of FilterEdges; graphs that enter at a later stage.  Integers and doubles are compared
for equality everywhere."""
import random
import time

import pytest

import graphs
import oracle_util as ou
import test_literal_loops as ll


# ------------------------------------------------------------------------------------------------ the four routes, one result shape
# {"weight": [(ind1, head1, ind2, head2, weight, groupweight)], "keep": [bool], "filter": [6-tuples], "assert": line,
#  "compress": ([(chr, pos, len, support, depth)], [6-tuples]), "final": ([(chr, pos, len)], [label], [(ind1, head1, ind2, head2, weight)])}
def literal_route(g, first=None, last=4, edges=None, keep=None, nodes=None, trace=None):
    p = g["params"]
    first = g["first"] if first is None else first
    nodes = g["nodes"] if nodes is None else nodes
    edges = [tuple(e[:5]) + ((e[5],) if len(e) > 5 else (0,)) for e in (g["edges"] if edges is None else edges)]
    d = {"dist_pos": p["dp"], "dist_idx": p["di"]}
    out = {}
    if first <= 0 <= last:
        edges = ll._filter_by_weight_literal(nodes, edges, min_w=p["w"], trace=trace, **d)
        out["weight"] = edges
    if first <= 1 <= last:
        keep = ll._filter_by_interleaving_literal(nodes, edges, **d)
        out["keep"] = keep
    if first <= 2 <= last:
        edges = ll._filter_edges_literal(nodes, edges, keep if keep is not None else [True] * len(edges), min_w=p["w"], max_deg=p["a"], trace=trace, **d)
        out["filter"] = edges
    if first <= 3 <= last:
        if not edges:
            out["assert"] = 2537
            return out
        nodes, edges = ll._compress_node_literal(nodes, edges)
        out["compress"] = (nodes, edges)
    if first <= 4 <= last:
        try:
            fn, label, fe, _ = ll._further_compress_literal(nodes, edges, ratio=p["r"], **d)
        except AssertionError:
            out["assert"] = 2862
            return out
        out["final"] = (fn, label, fe)
    return out


def oracle_route(built, tmp, g, first=None, last=4, edges=None, keep=None, nodes=None):
    first = g["first"] if first is None else first
    text = graphs.oracle_text(g["nodes"] if nodes is None else nodes, g["edges"] if edges is None else edges, keep)
    r = ou.graph_stages(built, text, tmp, graphs.oracle_flags(g["params"]), first, last)
    out = {k: r[k] for k in ("keep", "assert") if k in r}
    for k in ("weight", "filter"):
        if k in r:
            out[k] = [tuple(e[:6]) for e in r[k]]
    if "compress" in r:
        out["compress"] = ([tuple(n[:5]) for n in r["compress"][0]], [tuple(e[:6]) for e in r["compress"][1]])
    if "final" in r:
        fn, fe = r["final"]
        assert all(n[3] == 0 and n[4] == 0.0 for n in fn)  # (Support / AvgDepth are reset, ledger B15)
        out["final"] = ([tuple(n[:3]) for n in fn], [n[5] for n in fn], [tuple(e[:5]) for e in fe])
    return out


def _view(ctx, stage):
    """ctx.graph(stage) through numpy (a graph of 131 073 nodes, element by element through ctypes, takes seconds)"""
    import ctypes as C

    import numpy as np
    import squid_amd

    g = squid_amd.SqGraph()
    ctx._chk(ctx.lib.sq_graph_view(ctx.h, stage, C.byref(g)), "sq_graph_view")
    col = lambda ptr, k: np.ctypeslib.as_array(ptr, shape=(k,)).tolist() if k else []
    n, m = g.n_nodes, g.n_edges
    nodes = list(zip(col(g.chr, n), col(g.pos, n), col(g.len, n), col(g.support, n), col(g.avgdepth, n), col(g.label, n)))
    edges = list(zip(col(g.ind1, m), col(g.head1, m), col(g.ind2, m), col(g.head2, m), col(g.weight, m), col(g.groupweight, m)))
    return nodes, edges


def library_route(ctx, g, route, first=None, last=4, edges=None, keep=None, nodes=None, bounds=False):
    first = g["first"] if first is None else first
    r = ctx.debug_graph_stages(g["nodes"] if nodes is None else nodes, g["edges"] if edges is None else edges, route=route, first=first, last=last, bounds=bounds, keep=keep,
                               **graphs.ctx_params(g["params"]))
    out = {"fallback": r["fallback"], "depth_ambiguous": r["depth_ambiguous"]}
    ran = lambda k: first <= k <= last
    if ran(0):
        out["weight"] = _view(ctx, 3)[1]
    if ran(1):
        out["keep"] = [bool(b) for b in r["keep"]]
    if ran(2):
        out["filter"] = _view(ctx, 4)[1]
    if r["rc"]:
        assert r["rc"] == -6, r  # SQ_E_ASSERT: the only error the entry reports this way
        out["assert"] = 2537 if (ran(3) and not (out["filter"] if ran(2) else (g["edges"] if edges is None else edges))) else 2862
        return out
    if ran(3):
        n5, e5 = _view(ctx, 5)
        out["compress"] = ([n[:5] for n in n5], e5)
    if ran(4):
        fn, fe = _view(ctx, 0)
        assert all(n[3] == 0 and n[4] == 0.0 for n in fn)
        out["final"] = ([n[:3] for n in fn], [n[5] for n in fn], [e[:5] for e in fe])
    return out


STAGE_KEYS = ("weight", "keep", "filter", "assert", "compress", "final")


def _differences(want, got, what):
    """the stages on which two routes differ, as text (empty: none)"""
    bad = []
    for k in STAGE_KEYS:
        if (k in want) != (k in got):
            bad.append(f"{what}: stage {k!r} {'missing' if k in want else 'unexpected'}")
        elif k in want and want[k] != got[k]:
            w, g = want[k], got[k]
            if k == "compress":
                k, w, g = ("compress nodes", w[0], g[0]) if w[0] != g[0] else ("compress edges", w[1], g[1])
            elif k == "final":
                k, w, g = next((f"final {nm}", w[i], g[i]) for i, nm in enumerate(("nodes", "labels", "edges")) if w[i] != g[i])
            if isinstance(w, list) and isinstance(g, list):
                at = next((i for i, (x, y) in enumerate(zip(w, g)) if x != y), min(len(w), len(g)))
                bad.append(f"{what}: {k} differs at row {at} (lengths {len(w)} / {len(g)}): want {w[at:at + 2]} got {g[at:at + 2]}")
            else:
                bad.append(f"{what}: {k}: want {w} got {g}")
    return bad


def _is_disc(nodes, e, p):  # IsDiscordant, SegmentGraph.cpp:159-190
    a, b = nodes[e[0]], nodes[e[2]]
    return a[0] != b[0] or (b[1] - a[1] - a[2] > p["dp"] and e[2] - e[0] > p["di"]) or e[1] != 0 or e[3] != 1


def _longest_discordant_list(nodes, edges, p):
    """the most discordant edges in the Head and Tail lists of one node: past FC_CAP = 256 the FurtherCompressNode kernel hands the graph back"""
    cnt = {}
    for e in edges:
        if _is_disc(nodes, e, p):
            cnt[e[0]] = cnt.get(e[0], 0) + 1
            cnt[e[2]] = cnt.get(e[2], 0) + 1
    return max(cnt.values(), default=0)


@pytest.fixture(scope="module")
def reference():
    """seed -> (graph, the literals' stages, what the literals' trace counted); computed once and shared, never written to"""
    cache = {}

    def get(seed):
        if seed not in cache:
            g = graphs.graph(seed)
            trace = {}
            cache[seed] = (g, literal_route(g, trace=trace), trace)
        return cache[seed]

    return get


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_graph_stages_equal_the_literals(built, reference, tmp_path):
    """every graph of the seed list: the oracle's stage dumps against the literals -- group weights, KeepEdge, the filtered edges, the
    compressed nodes with AvgDepth as the same doubles, the final nodes, labels and multiplied weights; graphs that end with no edge in
    front of CompressNode must report the reference's assert (SegmentGraph.cpp:2537) on both sides"""
    bad = []
    for k, seed in enumerate(graphs.SEEDS):
        g, want, _ = reference(seed)
        bad += _differences(want, oracle_route(built, tmp_path / str(k), g), g["name"])
    assert not bad, "\n".join(bad[:20])


def test_oracle_graph_stages_from_filter_edges_equal_the_literal(built, reference, tmp_path):
    """a graph that enters at FilterEdges with a KeepEdge column of its own (the GPU test below takes the literal as the reference there)"""
    bad = []
    for k, seed in enumerate(graphs.RANDOM_SEEDS[:40]):
        g, ref, _ = reference(seed)
        keep = _random_keep(seed, len(ref["weight"]))
        bad += _differences(literal_route(g, first=2, edges=ref["weight"], keep=keep), oracle_route(built, tmp_path / str(k), g, first=2, edges=ref["weight"], keep=keep), g["name"])
    assert not bad, "\n".join(bad[:20])


def _random_keep(seed, m):
    rng = random.Random(seed * 31 + 5)
    return [rng.random() < 0.7 for _ in range(m)]


COVERAGE_FLOOR = 10  # graphs of the list in which every mechanism must occur


def test_seed_list_coverage(reference):
    """the seed list is not trivial: counted from the literals (their trace) and their agreement with the oracle above, each mechanism of
    the stages occurs in at least COVERAGE_FLOOR graphs, and at most a tenth of the graphs end empty in front of CompressNode"""
    count = dict.fromkeys(("group weight != weight", "long group", "opposite-pattern join", "interleaving deletion", "bad node", "GroupSelect deletion",
                           "depth-ratio deletion", "0/0 ratio kept", "CompressNode merge", "FurtherCompressNode merge", "more than one component"), 0)
    empty = 0
    for seed in graphs.SEEDS:
        g, ref, tr = reference(seed)
        count["group weight != weight"] += any(e[5] != e[4] for e in ref.get("weight", ()))
        count["long group"] += tr.get("long_groups", 0) > 0
        count["opposite-pattern join"] += tr.get("opposite_joins", 0) > 0
        count["interleaving deletion"] += not all(ref.get("keep", ()))
        count["bad node"] += len(tr.get("bad_nodes", ())) > 0
        count["GroupSelect deletion"] += tr.get("group_select_deletions", 0) > 0
        count["depth-ratio deletion"] += tr.get("ratio_deletions", 0) > 0
        count["0/0 ratio kept"] += tr.get("nan_ratio_kept", 0) > 0
        if "compress" in ref:
            count["CompressNode merge"] += len(ref["compress"][0]) < len(g["nodes"])
        if "final" in ref:
            before = ref["compress"][0] if "compress" in ref else g["nodes"]
            count["FurtherCompressNode merge"] += len(ref["final"][0]) < len(before)
            count["more than one component"] += max(ref["final"][1]) > 0
        empty += ref.get("assert") == 2537
    print("coverage over", len(graphs.SEEDS), "graphs:", count, "empty:", empty)
    assert all(v >= COVERAGE_FLOOR for v in count.values()), count
    assert 0 < empty <= len(graphs.SEEDS) // 10, empty


@pytest.mark.parametrize("cfg", ["C1", "T2"])
def test_graph_stages_mode_reproduces_a_normal_run(built, synth, tmp_path, cfg):
    """`--graph-stages` over the nodes_build / edges_build of a normal oracle run writes that run's stage dumps, byte for byte"""
    _, dump = ou.run_oracle(built, synth(cfg), tmp_path)
    text = graphs.oracle_text(ou.read_nodes(dump / "nodes_build.txt"), ou.read_edges(dump / "edges_build.txt"))
    r = ou.graph_stages(built, text, tmp_path / "again", graphs.oracle_flags(graphs.DEFAULT))
    assert "assert" not in r and len(r["final"][1]) > 0
    for f in ("edges_weight.txt", "edges_interleave.txt", "edges_filter.txt", "nodes_compress.txt", "edges_compress.txt", "nodes_final.txt", "edges_final.txt"):
        assert (tmp_path / "again" / f).read_bytes() == (dump / f).read_bytes(), f


# ------------------------------------------------------------------------------------------------ depth bounds (boxes chosen on the CPU)
BOUNDS_SEEDS = graphs.RANDOM_SEEDS[:60]


def _ratio(c1, c2):
    num, den = (c1, c2) if c1 > c2 else (c2, c1)
    return num / den if den != 0 else (float("inf") if num > 0 else float("nan"))


def _boxes(seed, g, edges_w):
    """nodes widened into (chr, pos, len, support, depth, lo, hi).  Even seeds: narrow boxes (1e-9 relative) on nodes none of whose edges
    has a depth ratio near 3 or 50 or a zero depth -- well clear of the thresholds; odd seeds: wide boxes on half the nodes -- they straddle
    the thresholds.  The depth is the midpoint of its box."""
    rng = random.Random(seed * 13 + 3)
    nodes = g["nodes"]
    risky = set()
    for e in edges_w:
        r = _ratio(nodes[e[0]][4], nodes[e[2]][4])
        if r != r or r == float("inf") or any(abs(r - t) <= 1e-6 * t for t in (3.0, 50.0)):
            risky.update((e[0], e[2]))
    out = []
    for i, n in enumerate(nodes):
        d = n[4]
        lo = hi = d
        if seed % 2 == 0:
            if i not in risky and d > 0 and rng.random() < 0.4:
                lo, hi = d * (1 - 1e-9), d * (1 + 1e-9)
        elif rng.random() < 0.5:
            lo, hi = (d * rng.uniform(0.1, 0.9), d * rng.uniform(1.1, 6.0)) if d > 0 else (0.0, rng.choice((0.25, 2.0)))
        mid = min(max(lo + (hi - lo) / 2, lo), hi)
        out.append(tuple(n[:4]) + (mid, lo, hi))
    return out


def _box_flag(nodes7, edges_w, bad, p):
    """the box rule as sq_graph.cpp / k_fe_edges state it (the project's own rule: the reference knows no bounds): does some coverage-ratio
    decision of FilterEdges depend on where inside their boxes the two depths lie"""
    passes = lambda e, r: not ((e[4] <= p["w"] + 2 and r > 3) or (e[4] > p["w"] + 2 and r > 50))
    for e in edges_w:
        na, nb = nodes7[e[0]], nodes7[e[2]]
        nearby = na[0] == nb[0] and abs(nb[1] - na[1] - na[2]) <= p["dp"]
        cond1 = ((e[0] not in bad and e[2] not in bad) or nearby) and e[5] > p["w"]
        if not (cond1 and (e[2] - e[0] > p["di"] or e[1] != 0 or e[3] != 1)):
            continue
        (alo, ahi), (blo, bhi) = na[5:7], nb[5:7]
        if alo == ahi and blo == bhi:
            continue
        if alo <= 0 and blo <= 0:
            return True
        sup = max(_ratio(ahi, blo), _ratio(alo, bhi))
        overlap = not (alo > bhi or blo > ahi)
        inf = 1.0 if overlap else min(_ratio(alo, bhi), _ratio(ahi, blo))
        if not (passes(e, sup) == passes(e, inf) == passes(e, _ratio(na[4], nb[4]))):
            return True
    return False


def _bounds_case(reference, seed):
    g, ref, tr = reference(seed)
    nodes7 = _boxes(seed, g, ref["weight"])
    return g, ref, nodes7, _box_flag(nodes7, ref["weight"], tr["bad_nodes"], g["params"])


def test_depth_boxes_give_both_flag_values(reference):
    """CPU: the boxes of the GPU test below are chosen so that at least 10 graphs have a decision that depends on the position inside a box
    and at least 10 have none, and boxes exist in all of them"""
    flags = []
    for seed in BOUNDS_SEEDS:
        _, _, nodes7, flag = _bounds_case(reference, seed)
        assert any(n[5] != n[6] for n in nodes7), seed
        flags.append(flag)
    assert flags.count(True) >= 10 and flags.count(False) >= 10, (flags.count(True), flags.count(False))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture()
def ctx(built):
    import squid_amd

    with squid_amd.Context() as c:
        yield c


@pytest.mark.gpu
def test_device_and_host_routes_equal_the_literals(ctx, reference):
    """every graph of the seed list through Context.debug_graph_stages by the kernels (route 1) and by the host functions (route 0), against
    the literals at stages 3, 4, 5 and 0: nodes with AvgDepth as equal doubles, edges with group weights, KeepEdge, labels, multiplied
    weights, the same assert where the graph ends empty.  The FurtherCompressNode kernel hands a graph back exactly where a node's lists hold
    more than FC_CAP = 256 discordant edges: fc_cap_255 / 256 / 257 report 0 / 0 / 1, no other graph of the list does.
    (scan_131073: the literals take about two seconds there and are still compared.)"""
    bad, fallbacks, t0 = [], {}, time.time()
    for seed in graphs.SEEDS:
        g, want, _ = reference(seed)
        for route in (1, 0):
            got = library_route(ctx, g, route)
            bad += _differences(want, got, f"{g['name']} route {route}")
            if route == 1:
                fallbacks[g["name"]] = got["fallback"]
            else:
                assert got["fallback"] == 0  # (the host route has nothing to hand back)
        at = want["compress"] if "compress" in want else (g["nodes"], g["edges"])
        if "final" in want:
            assert fallbacks[g["name"]] == (_longest_discordant_list(at[0], at[1], g["params"]) > 256), g["name"]
    print(f"{len(graphs.SEEDS)} graphs, both routes: {time.time() - t0:.2f} s")
    assert not bad, "\n".join(bad[:20])
    for k, want in ((255, 0), (256, 0), (257, 1)):
        assert fallbacks[f"fc_cap_{k}"] == want and fallbacks[f"fc_cap_{k}_front"] == want, (k, fallbacks[f"fc_cap_{k}"], fallbacks[f"fc_cap_{k}_front"])
    assert all(v == 0 for k, v in fallbacks.items() if not k.startswith("fc_cap_257")), {k: v for k, v in fallbacks.items() if v}


@pytest.mark.gpu
def test_depth_bounds_box_rule(ctx, reference):
    """FilterEdges with depth bounds: both routes keep the same edges and raise the same depth_ambiguous flag (the flag the CPU restatement
    of the rule predicts); where the flag is clear, no choice of depths inside the boxes changes a decision: the kept edges equal the
    literal FilterEdges at the midpoints, at every lower bound, at every upper bound and at eight random corners"""
    bad, seen = [], {0: 0, 1: 0}
    for seed in BOUNDS_SEEDS:
        g, ref, nodes7, flag = _bounds_case(reference, seed)
        p = g["params"]
        dev = library_route(ctx, g, 1, first=2, last=2, edges=ref["weight"], keep=ref["keep"], nodes=nodes7, bounds=True)
        host = library_route(ctx, g, 0, first=2, last=2, edges=ref["weight"], keep=ref["keep"], nodes=nodes7, bounds=True)
        if dev["filter"] != host["filter"] or dev["depth_ambiguous"] != host["depth_ambiguous"] or dev["depth_ambiguous"] != int(flag):
            bad.append(f"{g['name']}: device flag {dev['depth_ambiguous']}, host flag {host['depth_ambiguous']}, predicted {int(flag)}, kept {len(dev['filter'])} / {len(host['filter'])}")
            continue
        seen[dev["depth_ambiguous"]] += 1
        if dev["depth_ambiguous"]:
            continue
        rng = random.Random(seed * 17 + 1)
        picks = [[n[4] for n in nodes7], [n[5] for n in nodes7], [n[6] for n in nodes7]] + [[n[rng.choice((5, 6))] for n in nodes7] for _ in range(8)]
        for k, depths in enumerate(picks):
            exact = [n[:4] + (d,) for n, d in zip(nodes7, depths)]
            want = ll._filter_edges_literal(exact, ref["weight"], ref["keep"], min_w=p["w"], max_deg=p["a"], dist_pos=p["dp"], dist_idx=p["di"])
            if want != dev["filter"]:
                bad.append(f"{g['name']}: flag clear, but depth pick {k} changes the kept edges ({len(want)} / {len(dev['filter'])})")
    assert not bad, "\n".join(bad[:20])
    assert seen[0] >= 10 and seen[1] >= 10, seen


@pytest.mark.gpu
def test_graphs_that_enter_at_a_later_stage(ctx, reference):
    """at FilterEdges with a random KeepEdge column (60 random graphs), and at FurtherCompressNode with the hand-made graphs as they are (their
    raw edge lists; the big one is left to the test above): kernels == host functions == literals down to the final graph"""
    bad = []
    for seed in graphs.RANDOM_SEEDS[:60]:
        g, ref, _ = reference(seed)
        keep = _random_keep(seed, len(ref["weight"]))
        want = literal_route(g, first=2, edges=ref["weight"], keep=keep)
        for route in (1, 0):
            got = library_route(ctx, g, route, first=2, edges=ref["weight"], keep=keep)
            bad += _differences(want, got, f"{g['name']} from FilterEdges, route {route}")
            assert got["fallback"] == 0
    for name in graphs.HAND_NAMES:
        g = graphs.graph(name)
        if g["first"] == 4 or name in graphs.BIG or not g["edges"]:
            continue
        want = literal_route(g, first=4)
        for route in (1, 0):
            got = library_route(ctx, g, route, first=4)
            bad += _differences(want, got, f"{name} from FurtherCompressNode, route {route}")
            assert got["fallback"] == (route == 1 and _longest_discordant_list(g["nodes"], g["edges"], g["params"]) > 256), name
    assert not bad, "\n".join(bad[:20])
