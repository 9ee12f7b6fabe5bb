"""`squid --bwa` with the record automaton of BuildNode_BWA on the device (sq_bwa_nodes_on_device: the stream cut at every gap in the coverage,
one wave per stretch from a fresh state on the host's guesses, the host's walk over the reports -- squid_amd/csrc/sq_bwa_nodes.inc) against the
CPU oracle, against the other routes of the same context, and -- the loop alone -- against the host automaton in one go
(sq_debug_bwa_seed_nodes) on files and on the tables of the CPU fuzz.  The CPU suite runs the same kernel source emulated
(tests/test_bwa_nodes_emu.py)."""
import subprocess

import numpy as np
import pytest

import shapes
import squid_amd
from test_bwa import _oracle_bwa
from test_bwa_nodes_emu import FUZZ, SHAPE_SEEDS, check_fuzz_summary, fuzz_summary, nodes_emu, write_handmade_nodes  # noqa: F401 -- (nodes_emu: the module fixture that builds the harness)
from test_bwa_stage_gpu import SAMPLES, _launches
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

NODE_KERNELS = ("k_bwa_node_class", "k_bwa_node_tile_max", "k_bwa_node_tile_prefix", "k_bwa_node_cut", "k_bwa_node_scan", "k_bwa_node_scatter", "k_bwa_node_dis", "k_bwa_node_carry", "k_bwa_node_run")
NODE_ROWS = ("bwa_node_stretches", "bwa_node_stretches_run_again", "bwa_node_longest_stretch", "bwa_nodes_device_fallback")
SWITCHES = ("SQUID_BWA_STAGES_GPU", "SQUID_BWA_EDGES_GPU", "SQUID_BWA_NODES_GPU", "SQUID_BWA_PIECE")


def _nodes_route(t):
    """True: the seed nodes of this graph came from the kernels; the rows of the other route must be missing"""
    if any(k.startswith("k_bwa_node_") for k in t):
        assert set(NODE_KERNELS) <= set(t) and set(NODE_ROWS) <= set(t), sorted(t)
        assert "host_bwa_seed_nodes" not in t and _launches(t, "bwa_nodes_device_fallback") == 0, sorted(t)
        assert _launches(t, "bwa_node_stretches") > 1 and _launches(t, "bwa_node_longest_stretch") > 0, sorted(t)
        assert _launches(t, "k_bwa_depth_apply") > 0 and _launches(t, "bwa_device_fallback") == 0 and "host_bwa_node_depth" not in t, sorted(t)  # (it implies the resident table)
        return True
    assert "host_bwa_seed_nodes" in t and not (set(NODE_ROWS) & set(t)), sorted(t)
    return False


def _state(ctx, sv):
    k = ctx.counts()
    return sv, ctx.graph(1), ctx.graph(2), k["n_raw_edges"], k["n_unique_edges"], k["n_chim_fragments"], k["read_len"], _launches(ctx.timing(), "bwa_reads_records")


ROUTES = {"host": (False, False, False), "depth": (True, False, False), "edges": (False, True, False), "nodes": (False, False, True), "nodes+edges": (False, True, True)}


def _all_routes(ctx, dump, sv_path):
    """the nodes route against the oracle stage by stage; then host, depth-only, edges, nodes and nodes + edges on the same context"""
    ctx.bwa_nodes_on_device()
    ctx.build_graph()
    sv = _compare(ctx, dump, sv_path)
    t = ctx.timing()
    assert _nodes_route(t)
    assert _launches(t, "bwa_upload") == 1
    want = _state(ctx, sv)
    assert want[3] > 0 and want[6] > 0 and want[7] > 0
    for route, (depth, edges, nodes) in ROUTES.items():
        ctx.reset()
        ctx.bwa_on_device(depth); ctx.bwa_edges_on_device(edges); ctx.bwa_nodes_on_device(nodes)
        ctx.build_graph()
        ctx.order()
        assert _state(ctx, ctx.sv_text()) == want, route
        t2 = ctx.timing()
        assert _nodes_route(t2) == nodes, route
        assert any(k.startswith("k_bwa_edge_") for k in t2) == edges, route
        assert "bwa_upload" not in t2  # (uploaded once per ingested batch)
    return sv, t


def _no_switch(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("cfg,extra,flags,params", SAMPLES)
def test_nodes_route_equals_the_oracle_and_the_other_routes(built, synth, tmp_path, monkeypatch, cfg, extra, flags, params):
    _no_switch(monkeypatch)
    pre = synth(cfg, "--bwa", *extra)
    sv_path, dump = _oracle_bwa(built, pre, tmp_path, *flags)
    kw = dict(min_mapqual=1)
    kw.update(params)
    with squid_amd.Context(star_mapq=False, **kw) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        sv, _ = _all_routes(ctx, dump, sv_path)
        assert sv.count("\n") > 1


FIELDS = ("seeds", "read_len", "n_reads_records", "flush_nodes", "marks_closed")


def _same_loop(r1, r0):
    assert r1["fallback"] == 0 and r0["stretches"] == 1
    for f in FIELDS:
        assert r1[f] == r0[f], f


def test_debug_routes_on_t2(built, synth, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2", "--bwa")
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        r1, r0 = ctx.debug_bwa_seed_nodes(1), ctx.debug_bwa_seed_nodes(0)  # (the debug call uploads the batch by itself)
        _same_loop(r1, r0)
        assert len(r0["seeds"]) > 0 and r1["stretches"] > 1 and r0["flush_nodes"] >= 1
        assert set(NODE_KERNELS) <= set(ctx.timing())
        # the next graph of the context on the nodes route finds the table the debug call left
        ctx.bwa_nodes_on_device()
        ctx.build_graph()
        ctx.order()
        t = ctx.timing()
        assert _nodes_route(t) and "bwa_upload" not in t
        assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()


def test_debug_routes_on_the_hand_made_bam(built, tmp_path, monkeypatch):
    """a stretch whose guess is wrong (run again on the host) and marks the zero-coverage rule closes: tests/test_bwa_nodes_emu.py says why"""
    _no_switch(monkeypatch)
    pre = tmp_path / "hand"
    write_handmade_nodes(f"{pre}.bam")
    sv_path, dump = _oracle_bwa(built, pre, tmp_path, "-mq", "10")
    with squid_amd.Context(star_mapq=False, min_mapqual=10) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        r1, r0 = ctx.debug_bwa_seed_nodes(1), ctx.debug_bwa_seed_nodes(0)
        _same_loop(r1, r0)
        assert r1["again"] >= 1 and r0["marks_closed"] >= 1 and r0["flush_nodes"] >= 2 and r1["stretches"] >= 4
        ctx.bwa_nodes_on_device()
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        t = ctx.timing()
        assert _nodes_route(t) and _launches(t, "bwa_node_stretches_run_again") >= 1


# the four shapes of the CPU file; the last two through the device reader
@pytest.mark.parametrize("seed,through_gpu", list(zip(SHAPE_SEEDS, ("0", "0", "1", "1"))))
def test_debug_routes_on_random_shapes(built, synth, monkeypatch, seed, through_gpu):
    _no_switch(monkeypatch)
    monkeypatch.setenv("SQUID_BWA_GPU", through_gpu)
    assert seed in shapes.BWA_SEEDS
    gen, _, params = shapes.draw_bwa(seed)
    pre = synth("T2", *gen)
    with squid_amd.Context(**params) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        assert ctx.counts()["chimeric_through_gpu_reader"] == int(through_gpu)
        r1, r0 = ctx.debug_bwa_seed_nodes(1), ctx.debug_bwa_seed_nodes(0)
        _same_loop(r1, r0)
        assert len(r0["seeds"]) > 0 and r1["stretches"] > 1


def read_fuzz_cases(path):
    """the cases `bwa_nodes_emu --fuzz --write` keeps: (records, blk_off, blocks, fallback)"""
    rows = [line.split() for line in open(path)]
    cases, at = [], 0
    while at < len(rows):
        assert rows[at][0] == "case"
        nr, nb, fallback = (int(x) for x in rows[at][1:])
        at += 1
        recs = np.array(rows[at:at + nr], dtype=np.int64).reshape(-1, 9); at += nr
        blocks = np.array(rows[at:at + nb], dtype=np.int32).reshape(-1, 4); at += nb
        blk_off = np.concatenate([[0], np.cumsum(recs[:, 8])]).astype(np.uint32)
        assert int(blk_off[-1]) == nb
        cases.append((recs[:, :8].astype(np.int32), blk_off, blocks, fallback))
    return cases


def test_kernels_against_the_host_automaton_on_the_fuzz_tables(nodes_emu, built, tmp_path):  # noqa: F811
    """the tables of the CPU fuzz (tools/bwa_nodes_emu.cpp --fuzz, same seed, written out as numbers) through sq_debug_bwa_seed_nodes_tables --
    the tables become a batch of the library's own layout and go through the one upload path -- route 1, the kernels, against route 0, the host
    automaton in one go: every field on every table that was not planted; the fallback flag on exactly the planted ones; totals equal to the
    harness's summary.  The harness starts every fifth case from a read length of 60 (as if a chimeric file had set it); so does this test"""
    out = subprocess.run([str(nodes_emu), "--fuzz", *FUZZ, "--write", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    want = fuzz_summary(out.stdout)
    check_fuzz_summary(want)
    cases = read_fuzz_cases(tmp_path / "cases.txt")
    assert len(cases) == 60
    tot = dict.fromkeys(("records", "seeds", "reads", "stretches", "again", "single", "flush_nodes", "marks_closed", "fallbacks"), 0)
    longest = 0
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        for k, (recs, blk_off, blocks, planted) in enumerate(cases):
            rl = 60 if k % 5 == 4 else 0
            r1 = ctx.debug_bwa_seed_nodes_tables(recs, blk_off, blocks, route=1, read_len=rl)
            assert r1["fallback"] == planted, k
            if planted:
                tot["fallbacks"] += 1
                continue
            r0 = ctx.debug_bwa_seed_nodes_tables(recs, blk_off, blocks, route=0, read_len=rl)
            _same_loop(r1, r0)
            tot["records"] += len(recs); tot["seeds"] += len(r1["seeds"]); tot["reads"] += r1["n_reads_records"]; tot["stretches"] += r1["stretches"]; tot["again"] += r1["again"]
            tot["single"] += r1["single"]; tot["flush_nodes"] += r1["flush_nodes"]; tot["marks_closed"] += r1["marks_closed"]
            longest = max(longest, r1["longest"])
    assert tot == {k: want[k] for k in tot}, (tot, want)
    assert longest == want["longest"]


@pytest.mark.parametrize("env,call,want", [("0", True, False), ("1", False, True), (None, False, False), (None, True, True)])
def test_environment_override_and_call(built, synth, monkeypatch, env, call, want):
    """SQUID_BWA_NODES_GPU, read when the context is created: =0 forbids the route whatever the call says, =1 forces it without the call (and
    with it the resident table)"""
    _no_switch(monkeypatch)
    if env is not None:
        monkeypatch.setenv("SQUID_BWA_NODES_GPU", env)
    pre = synth("T2", "--bwa")
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        ctx.bwa_nodes_on_device(call)
        ctx.build_graph()
        ctx.order()
        text = ctx.sv_text()
        assert _nodes_route(ctx.timing()) == want
    assert text == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()


def test_command_line_flag(built, synth, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2", "--bwa")
    for out, extra in (("p", ()), ("q", ("--device-bwa-nodes",))):
        subprocess.check_call([str(built / "squid"), "--bwa", "-b", f"{pre}.bam", "-o", str(tmp_path / out), "-G", "1", "-CO", "1", *extra], stdout=subprocess.DEVNULL)
    for suffix in ("_sv.txt", "_graph.txt", "_component_pri.txt"):
        assert (tmp_path / f"q{suffix}").read_bytes() == (tmp_path / f"p{suffix}").read_bytes(), suffix
    assert (tmp_path / "p_sv.txt").read_text().count("\n") > 1
    assert "--device-bwa-nodes" in subprocess.run([str(built / "squid"), "--help"], capture_output=True, text=True).stdout


def test_star_context_accepts_the_call(built, synth, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2")
    texts = []
    for on in (False, True):
        with squid_amd.Context() as ctx:
            ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
            ctx.bwa_nodes_on_device(on)
            ctx.build_graph()
            ctx.order()
            texts.append(ctx.sv_text())
            assert not any(k.startswith("k_bwa_") or k.startswith("bwa_") or k.startswith("host_bwa_") for k in ctx.timing())
    assert texts[0] == texts[1] and texts[0].count("\n") > 1


def test_clear_records_and_a_second_file(built, synth, tmp_path, monkeypatch):
    """sq_clear_records drops the table; the next batch gets a table and stretches of its own"""
    _no_switch(monkeypatch)
    first, second = synth("T2", "--bwa"), synth("T2", "--bwa", "--seed", "4242")
    sv_path, dump = _oracle_bwa(built, second, tmp_path)
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.bwa_nodes_on_device()
        ctx.load_bwa(f"{first}.bam")
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()
        assert _nodes_route(ctx.timing())
        ctx.clear_records()
        ctx.load_bwa(f"{second}.bam")
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        t = ctx.timing()
        assert _nodes_route(t) and _launches(t, "bwa_upload") == 1
