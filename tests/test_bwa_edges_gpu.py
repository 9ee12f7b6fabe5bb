"""`squid --bwa` with the record loop of RawEdges on the device (sq_bwa_edges_on_device: a fragment table made from the resident records, the
position chain of the chimeric device stages, one lane per record for the edges, the loop's three lists compacted in record order --
squid_amd/csrc/sq_bwa_edges.inc) against the CPU oracle, against the host route and the depth-only device route of the same context, and --
the loop alone -- against the host loop in one go (sq_debug_bwa_raw_edges) on files and on the tables of the CPU fuzz.  The CPU suite runs
the same kernel source emulated (tests/test_bwa_edges_emu.py)."""
import subprocess

import numpy as np
import pytest

import shapes
import squid_amd
from test_bwa import _oracle_bwa
from test_bwa_edges_emu import FUZZ, edges_emu, fuzz_summary, write_handmade_edges  # noqa: F401 -- (edges_emu: the module fixture that builds the harness)
from test_bwa_stage_gpu import SAMPLES, _launches
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

EDGE_KERNELS = ("k_bwa_frag_count", "k_bwa_frag_scan", "k_bwa_frag_fill", "k_bwa_edge_classify", "k_bwa_edge_scan", "k_bwa_edge_soft", "k_bwa_edge_fragment", "k_bwa_edge_compact",
                "k_bwa_edge_lists")
SWITCHES = ("SQUID_BWA_STAGES_GPU", "SQUID_BWA_EDGES_GPU", "SQUID_BWA_PIECE")


def _edge_rows(t):
    return sorted(k for k in t if k.startswith("k_bwa_edge_") or k.startswith("k_bwa_frag_"))


def _route(t):
    """'edges' | 'depth' | 'host' from a context's timing table after build_graph .. call_sv; the rows of the other routes must be missing"""
    if _edge_rows(t):
        assert set(EDGE_KERNELS) <= set(t), sorted(t)
        assert _launches(t, "bwa_edges_device_fallback") == 0 and "host_bwa_raw_edges" not in t and "host_bwa_raw_edges_tail" in t, sorted(t)
        assert _launches(t, "k_bwa_classify") == 2 and _launches(t, "bwa_device_fallback") == 0 and _launches(t, "k_bwa_depth_apply") > 0, sorted(t)
        assert _launches(t, "bwa_edge_soft_fragments") is not None and _launches(t, "bwa_edge_lists") > 0, sorted(t)
        return "edges"
    assert "host_bwa_raw_edges" in t and "bwa_edges_device_fallback" not in t and "host_bwa_raw_edges_tail" not in t and "bwa_edge_lists" not in t, sorted(t)
    return "depth" if _launches(t, "k_bwa_depth_apply") else "host"


def _state(ctx, sv):
    k = ctx.counts()
    return sv, ctx.graph(1), ctx.graph(2), k["n_raw_edges"], k["n_unique_edges"], k["n_chim_fragments"]


def _all_routes(ctx, dump, sv_path):
    """the edges route against the oracle; then the host route, the depth-only device route and the edges route again on the same context"""
    ctx.bwa_edges_on_device()
    ctx.build_graph()
    sv = _compare(ctx, dump, sv_path)
    t = ctx.timing()
    assert _route(t) == "edges"
    assert _launches(t, "bwa_upload") == 1
    want_frags = sum(1 for line in (dump / "chimrecord.txt").read_text().splitlines() if not line.startswith("#"))
    assert ctx.counts()["n_chim_fragments"] == want_frags
    want = _state(ctx, sv)
    assert want[3] > 0 and want[4] > 0
    for route in ("host", "depth", "edges"):
        ctx.reset()
        ctx.bwa_edges_on_device(route == "edges")
        ctx.bwa_on_device(route == "depth")
        ctx.build_graph()
        ctx.order()
        assert _state(ctx, ctx.sv_text()) == want, route
        t2 = ctx.timing()
        assert _route(t2) == route
        assert "bwa_upload" not in t2  # (uploaded once per ingested batch)
    return sv, t


def _no_switch(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("cfg,extra,flags,params", SAMPLES)
def test_edges_route_equals_the_oracle_and_the_other_routes(built, synth, tmp_path, monkeypatch, cfg, extra, flags, params):
    _no_switch(monkeypatch)
    pre = synth(cfg, "--bwa", *extra)
    sv_path, dump = _oracle_bwa(built, pre, tmp_path, *flags)
    kw = dict(min_mapqual=1)
    kw.update(params)
    with squid_amd.Context(star_mapq=False, **kw) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        sv, t = _all_routes(ctx, dump, sv_path)
        assert sv.count("\n") > 1
        assert _launches(t, "bwa_edge_soft_fragments") > 0  # (first blocks at node edges: the chain had something to resolve in record order)


def test_edges_route_on_the_hand_made_bam(built, tmp_path, monkeypatch):
    """multi-aligned second mates (one whose -1 edge is added, one whose first mate added nothing), a reverse-strand record of three blocks, first
    blocks at read offset 15 and 16: tests/test_bwa_edges_emu.py checks on the CPU that the host loop alone yields them"""
    _no_switch(monkeypatch)
    pre = tmp_path / "hand"
    write_handmade_edges(f"{pre}.bam")
    sv_path, dump = _oracle_bwa(built, pre, tmp_path, "-mq", "10")
    with squid_amd.Context(star_mapq=False, min_mapqual=10) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        sv, t = _all_routes(ctx, dump, sv_path)
        assert sv.count("\n") > 1
        r1, r0 = ctx.debug_bwa_raw_edges(1), ctx.debug_bwa_raw_edges(0)
        _same_loop(r1, r0)
        assert len(r0["second"]) == 2 and len(r0["first_dis"]) >= 8 and len(r0["part"]) >= 3


FIELDS = ("keys", "weights", "part", "first_dis", "second", "second_keys", "final_pos", "n_emitted")


def _same_loop(r1, r0):
    assert r1["fallback"] == 0
    for f in FIELDS:
        assert r1[f] == r0[f], f
    assert sum(r0["weights"]) == r0["n_emitted"] and r0["keys"] == sorted(set(r0["keys"]))
    assert r0["part"] == sorted(r0["part"]) and r0["first_dis"] == sorted(r0["first_dis"]) and r0["second"] == sorted(r0["second"])


def test_debug_routes_on_t2(built, synth, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2", "--bwa")
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        ctx.build_graph()  # (host route: the debug call uploads the batch by itself)
        r1, r0 = ctx.debug_bwa_raw_edges(1), ctx.debug_bwa_raw_edges(0)
        _same_loop(r1, r0)
        assert r1["n_soft"] > 0 and len(r0["part"]) > 0 and len(r0["first_dis"]) > 0 and r0["n_emitted"] > len(r0["keys"]) > 0
        assert set(EDGE_KERNELS) <= set(ctx.timing())
        # the next graph of the context on the edges route finds the table the debug call left
        ctx.reset()
        ctx.bwa_edges_on_device()
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()


# four of the random --bwa shapes: 250-base reads, the longest Reads list, odd pairs at 13 %, 50-base reads; the last two through the device reader
SHAPE_SEEDS = ((2, "0"), (6, "0"), (12, "1"), (14, "1"))


@pytest.mark.parametrize("seed,through_gpu", SHAPE_SEEDS)
def test_debug_routes_on_random_shapes(built, synth, monkeypatch, seed, through_gpu):
    _no_switch(monkeypatch)
    monkeypatch.setenv("SQUID_BWA_GPU", through_gpu)
    assert seed in shapes.BWA_SEEDS
    gen, _, params = shapes.draw_bwa(seed)
    pre = synth("T2", *gen)
    with squid_amd.Context(**params) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        assert ctx.counts()["chimeric_through_gpu_reader"] == int(through_gpu)
        ctx.bwa_edges_on_device()
        ctx.build_graph()
        assert _launches(ctx.timing(), "bwa_edges_device_fallback") == 0
        r1, r0 = ctx.debug_bwa_raw_edges(1), ctx.debug_bwa_raw_edges(0)
        _same_loop(r1, r0)
        assert len(r0["part"]) > 0 and r0["n_emitted"] > 0


def read_fuzz_cases(path):
    """the cases `bwa_edges_emu --fuzz --write` keeps: (nodes, records, blk_off, blocks, asserts, soft)"""
    rows = [line.split() for line in open(path)]
    cases, at = [], 0
    while at < len(rows):
        assert rows[at][0] == "case"
        nn, nr, nb, asserts, soft = (int(x) for x in rows[at][1:])
        at += 1
        nodes = np.array(rows[at:at + nn], dtype=np.int32).reshape(-1, 3); at += nn
        recs = np.array(rows[at:at + nr], dtype=np.int64).reshape(-1, 9); at += nr
        blocks = np.array(rows[at:at + nb], dtype=np.int32).reshape(-1, 4); at += nb
        blk_off = np.concatenate([[0], np.cumsum(recs[:, 8])]).astype(np.uint32)
        assert int(blk_off[-1]) == nb
        cases.append((nodes, recs[:, :8].astype(np.int32), blk_off, blocks, asserts, soft))
    return cases


def test_kernels_against_the_host_loop_on_the_fuzz_tables(edges_emu, built, tmp_path):  # noqa: F811
    """the tables of the CPU fuzz (tools/bwa_edges_emu.cpp --fuzz, same seed, written out as numbers) through sq_debug_bwa_raw_edges_tables -- the
    table-taking form of the debug call: the tables become a batch of the library's own layout and go through the one upload path, so there is no
    second ingest -- route 1, the kernels, against route 0, the host loop: every field on every case on which the loop does not assert; the
    fallback flag on exactly the cases on which it does (route 0 fails there with SQ_E_ASSERT; the kernels raise their flag in front of any access
    outside the node table); the soft fragments the emulated run printed"""
    out = subprocess.run([str(edges_emu), "--fuzz", *FUZZ, "--write", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    want = fuzz_summary(out.stdout)
    cases = read_fuzz_cases(tmp_path / "cases.txt")
    assert len(cases) == 60
    soft = asserts = records = emitted = 0
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        for k, (nodes, recs, blk_off, blocks, asserting, case_soft) in enumerate(cases):
            if len(nodes) == 0:
                assert len(recs) == 0
            r1 = ctx.debug_bwa_raw_edges_tables(nodes, recs, blk_off, blocks, route=1)
            if asserting:
                assert r1["fallback"] == 1, k
                with pytest.raises(squid_amd.SquidError):
                    ctx.debug_bwa_raw_edges_tables(nodes, recs, blk_off, blocks, route=0)
                asserts += 1
                continue
            r0 = ctx.debug_bwa_raw_edges_tables(nodes, recs, blk_off, blocks, route=0)
            if len(recs) == 0:
                assert r1["fallback"] == 0 and r0["keys"] == [] and r1["keys"] == [] and r1["final_pos"] == r0["final_pos"] == 0, k
                continue
            _same_loop(r1, r0)
            assert r1["n_soft"] == case_soft, k
            soft += r1["n_soft"]; records += len(recs); emitted += r0["n_emitted"]
    assert (records, soft, asserts, emitted) == (want["records"], want["soft"], want["asserts"], want["emitted"])
    assert 1 <= asserts <= 15 and soft > 1000


@pytest.mark.parametrize("env,call,want", [("0", True, "host"), ("1", False, "edges"), (None, False, "host"), (None, True, "edges")])
def test_environment_override_and_call(built, synth, monkeypatch, env, call, want):
    """SQUID_BWA_EDGES_GPU, read when the context is created: =0 forbids the route whatever the call says, =1 forces it without the call (and
    with it the resident table)"""
    _no_switch(monkeypatch)
    if env is not None:
        monkeypatch.setenv("SQUID_BWA_EDGES_GPU", env)
    pre = synth("T2", "--bwa")
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        ctx.bwa_edges_on_device(call)
        ctx.build_graph()
        ctx.order()
        text = ctx.sv_text()
        assert _route(ctx.timing()) == want
    assert text == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()


def test_command_line_flag(built, synth, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2", "--bwa")
    for out, extra in (("p", ()), ("q", ("--device-bwa-edges",))):
        subprocess.check_call([str(built / "squid"), "--bwa", "-b", f"{pre}.bam", "-o", str(tmp_path / out), "-G", "1", "-CO", "1", *extra], stdout=subprocess.DEVNULL)
    for suffix in ("_sv.txt", "_graph.txt", "_component_pri.txt"):
        assert (tmp_path / f"q{suffix}").read_bytes() == (tmp_path / f"p{suffix}").read_bytes(), suffix
    assert (tmp_path / "p_sv.txt").read_text().count("\n") > 1
    assert "--device-bwa-edges" in subprocess.run([str(built / "squid"), "--help"], capture_output=True, text=True).stdout


def test_star_context_accepts_the_call(built, synth, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2")
    texts = []
    for on in (False, True):
        with squid_amd.Context() as ctx:
            ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
            ctx.bwa_edges_on_device(on)
            ctx.build_graph()
            ctx.order()
            texts.append(ctx.sv_text())
            assert not any(k.startswith("k_bwa_") or k.startswith("bwa_") or k.startswith("host_bwa_") for k in ctx.timing())
    assert texts[0] == texts[1] and texts[0].count("\n") > 1


def test_clear_records_and_a_second_file(built, synth, tmp_path, monkeypatch):
    """sq_clear_records drops the table; the next batch gets a table and a fragment table of its own"""
    _no_switch(monkeypatch)
    first, second = synth("T2", "--bwa"), synth("T2", "--bwa", "--seed", "4242")
    sv_path, dump = _oracle_bwa(built, second, tmp_path)
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.bwa_edges_on_device()
        ctx.load_bwa(f"{first}.bam")
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()
        assert _route(ctx.timing()) == "edges"
        ctx.clear_records()
        ctx.load_bwa(f"{second}.bam")
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        t = ctx.timing()
        assert _route(t) == "edges" and _launches(t, "bwa_upload") == 1
