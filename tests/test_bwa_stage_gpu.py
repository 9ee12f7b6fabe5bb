"""`squid --bwa` with node depth and breakpoint support on the device (sq_bwa_on_device: the decoded batch resident in HBM, a class byte per record,
the one-way depth cursor restated as a prefix maximum -- squid_amd/csrc/sq_bwa_stage.inc -- and the breakpoint kernels of the STAR path) against the
CPU oracle and against the host route of the same context: every stage snapshot, the orders, the breakpoint table and `_sv.txt` identical, with
no fallback to the host loops on the samples named here.  The CPU suite runs the same kernel source emulated (tests/test_bwa_stage_emu.py)."""
import subprocess

import numpy as np
import pytest

import bamwriter as bw
import oracle_util as ou
import shapes
import squid_amd
from test_bwa import _oracle_bwa
from test_bwa_stage_emu import (FUZZ, LONG_FALLBACK, LONG_LENGTHS, LONG_SEED, _literal_depth_loop, _read_cases, check_long_summary, emu, fuzz_summary,  # noqa: F401 -- (emu: the module
                                long_summary, read_long_cases)                                                                            # fixture that builds the harness)
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

HOST_ROWS = {"host_bwa_node_depth", "host_bwa_bp_support"}


def _launches(t, name):
    return t[name]["launches"] if name in t else None


def _route(t):
    """'device' | 'host' from a context's timing table after build_graph .. call_sv; the rows of the other route must be missing"""
    if _launches(t, "k_bwa_depth_apply"):
        assert not (HOST_ROWS & set(t)), sorted(t)
        assert _launches(t, "k_bp2") > 0 and _launches(t, "k_bwa_classify") == 2 and _launches(t, "bwa_device_fallback") == 0, sorted(t)
        return "device"
    assert HOST_ROWS <= set(t) and not any(k.startswith("k_bwa_") for k in t) and "bwa_device_fallback" not in t and "k_bp2" not in t, sorted(t)
    return "host"


def _counts(t):
    return _launches(t, "bwa_reads_records"), _launches(t, "bwa_bp_records")


def _both_routes(ctx, dump, sv_path):
    """device route against the oracle; then the host route and the device route again on the same context (the table stays resident)"""
    ctx.bwa_on_device()
    ctx.build_graph()
    sv = _compare(ctx, dump, sv_path)
    t = ctx.timing()
    assert _route(t) == "device"
    assert _launches(t, "bwa_upload") == 1 and _launches(t, "bwa_depth_held_blocks") is not None
    want_frags = sum(1 for line in (dump / "chimrecord.txt").read_text().splitlines() if not line.startswith("#"))
    assert ctx.counts()["n_chim_fragments"] == want_frags
    counts = _counts(t)
    assert counts[0] > 0 and counts[1] > 0
    nodes1 = ctx.graph(1)["nodes"]
    for on in (False, True):
        ctx.reset()
        ctx.bwa_on_device(on)
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == sv
        assert ctx.graph(1)["nodes"] == nodes1 and ctx.breakpoints() == ou.read_breakpoints(dump / "breakpoints.txt")
        t2 = ctx.timing()
        assert _route(t2) == ("device" if on else "host")
        assert _counts(t2) == counts, (on, _counts(t2), counts)
        assert "bwa_upload" not in t2  # (uploaded once per ingested batch)
    return sv, t


SAMPLES = [
    ("T2", (), (), {}),
    ("C2", (), (), {}),
    ("T2", ("--seed", "4242"), (), {}),
    ("T2", (), ("-w", "2", "-a", "20", "-mq", "30"), dict(min_edge_weight=2, max_allowed_degree=20, min_mapqual=30)),
]


@pytest.mark.parametrize("cfg,extra,flags,params", SAMPLES)
def test_device_route_equals_the_oracle_and_the_host_route(built, synth, tmp_path, monkeypatch, cfg, extra, flags, params):
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    pre = synth(cfg, "--bwa", *extra)
    sv_path, dump = _oracle_bwa(built, pre, tmp_path, *flags)
    kw = dict(min_mapqual=1)
    kw.update(params)
    with squid_amd.Context(star_mapq=False, **kw) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        sv, t = _both_routes(ctx, dump, sv_path)
        assert sv.count("\n") > 1
        assert _launches(t, "bwa_depth_held_blocks") > 0  # (spliced reads in front of later records: the cursor holds blocks, ledger W6)


def test_batch_that_came_through_the_device_reader(built, synth, tmp_path, monkeypatch):
    """SQUID_BWA_GPU=1: the batch was decoded on the device, copied back, and is uploaded again as the table (keeping the reader's copy is out of scope)"""
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    monkeypatch.setenv("SQUID_BWA_GPU", "1")
    pre = synth("T2", "--bwa")
    sv_path, dump = _oracle_bwa(built, pre, tmp_path)
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        assert ctx.counts()["chimeric_through_gpu_reader"] == 1
        _both_routes(ctx, dump, sv_path)


def test_depth_kernels_against_the_host_loop_on_the_fuzz_tables(emu, built, tmp_path):
    """the tables of the CPU fuzz (tools/bwa_stage_emu.cpp --fuzz, same seed, written out as numbers) through sq_debug_bwa_depth: route 1, the kernels,
    against route 0, the host loop -- every Support and sum; the fallback flag on exactly the cases whose chromosomes go down along Reads; the held
    blocks the emulated run counted"""
    out = subprocess.run([str(emu), "--fuzz", *FUZZ, "--write", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    want = fuzz_summary(out.stdout)
    cases = _read_cases(tmp_path / "cases.txt")
    assert len(cases) == 60
    held = fallbacks = blocks = 0
    with squid_amd.Context() as ctx:
        for k, (nodes, reads) in enumerate(cases):
            r1 = ctx.debug_bwa_depth(nodes, reads, route=1)
            r0 = ctx.debug_bwa_depth(nodes, reads, route=0)
            chroms = [c for c, _, _ in reads]
            decreasing = any(c < m for c, m in zip(chroms[1:], np.maximum.accumulate(chroms)[:-1])) if len(chroms) > 1 else False
            assert r1["fallback"] == int(decreasing), k
            assert (r0["support"], r0["sums"]) == _literal_depth_loop(nodes, reads), k
            if decreasing:
                fallbacks += 1
                continue
            assert (r1["support"], r1["sums"]) == (r0["support"], r0["sums"]), k
            held += r1["held"]; blocks += len(reads)
    assert (blocks, held, fallbacks) == (want["blocks"], want["held"], want["fallbacks"])
    assert 4 * held >= blocks and fallbacks > 0


def test_depth_kernels_on_long_tables(emu, built, tmp_path):
    """the tables of tools/bwa_stage_emu.cpp --fuzz-long (Reads lists of one and two rounds of depth_prefix, one block short and one block beyond;
    what must cross a round only the carry brings) through sq_debug_bwa_depth: route 1, the kernels, against route 0, the host loop, against the
    literal loop of the reference -- every Support and sum, the fallback flag on the one table whose chromosomes go down (at the first block of
    the second round), and per table the held blocks the emulated run counted"""
    out = subprocess.run([str(emu), "--fuzz-long", LONG_SEED, "--write", str(tmp_path / "long.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    want, per_case = long_summary(out.stdout)
    check_long_summary(want, per_case)
    cases = read_long_cases(tmp_path / "long.txt")
    assert [len(r) for _, r in cases] == LONG_LENGTHS
    with squid_amd.Context() as ctx:
        for k, (nodes, reads) in enumerate(cases):
            assert len(reads) <= 131073 and bool((np.diff(reads[:, 0]) >= 0).all()) == (k != LONG_FALLBACK), k
            r1 = ctx.debug_bwa_depth(nodes, reads, route=1)
            r0 = ctx.debug_bwa_depth(nodes, reads, route=0)
            assert r1["fallback"] == int(k == LONG_FALLBACK) == per_case[k][4], k
            assert (r0["support"], r0["sums"]) == _literal_depth_loop(nodes.tolist(), reads.tolist()), k
            if k == LONG_FALLBACK:
                continue
            assert (r1["support"], r1["sums"]) == (r0["support"], r0["sums"]), k
            assert (len(nodes), len(reads), r1["held"], sum(r1["support"])) == per_case[k][:4], k


# ---- a hand-made BAM: two contigs, a discordant cluster between them (node boundaries, an edge, breakpoints), a spliced read in front of five
# unspliced ones, and one record failing each factor of the two filters
A, B_ = 0, 1
PAIRED, PROPER, UNMAPPED, MATE_UNMAPPED, REV, MATE_REV, FIRST, SECOND, DUP, SUPPL = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x400, 0x800
NH1 = b"NHC\x01"


def handmade_records():
    recs = []  # (refid, pos, record bytes)

    def add(name, refid, pos, mapq, flag, cigar, mrefid, mpos, tags=NH1, lseq=None):
        recs.append((refid if refid >= 0 else 1 << 30, pos, bw.record(name, refid, pos, mapq, flag, cigar, mrefid, mpos, tags=tags, lseq=lseq)))

    def pair(name, left, right, mapq=60, right_flag=0, right_tags=NH1, right_mapq=None):
        """a concordant pair on contig A: first mate forward at `left`, second mate reverse at `right` (the right-hand record is the one
        ExactBPConcordantSupport counts, from the mate's position to its own end)"""
        add(name, A, left, mapq, PAIRED | PROPER | MATE_REV | FIRST, "60M", A, right)
        add(name, A, right, mapq if right_mapq is None else right_mapq, PAIRED | PROPER | REV | SECOND | right_flag, "60M", A, left, tags=right_tags)

    # seven discordant pairs A:3000.. <-> B:2000..: a dense discordant run on either contig (a seed node each) and an edge of weight 7
    for k in range(7):
        add(f"tra{k}", A, 3000 + k, 60, PAIRED | MATE_REV | FIRST, "60M", B_, 2000 + k)
        add(f"tra{k}", B_, 2000 + k, 60, PAIRED | REV | SECOND, "60M", A, 3000 + k)
    # concordant pairs over the breakpoints of contig A: left mates inside the node in front of 3000, right mates inside the seed node
    for k in range(6):
        pair(f"good{k}", 2900 + k, 3004 + k)
    # one record failing one factor of the filters at a time, each as the right-hand record of such a pair
    pair("f_xa", 2910, 3003, right_tags=NH1 + b"XAZchrB,+100,60M,0;\x00")
    pair("f_ih", 2911, 3002, right_tags=NH1 + b"IHC\x02")
    pair("f_mapq0", 2912, 3001, right_mapq=0)
    pair("f_lowmapq", 2913, 3005, right_mapq=5)     # (-mq 10: it feeds Reads and is not counted at the breakpoints)
    pair("f_dup", 2914, 3006, right_flag=DUP)
    add("f_unmapped", A, 2915, 60, PAIRED | MATE_REV | FIRST, "60M", A, 3007)
    add("f_unmapped", A, 3007, 0, PAIRED | UNMAPPED | SECOND, [], A, 2915, lseq=60)
    # mate to the right: the pair turned round -- the record at 3008 is the LEFT-hand one of its pair (mate at 3009), the one at 3009 counts
    add("f_mate_right", A, 3008, 60, PAIRED | PROPER | MATE_REV | FIRST, "60M", A, 3009)
    add("f_mate_right", A, 3009, 60, PAIRED | PROPER | REV | SECOND, "60M", A, 3008)
    # both mates at one position: the second mate is the one dropped
    add("f_same_pos", A, 2990, 60, PAIRED | PROPER | MATE_REV | FIRST, "60M", A, 2990)
    add("f_same_pos", A, 2990, 60, PAIRED | PROPER | REV | SECOND, "60M", A, 2990)
    # a read RawEdges rebuilds a fragment from: soft-clipped primary over the breakpoint at 3000 + hard-clipped supplementary record on B; its raw
    # QNAME is in the name set, so neither record is counted.  The last name group of the partial reads is never flushed (W3): `zz_last` stays out
    add("split1", A, 2970, 60, PAIRED | MATE_UNMAPPED | FIRST, "40M20S", -1, -1)
    add("split1", B_, 2030, 60, PAIRED | MATE_UNMAPPED | FIRST | SUPPL, "40H20M", -1, -1)
    add("zz_last", A, 2975, 60, PAIRED | MATE_UNMAPPED | FIRST, "40M20S", -1, -1)
    # contig B: a spliced read, then five unspliced reads inside its left exon: the cursor stands behind the intron when they come
    add("spliced", B_, 500, 60, PAIRED | MATE_UNMAPPED | FIRST, "30M5000N30M", -1, -1)
    for k in range(5):
        add(f"exon{k}", B_, 501 + k, 60, PAIRED | MATE_UNMAPPED | FIRST, "20M", -1, -1)
    # coverage in front of them, in the same node, that IS counted
    for k in range(3):
        add(f"before{k}", B_, 300 + k, 60, PAIRED | MATE_UNMAPPED | FIRST, "60M", -1, -1)
    recs.sort(key=lambda r: (r[0], r[1]))
    return [r[2] for r in recs]


def write_handmade(path):
    bw.write_bam(path, [("chrA", 20000), ("chrB", 10000)], handmade_records())


def test_hand_made_bam(built, tmp_path, monkeypatch):
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    pre = tmp_path / "hand"
    write_handmade(f"{pre}.bam")
    sv_path, dump = _oracle_bwa(built, pre, tmp_path, "-mq", "10")
    nodes = ou.read_nodes(dump / "nodes_build.txt")
    # the node of contig B that holds the left exon ends in front of the intron's far side: the first block of `spliced` is counted there,
    # `exon0..4`, which lie inside the same node, are not -- the cursor stands at the block behind the intron when they come
    left = [n for n in nodes if n[0] == B_ and n[1] <= 500 and 521 + 5 <= n[1] + n[2]]
    assert len(left) == 1 and left[0][1] + left[0][2] < 5530, nodes
    assert left[0][3] == 1, nodes
    assert sum(n[3] for n in nodes if n[0] == B_ and n[1] + n[2] <= 500) == 3, nodes  # (`before0..2`, in front of it, are)
    assert any(len(b) for b in ou.read_breakpoints(dump / "breakpoints.txt"))
    with squid_amd.Context(star_mapq=False, min_mapqual=10) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        sv, t = _both_routes(ctx, dump, sv_path)
        assert _launches(t, "bwa_depth_held_blocks") >= 5
        g1 = ctx.graph(1)["nodes"]
        assert [n[:5] for n in g1] == [n[:5] for n in nodes]


# the second case: seed 12 of the random --bwa shapes, MAPQ spread over 1..40 at -mq 30 -- two thirds of the records that feed Reads are in the
# table and are not counted at a breakpoint
PROBE_SEED = 12


@pytest.mark.parametrize("case", ["C2", "shape12"])
def test_cursor_probes(built, synth, monkeypatch, case):
    """sq_debug_bp_support on a --bwa context of the device route: a few hundred breakpoints, runs of adjacent positions inside covered exons
    included (the cursor moves one entry per record, so it lags behind them) -- the kernels over the table against the host loop over the batch"""
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    if case == "C2":
        pre, mq = synth("C2", "--bwa"), 1
    else:
        gen, _, params = shapes.draw_bwa(PROBE_SEED)
        assert case == f"shape{PROBE_SEED}" and shapes.mapq_range(gen) == (1, 40) and params["min_mapqual"] == 30
        pre, mq = synth("T2", *gen), 30
    with squid_amd.Context(star_mapq=False, min_mapqual=mq) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        ctx.bwa_on_device()
        ctx.build_graph()
        nodes = ctx.graph(1)["nodes"]
        covered = sorted((n for n in nodes if n[3] > 50 and n[2] > 200), key=lambda n: -n[3])[:12]
        assert len(covered) >= 6
        rng = np.random.default_rng(11)
        bps = set()
        for c, p, length, *_ in covered:
            at = p + int(rng.integers(10, length - 60))
            bps.update((c, at + k) for k in range(25))            # a run of adjacent positions
            bps.update((c, p + int(x)) for x in rng.integers(0, length, 6))
        for c, p, length, *_ in nodes[:: max(1, len(nodes) // 40)]:
            bps.add((c, p)); bps.add((c, p + length - 1))
        bps = sorted(bps)
        assert len(bps) > 300
        ch, po = [b[0] for b in bps], [b[1] for b in bps]
        dev = ctx.bp_support(ch, po)
        host = ctx.bp_support(ch, po, host_walk=True)
        assert dev.tolist() == host.tolist()
        assert int(host.max()) > 10 and int((host > 0).sum()) > 100
        assert _launches(ctx.timing(), "k_bp2") > 0


@pytest.mark.parametrize("env,call,want", [("0", True, "host"), ("1", False, "device"), (None, False, "host"), (None, True, "device")])
def test_environment_override_and_call(built, synth, monkeypatch, env, call, want):
    """SQUID_BWA_STAGES_GPU, read when the context is created: =0 forbids the route whatever the call says, =1 forces it without the call"""
    if env is None:
        monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    else:
        monkeypatch.setenv("SQUID_BWA_STAGES_GPU", env)
    pre = synth("T2", "--bwa")
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        ctx.bwa_on_device(call)
        ctx.build_graph()
        ctx.order()
        text = ctx.sv_text()
        assert _route(ctx.timing()) == want
    assert text == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()


def test_command_line_flag(built, synth, tmp_path, monkeypatch):
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    pre = synth("T2", "--bwa")
    for out, extra in (("p", ()), ("q", ("--device-bwa",))):
        subprocess.check_call([str(built / "squid"), "--bwa", "-b", f"{pre}.bam", "-o", str(tmp_path / out), "-G", "1", "-CO", "1", *extra], stdout=subprocess.DEVNULL)
    for suffix in ("_sv.txt", "_graph.txt", "_component_pri.txt"):
        assert (tmp_path / f"q{suffix}").read_bytes() == (tmp_path / f"p{suffix}").read_bytes(), suffix
    assert (tmp_path / "p_sv.txt").read_text().count("\n") > 1
    assert "--device-bwa" in subprocess.run([str(built / "squid"), "--help"], capture_output=True, text=True).stdout


def test_star_context_accepts_the_call(built, synth, monkeypatch):
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    pre = synth("T2")
    texts = []
    for on in (False, True):
        with squid_amd.Context() as ctx:
            ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
            ctx.bwa_on_device(on)
            ctx.build_graph()
            ctx.order()
            texts.append(ctx.sv_text())
            assert not any(k.startswith("k_bwa_") or k.startswith("bwa_") for k in ctx.timing())
    assert texts[0] == texts[1] and texts[0].count("\n") > 1


def test_clear_records_and_a_second_file(built, synth, tmp_path, monkeypatch):
    """sq_clear_records drops the table; the next batch gets one of its own; the STAR-mode calls keep refusing the context"""
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    first, second = synth("T2", "--bwa"), synth("T2", "--bwa", "--seed", "4242")
    sv_path, dump = _oracle_bwa(built, second, tmp_path)
    with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
        ctx.bwa_on_device()
        ctx.load_bwa(f"{first}.bam")
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2bwa_sv.txt").read_text()
        assert _route(ctx.timing()) == "device"
        with pytest.raises(squid_amd.SquidError):
            ctx.save_records(tmp_path / "cache.bin")
        with pytest.raises(squid_amd.SquidError):
            ctx._chk(ctx.lib.sq_ingest_concordant_file(ctx.h, f"{first}.bam".encode(), 4), "sq_ingest_concordant_file")
        ctx.clear_records()
        ctx.load_bwa(f"{second}.bam")
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        t = ctx.timing()
        assert _route(t) == "device" and _launches(t, "bwa_upload") == 1
