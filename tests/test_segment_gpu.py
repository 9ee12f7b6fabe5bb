"""BuildNode_STAR's segmentation automaton on the device (sq_segment_on_device: one wave per active stretch of the concordant stream from a fresh
state on the guess that a node exists in front and is too far away to matter, the host's walk over the reports -- squid_amd/csrc/
sq_segment_stage.inc) against the CPU oracle, against the host route of the same context, against the literal reading of the reference, and
-- the automaton alone -- against the host automaton in one go (sq_debug_segment_seeds) on files and on the tables of the CPU fuzz.  The CPU
suite runs the same kernel source emulated (tests/test_segment_emu.py)."""
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import shapes
import squid_amd
from test_chim_stage_gpu import _route as _chim_route
from test_gpu_parity import LOW_SUPPORT_SAMPLES, _compare
from test_segment_emu import FUZZ, check_fuzz_summary, fuzz_summary, segment_emu  # noqa: F401 -- (segment_emu: the module fixture that builds the harness)

pytestmark = pytest.mark.gpu

SEG_ROWS = ("segment_stretches", "segment_stretches_run_again", "segment_longest_stretch", "segment_device_fallback")
SWITCHES = ("SQUID_SEGMENT_GPU", "SQUID_CHIM_STAGES_GPU", "SQUID_REPLAY_CHECK")


def _launches(t, name):
    return t.get(name, {}).get("launches", 0)


def _seg_route(t):
    """True: the seed nodes of this graph came from the kernel; the rows of the other route must be missing"""
    if any(k.startswith("k_seg_") for k in t):
        assert "k_seg_run" in t and "host_segment_walk" in t and set(SEG_ROWS) <= set(t), sorted(t)
        assert "host_segment_replay" not in t and _launches(t, "segment_device_fallback") == 0, sorted(t)
        assert _launches(t, "segment_stretches") > 1 and _launches(t, "segment_longest_stretch") > 0, sorted(t)
        assert _launches(t, "segment_stretches_run_again") < _launches(t, "segment_stretches"), sorted(t)
        return True
    assert "host_segment_replay" in t and not (set(SEG_ROWS) & set(t)) and "host_segment_walk" not in t, sorted(t)
    return False


def _no_switch(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _state(ctx, sv):
    k = ctx.counts()
    return sv, ctx.graph(1), ctx.graph(2), k["n_raw_edges"], k["n_unique_edges"], k["n_break"], k["replay_candidates_checked"], k["replay_count_mismatches"]


SAMPLES = [("T2", (), (), {}), ("C2", (), (), {}), ("C2", ("--support", "2,6"), (), {}), LOW_SUPPORT_SAMPLES[0]]


def test_the_dense_sample_is_the_one_the_chimeric_stage_tests_use():
    from test_chim_stage_gpu import SAMPLES as CHIM_SAMPLES

    assert LOW_SUPPORT_SAMPLES[0] == ("C5", ("--records", "300000", "--tsv", "1500", "--support", "2,8"), (), {}) and LOW_SUPPORT_SAMPLES[0] in CHIM_SAMPLES


@pytest.mark.parametrize("cfg,gen,flags,params", SAMPLES)
def test_device_route_equals_the_oracle_and_the_host_route(built, synth, tmp_path, monkeypatch, cfg, gen, flags, params):
    _no_switch(monkeypatch)
    monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")
    pre = synth(cfg, *gen)
    sv_path, dump = ou.run_oracle(built, pre, tmp_path, *flags)
    with squid_amd.Context(**params) as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.segment_on_device()
        ctx.build_graph()
        sv = _compare(ctx, dump, sv_path)
        assert _seg_route(ctx.timing())
        want = _state(ctx, sv)
        assert want[6] == 0 and want[7] == 0  # (SQUID_REPLAY_CHECK is a facility of the host route)
        for route, (seg, chim) in {"host": (False, False), "device": (True, False), "device + chimeric": (True, True)}.items():
            ctx.reset()
            ctx.segment_on_device(seg); ctx.chimeric_on_device(chim)
            ctx.build_graph()
            ctx.order()
            assert _state(ctx, ctx.sv_text()) == want, route
            t = ctx.timing()
            assert _seg_route(t) == seg, route
            assert _chim_route(t) == (("device", 0) if chim else ("host", 0)), route


def _same(r1, r0):
    assert r1["fallback"] == 0 and r0["fallback"] == 0
    assert r1["seeds"] == r0["seeds"] and r1["extended"] == r0["extended"]
    assert r0["again"] == 0 and r0["stretches"] == r1["stretches"]


@pytest.mark.parametrize("cfg", ["T2", "C2"])
def test_debug_routes_on_the_samples(built, synth, monkeypatch, cfg):
    _no_switch(monkeypatch)
    pre = synth(cfg)
    with squid_amd.Context() as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        r1, r0 = ctx.debug_segment_seeds(1), ctx.debug_segment_seeds(0)
        _same(r1, r0)
        assert len(r0["seeds"]) >= 3 and r1["stretches"] > 1 and r1["again"] < r1["stretches"] and r1["kept_with_nodes"] > 0
        assert "k_seg_run" in ctx.timing()
        # the next graph of the context is not disturbed by the debug calls
        ctx.build_graph()
        ctx.order()
        if cfg == "T2":
            assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2_sv.txt").read_text()
        assert not _seg_route(ctx.timing())


# four of the 24 random STAR shapes: the 50-base reads, the 250-base reads, the most clipped, the most contigs; the last two through the device reader
SHAPE_SEEDS = [14, 2, 19, 4]


def test_the_four_shape_seeds_are_what_they_are_named_for():
    drawn = {s: list(shapes.draw(s)[0]) for s in shapes.SEEDS}
    assert shapes.read_len(drawn[14]) == 50 == min(shapes.read_len(g) for g in drawn.values())
    assert shapes.read_len(drawn[2]) == 250 == max(shapes.read_len(g) for g in drawn.values())
    clip = {s: float(g[g.index("--clip-frac") + 1]) for s, g in drawn.items() if "--clip-frac" in g}
    assert max(clip, key=clip.get) == 19
    contigs = {s: len(g[g.index("--contigs") + 1].split(",")) for s, g in drawn.items() if "--contigs" in g}
    assert contigs[4] == max(contigs.values())


@pytest.mark.parametrize("seed,gpu_inflate", list(zip(SHAPE_SEEDS, ("0", "0", "1", "1"))))
def test_debug_routes_on_random_shapes(built, synth, monkeypatch, seed, gpu_inflate):
    _no_switch(monkeypatch)
    monkeypatch.setenv("SQUID_GPU_INFLATE", gpu_inflate)
    gen, _, params = shapes.draw(seed)
    pre = synth("T2", *gen)
    with squid_amd.Context(**params) as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        r1, r0 = ctx.debug_segment_seeds(1), ctx.debug_segment_seeds(0)
        _same(r1, r0)
        assert len(r0["seeds"]) > 0 and r1["stretches"] > 1


def read_fuzz_cases(path):
    """the cases `segment_emu --fuzz --write` keeps: (read_len, recs6, disc4, part2, rest_off, rest_pos, rest_len, trigger, zero3, flagged stretches, seeds)"""
    lines = open(path).read().split("\n")
    cases, at = [], 0
    while at < len(lines) and lines[at]:
        head = lines[at].split()
        assert head[0] == "case"
        rl, nr, nd, npart, ncl, nrest, nz, flagged, nseeds = (int(x) for x in head[1:])
        at += 1
        recs = np.array([ln.split() for ln in lines[at:at + nr]], dtype=np.int32).reshape(-1, 6); at += nr
        arrays = [np.array(lines[at + i].split(), dtype=np.int32) for i in range(7)]; at += 7
        disc4, part2, rest_off, rest_pos, rest_len, trigger, zero3 = arrays
        assert (len(disc4), len(part2), len(rest_off), len(rest_pos), len(trigger), len(zero3)) == (4 * nd, 2 * npart, ncl + 1, nrest, ncl, 3 * nz)
        cases.append((rl, recs, disc4, part2, rest_off, rest_pos, rest_len, trigger, zero3, flagged, nseeds))
    return cases


def test_kernel_against_the_host_automaton_on_the_fuzz_tables(segment_emu, built, tmp_path):  # noqa: F811
    """the tables of the CPU fuzz (tools/segment_emu.cpp --fuzz, same seed, written out as numbers) through sq_debug_segment_seeds_tables: route
    1, the kernel plus the walk, against route 0, the host automaton in one go, case by case; the stretches flagged for a capacity are exactly
    the planted ones; totals equal to the harness's summary"""
    out = subprocess.run([str(segment_emu), "--fuzz", *FUZZ, "--write", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    want = fuzz_summary(out.stdout)
    check_fuzz_summary(want)
    cases = read_fuzz_cases(tmp_path / "cases.txt")
    assert len(cases) == int(FUZZ[0])
    tot = dict.fromkeys(("records", "seeds", "stretches", "again", "kept_with_nodes", "leading_kept_unused", "sens", "flagged"), 0)
    del tot["leading_kept_unused"]
    longest = extended = 0
    with squid_amd.Context() as ctx:
        for k, (rl, recs, disc4, part2, rest_off, rest_pos, rest_len, trigger, zero3, flagged, nseeds) in enumerate(cases):
            r1 = ctx.debug_segment_seeds_tables(rl, recs, disc4, part2, rest_off, rest_pos, rest_len, trigger, zero3, route=1)
            r0 = ctx.debug_segment_seeds_tables(rl, recs, disc4, part2, rest_off, rest_pos, rest_len, trigger, zero3, route=0)
            try:
                _same(r1, r0)
                assert r1["flagged"] == flagged and len(r0["seeds"]) == nseeds
            except AssertionError as e:
                raise AssertionError(f"case {k}: {e}") from e
            tot["records"] += len(recs); tot["seeds"] += len(r1["seeds"]); tot["stretches"] += r1["stretches"]; tot["again"] += r1["again"]; tot["kept_with_nodes"] += r1["kept_with_nodes"]
            tot["sens"] += r1["sens"]; tot["flagged"] += r1["flagged"]
            longest = max(longest, r1["longest"]); extended += r1["extended"]
    assert tot == {k: want[k] for k in tot}, (tot, want)
    assert longest == want["longest"] and extended == want["ext0"] + want["ext1"] + want["ext2"]


@pytest.mark.parametrize("cfg,gen,flags", [("T2", (), ()), ("C2", ("--interleave", "6"), ())])
def test_device_route_nodes_against_the_literal_automaton(built, synth, tmp_path, monkeypatch, cfg, gen, flags):
    """two inputs of tests/test_literal_build_node.py: the node table of the device route equals the literal reading of SegmentGraph.cpp"""
    from test_literal_build_node import GPU_CASES, _build_node_star_literal, _inputs

    _no_switch(monkeypatch)
    assert (cfg, gen, flags) in GPU_CASES
    pre, dump, chim, rec, read_len, ref_len = _inputs(built, synth, tmp_path, cfg, gen, flags)
    _, nodes, _, _ = _build_node_star_literal(rec, chim, read_len, ref_len, min_mapq=255)
    with squid_amd.Context() as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.segment_on_device()
        ctx.build_graph()
        got = [(int(n[0]), int(n[1]), int(n[2])) for n in ctx.graph(1)["nodes"]]
        assert _seg_route(ctx.timing())
    assert got == nodes


@pytest.mark.parametrize("env,call,want", [("0", True, False), ("1", False, True), (None, False, False), (None, True, True)])
def test_environment_override_and_call(built, synth, monkeypatch, env, call, want):
    """SQUID_SEGMENT_GPU, read when the context is created: =0 forbids the route whatever the call says, =1 forces it without the call"""
    _no_switch(monkeypatch)
    if env is not None:
        monkeypatch.setenv("SQUID_SEGMENT_GPU", env)
    pre = synth("T2")
    with squid_amd.Context() as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.segment_on_device(call)
        ctx.build_graph()
        ctx.order()
        text = ctx.sv_text()
        assert _seg_route(ctx.timing()) == want
    assert text == (squid_amd.ROOT / "tests" / "golden" / "T2_sv.txt").read_text()


def test_command_line_flag(built, synth, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2")
    for out, extra in (("p", ()), ("q", ("--device-segment",))):
        subprocess.check_call([str(built / "squid"), "-b", f"{pre}.bam", "-c", f"{pre}.chim.bam", "-o", str(tmp_path / out), "-G", "1", "-CO", "1", *extra], stdout=subprocess.DEVNULL)
    for suffix in ("_sv.txt", "_graph.txt", "_component_pri.txt"):
        assert (tmp_path / f"q{suffix}").read_bytes() == (tmp_path / f"p{suffix}").read_bytes(), suffix
    assert (tmp_path / "p_sv.txt").read_text().count("\n") > 1
    assert "--device-segment" in subprocess.run([str(built / "squid"), "--help"], capture_output=True, text=True).stdout


def test_bwa_context_accepts_the_call(built, synth, monkeypatch):
    _no_switch(monkeypatch)
    pre = synth("T2", "--bwa")
    texts = []
    for on in (False, True):
        with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
            ctx.load_bwa(f"{pre}.bam")
            ctx.segment_on_device(on)
            ctx.build_graph()
            ctx.order()
            texts.append(ctx.sv_text())
            t = ctx.timing()
            assert not any(k.startswith("k_seg_") for k in t) and not (set(SEG_ROWS) & set(t))
    assert texts[0] == texts[1] and texts[0].count("\n") > 1


def test_sharded_run_keeps_the_host_replay(built, synth, monkeypatch):
    """two virtual ranks: with the switch on every rank still replays on the host (the sharded hypotheses stay host work), same results"""
    from squid_amd.dist import VirtualWorld
    from test_gpu_parity import _sharded_contexts

    _no_switch(monkeypatch)
    pre = synth("T2")
    results = []
    for on in (False, True):
        ctxs = _sharded_contexts(pre, 2)
        try:
            for c in ctxs:
                c.segment_on_device(on)
            vw = VirtualWorld(ctxs)
            vw.build_graph()
            for c in ctxs:
                c.order()
            rows = vw.call_sv()
            results.append([(c.graph(1), c.graph(2), rows[r]) for r, c in enumerate(ctxs)])
            for c in ctxs:
                t = c.timing()
                assert not any(k.startswith("k_seg_") for k in t) and "host_segment_replay" in t and not (set(SEG_ROWS) & set(t))
        finally:
            for c in ctxs:
                c.close()
    assert results[0] == results[1] and len(results[0][0][0]["nodes"]) > 3


def test_clear_records_and_a_second_file(built, synth, tmp_path, monkeypatch):
    """sq_clear_records and another pair of files: the next graph gets a plan, tables and stretches of its own"""
    _no_switch(monkeypatch)
    monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")
    first, second = synth("T2"), synth("T2", "--seed", "4242")
    sv_path, dump = ou.run_oracle(built, second, tmp_path)
    with squid_amd.Context() as ctx:
        ctx.segment_on_device()
        ctx.load(f"{first}.bam", f"{first}.chim.bam")
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == (squid_amd.ROOT / "tests" / "golden" / "T2_sv.txt").read_text()
        t1 = ctx.timing()
        assert _seg_route(t1)
        ctx.clear_records()
        ctx.load(f"{second}.bam", f"{second}.chim.bam")
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        t2 = ctx.timing()
        assert _seg_route(t2) and _launches(t2, "k_seg_run") == 1
