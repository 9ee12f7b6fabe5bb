"""The chimeric graph stages on the device (sq_chimeric_on_device: RawEdgesChim and ExactBreakpoint + CountTop as kernels over a fragment
table in HBM, squid_amd/csrc/sq_chim_stage.inc) against the CPU oracle and against the host route of the same context: every stage
snapshot, the orders, the breakpoint table and `_sv.txt` identical, with ZERO fallbacks to the host on the samples named here.  The
CPU suite runs the same kernel source emulated (tests/test_chim_stage_emu.py)."""
import re
import subprocess
from pathlib import Path

import pytest

import oracle_util as ou
import squid_amd
from test_gpu_parity import LOW_SUPPORT_SAMPLES, PARAM_SETS, _compare, _sharded_contexts, _ShardView

pytestmark = pytest.mark.gpu
SQ_E_ASSERT = -6


def _route(timing):
    """('device' | 'host', fallbacks) from a context's timing table"""
    kernels = {k for k, v in timing.items() if k.startswith("k_chim_") and v["launches"] > 0}
    host = {"host_chimeric_edges", "host_exact_breakpoints"} & set(timing)
    if kernels:
        assert not host or timing["chim_device_fallback"]["launches"] > 0, timing.keys()
        return "device", timing["chim_device_fallback"]["launches"]
    assert host == {"host_chimeric_edges", "host_exact_breakpoints"} and "chim_device_fallback" not in timing, timing.keys()
    return "host", 0


SAMPLES = [
    ("T2", (), (), {}),
    ("C2", (), (), {}),
    ("C2", ("--support", "2,6"), ("-w", "1", "-a", "50"), dict(min_edge_weight=1, max_allowed_degree=50)),
    ("C2", ("--support", "2,6"), (), {}),
] + [s for s in LOW_SUPPORT_SAMPLES if s[0] == "C5"] + [
    ("C5g", ("--records", "200000", "--tsv", "400"), ("-w", "1", "-a", "50"), dict(min_edge_weight=1, max_allowed_degree=50)),
]


@pytest.mark.parametrize("cfg,gen,flags,params", SAMPLES)
def test_device_route_equals_the_oracle_and_the_host_route(built, synth, tmp_path, monkeypatch, cfg, gen, flags, params):
    monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")
    monkeypatch.delenv("SQUID_CHIM_STAGES_GPU", raising=False)
    pre = synth(cfg, *gen)
    sv_path, dump = ou.run_oracle(built, pre, tmp_path, *flags)
    with squid_amd.Context(**params) as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.chimeric_on_device()
        ctx.build_graph()
        sv = _compare(ctx, dump, sv_path)
        t = ctx.timing()
        assert _route(t) == ("device", 0), t.keys()
        assert "chim_soft_fragments" in t and "chim_upload" in t
        for on in (False, True):
            ctx.reset()
            ctx.chimeric_on_device(on)
            ctx.build_graph()
            ctx.order()
            assert ctx.sv_text() == sv
            assert _route(ctx.timing()) == (("device", 0) if on else ("host", 0))


@pytest.mark.parametrize("flags,params", PARAM_SETS)
def test_device_route_with_other_parameters(built, synth, tmp_path, monkeypatch, flags, params):
    """(-dp / -di change edge_discordant, which both stages evaluate on the device)"""
    monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")
    pre = synth("T2")
    sv_path, dump = ou.run_oracle(built, pre, tmp_path, *flags)
    with squid_amd.Context(**params) as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.chimeric_on_device()
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        assert _route(ctx.timing()) == ("device", 0)


def test_device_route_on_every_rank_of_a_sharded_run(built, synth, tmp_path, monkeypatch):
    from squid_amd.dist import VirtualWorld

    monkeypatch.delenv("SQUID_EXACT_DEPTH", raising=False)
    pre = synth("T2")
    sv_path, dump = ou.run_oracle(built, pre, tmp_path)
    ctxs = _sharded_contexts(pre, 3, [(0, 1), (1, 2), (2, 3)])
    try:
        for c in ctxs:
            c.chimeric_on_device()
        vw = VirtualWorld(ctxs)
        vw.build_graph()
        for c in ctxs:
            c.order()
        rows = vw.call_sv()
        for r, c in enumerate(ctxs):
            _compare(_ShardView(c, rows[r]), dump, sv_path, depth_exact=False)
            assert _route(c.timing()) == ("device", 0)
    finally:
        for c in ctxs:
            c.close()


def test_bwa_context_ignores_the_switch(built, synth):
    pre = synth("T2", "--bwa")
    texts = []
    for on in (False, True):
        with squid_amd.Context(star_mapq=False, min_mapqual=1) as ctx:
            ctx.load_bwa(f"{pre}.bam")
            ctx.chimeric_on_device(on)
            ctx.build_graph()
            ctx.order()
            texts.append(ctx.sv_text())
            assert not any(k.startswith("k_chim_") for k in ctx.timing())
    assert texts[0] == texts[1] and texts[0].count("\n") > 1


def _read_cases(path):
    toks = Path(path).read_text().split()
    at, cases = 0, []

    def take(n):
        nonlocal at
        v = [int(x) for x in toks[at:at + n]]
        at += n
        return v

    while at < len(toks):
        assert toks[at] == "case"
        at += 1
        n1, n2, nf, _, ne = take(5)
        nodes1 = [tuple(take(3)) for _ in range(n1)]
        nodes2 = [tuple(take(3)) for _ in range(n2)]
        frags = []
        for _ in range(nf):
            na, nb, atot, btot = take(4)
            a = [tuple(take(6)) for _ in range(na)]
            b = [tuple(take(6)) for _ in range(nb)]
            frags.append((a, b, atot, btot))
        edges = [tuple(take(4)) for _ in range(ne)]
        cases.append((nodes1, nodes2, frags, edges))
    return cases


def test_fuzzed_tables_on_the_device(built, tmp_path):
    """the cases of the CPU fuzz (tools/chim_stage_emu.cpp --fuzz, same seed; written out as numbers) through sq_debug_chim_stages: host route and
    device route on the same tables -- no difference in the raw edges, the trimmed blocks behind either stage, the per-edge breakpoint lists or the
    return codes (the cases that trip the reference's assert included), and the device counts the soft fragments the host's classification counts"""
    exe = tmp_path / "chim_stage_emu"
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-DSQ_WAVE_EMU", "-I", str(squid_amd.ROOT / "include"), "-o", str(exe), str(squid_amd.ROOT / "tools" / "chim_stage_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    out = subprocess.run([str(exe), "--fuzz", "60", "20261016", "--write", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    m = re.search(r"(\d+) fragments, chim_soft_fragments stage 1: (\d+) \(share [0-9.]+\), stage 2: (\d+) .* (\d+) cases trip", out.stdout)
    want_frags, want_s1, want_s2, want_asserts = (int(x) for x in m.groups())
    cases = _read_cases(tmp_path / "cases.txt")
    assert len(cases) == 60
    frags = s1 = s2 = asserts = biggest = 0
    with squid_amd.Context() as ctx:
        for k, (nodes1, nodes2, fr, edges) in enumerate(cases):
            r = ctx.debug_chim_stages(nodes1, nodes2, fr, edges)
            assert r["differences"] == 0 and r["host_rc"] == r["device_rc"], (k, r)
            if r["host_rc"] == SQ_E_ASSERT:
                asserts += 1
                continue
            assert r["host_rc"] == 0, (k, r)
            assert (r["device_soft_1"], r["device_soft_2"]) == (r["host_soft_1"], r["host_soft_2"]), (k, r)
            frags += len(fr); s1 += r["device_soft_1"]; s2 += r["device_soft_2"]
    assert (frags, s1, s2, asserts) == (want_frags, want_s1, want_s2, want_asserts)
    assert 4 * s1 >= frags and 4 * s2 >= frags


def test_block_outside_the_node_table_reports_the_reference_assert_on_both_routes(built):
    """a block behind the last node of the table has no node to be counted for: RawEdgesChim's edge (i, i + 1) is out of range, the reference asserts
    (SegmentGraph.cpp:1410); host route and device route return SQ_E_ASSERT"""
    nodes = [(0, 0, 500), (0, 500, 500)]
    frags = [([(0, 100, 0, 50, 50, 0), (0, 600, 50, 50, 50, 0)], [], 150, 150), ([(0, 2000, 0, 40, 40, 0)], [(0, 300, 0, 50, 50, 1)], 150, 150)]
    with squid_amd.Context() as ctx:
        r = ctx.debug_chim_stages(nodes, nodes, frags, [(0, 1, 0, 1)])
        assert r["host_rc"] == SQ_E_ASSERT and r["device_rc"] == SQ_E_ASSERT and r["differences"] == 0, r
        r = ctx.debug_chim_stages(nodes, nodes, frags[:1], [(0, 1, 0, 1)])
        assert r["host_rc"] == 0 and r["device_rc"] == 0 and r["differences"] == 0, r


def test_command_line_flag(built, synth, tmp_path, monkeypatch):
    monkeypatch.delenv("SQUID_CHIM_STAGES_GPU", raising=False)
    pre = synth("T2")
    for out, extra in (("p", ()), ("q", ("--device-chimeric",))):
        subprocess.check_call([str(built / "squid"), "-b", f"{pre}.bam", "-c", f"{pre}.chim.bam", "-o", str(tmp_path / out), *extra], stdout=subprocess.DEVNULL)
    assert (tmp_path / "q_sv.txt").read_bytes() == (tmp_path / "p_sv.txt").read_bytes()
    assert (tmp_path / "p_sv.txt").read_text().count("\n") > 1


def test_environment_override(built, synth, monkeypatch):
    """SQUID_CHIM_STAGES_GPU, read when the context is created: =0 forbids the device route whatever the call says, =1 forces it without the call"""
    pre = synth("T2")
    texts = []
    for env, call, want in (("0", True, "host"), ("1", False, "device")):
        monkeypatch.setenv("SQUID_CHIM_STAGES_GPU", env)
        with squid_amd.Context() as ctx:
            ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
            ctx.chimeric_on_device(call)
            ctx.build_graph()
            ctx.order()
            texts.append(ctx.sv_text())
            assert _route(ctx.timing()) == (want, 0)
    assert texts[0] == texts[1]


def test_forced_fallback_takes_the_host_route_with_the_same_results(built, synth, tmp_path, monkeypatch):
    """SQUID_CHIM_SOFT_MAX=0: T2's stage 1 has soft fragments, more than the (debug) bound allows -- the stage is handed back to the host, counted
    once, and the breakpoint stage follows it there; results as ever"""
    monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")
    monkeypatch.setenv("SQUID_CHIM_SOFT_MAX", "0")
    pre = synth("T2")
    sv_path, dump = ou.run_oracle(built, pre, tmp_path)
    with squid_amd.Context() as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.chimeric_on_device()
        ctx.build_graph()
        _compare(ctx, dump, sv_path)
        t = ctx.timing()
        assert t["chim_device_fallback"]["launches"] == 1
        assert {"host_chimeric_edges", "host_exact_breakpoints"} <= set(t)
