"""FurtherCompressNode's walk over independent windows on the device (sq_compress_windows_on_device: the cut kernels of
squid_amd/csrc/sq_compress_stage.inc, k_further_compress launched over the window table, the id offsets behind it) against the rule of
tests/test_fc_windows_emu.py, against the per-chromosome route and the host function of the same context, and end to end against the
CPU oracle.  The rule itself, the state at the cuts and the kernel source emulated are the CPU file's."""
import subprocess

import pytest

import graphs
import oracle_util as ou
import squid_amd
import test_fc_windows_emu as fw
from test_fc_windows_emu import seed_inputs  # noqa: F401 -- (the module fixture that brings the seed list into its stage-4 form)
from test_graph_stage_fuzz import _differences, library_route

pytestmark = pytest.mark.gpu
SWITCH = "SQUID_COMPRESS_WINDOWS_GPU"


@pytest.fixture
def no_env(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)


def _rule_table(g):
    p = g["params"]
    return fw.table(fw.rule(fw.Lists(g["nodes"], g["edges"], p["dp"], p["di"]))[0])


def _device_table(ctx, g):
    return ctx.debug_fc_windows(g["nodes"], g["edges"], concord_dist_pos=g["params"]["dp"], concord_dist_idx=g["params"]["di"])


def _launches(t, row):
    return t[row]["launches"] if row in t else None


def test_window_table_of_the_hand_made_graphs(built, no_env):
    with squid_amd.Context() as ctx:
        for g in fw.hand_graphs():
            assert _device_table(ctx, g) == _rule_table(g), g["name"]


def test_window_table_of_the_seed_list(built, no_env, seed_inputs):  # noqa: F811
    gs = [g for g in (seed_inputs(s) for s in graphs.SEEDS) if g is not None]
    with squid_amd.Context() as ctx:
        bad = [g["name"] for g in gs if _device_table(ctx, g) != _rule_table(g)]
    assert not bad, bad[:10]


def test_window_table_of_the_random_family(built, no_env):
    with squid_amd.Context() as ctx:
        bad = [s for s in list(fw.RANDOM_FAMILY)[:200] if (lambda g: _device_table(ctx, g) != _rule_table(g))(fw.random_fc_graph(s))]
    assert not bad, bad[:10]


def _three_routes(ctx, g, first):
    """route 1 over windows against route 0 and route 1 per chromosome: every stage the routes hand out, rc (an assert of the reference shows
    as a stage), fallback and depth_ambiguous; returns the differences, the windows' result and its timing rows"""
    ctx.compress_windows_on_device(False)
    host = library_route(ctx, g, 0, first=first)
    ctx.timing_accumulate(True)  # (empties the table: the debug entry adds to it)
    per_chr = library_route(ctx, g, 1, first=first)
    assert "fc_windows" not in ctx.timing()
    ctx.compress_windows_on_device(True)
    ctx.timing_accumulate(True)
    windows = library_route(ctx, g, 1, first=first)
    t = ctx.timing()
    bad = _differences(per_chr, windows, g["name"] + " (windows / per chromosome)") + _differences(host, windows, g["name"] + " (windows / host)")
    if per_chr["fallback"] != windows["fallback"] or host["fallback"] != 0:
        bad.append(f"{g['name']}: fallback {host['fallback']} / {per_chr['fallback']} / {windows['fallback']}")
    if not host["depth_ambiguous"] == per_chr["depth_ambiguous"] == windows["depth_ambiguous"]:
        bad.append(f"{g['name']}: depth_ambiguous {host['depth_ambiguous']} / {per_chr['depth_ambiguous']} / {windows['depth_ambiguous']}")
    return bad, windows, t


def test_stage_routes_agree_on_the_seed_list(built, no_env, seed_inputs):  # noqa: F811
    """every graph of the seed list from its own first stage: nodes, edges, labels, weights, rc and fallback of route 1 over windows equal
    route 0 and route 1 per chromosome; fc_windows is the rule's count for the graph as it entered the stage"""
    bad = []
    with squid_amd.Context() as ctx:
        for seed in graphs.SEEDS:
            g = graphs.graph(seed)
            b, windows, t = _three_routes(ctx, g, g["first"])
            bad += b
            g4 = seed_inputs(seed)
            if g4 is not None and "final" in windows:
                if _launches(t, "fc_windows") != len(_rule_table(g4)) - 1:
                    bad.append(f"{g['name']}: fc_windows {_launches(t, 'fc_windows')}, the rule counts {len(_rule_table(g4)) - 1}")
            elif "final" not in windows and "fc_windows" in t:
                bad.append(f"{g['name']}: fc_windows without the stage")
    assert not bad, "\n".join(bad[:20])


def test_stage_routes_agree_on_the_hand_made_graphs(built, no_env):
    bad = []
    with squid_amd.Context() as ctx:
        for g in fw.hand_graphs():
            b, windows, t = _three_routes(ctx, g, 4)
            bad += b
            win = _rule_table(g)
            if _launches(t, "fc_windows") != len(win) - 1:
                bad.append(f"{g['name']}: fc_windows {_launches(t, 'fc_windows')}, the rule counts {len(win) - 1}")
            if _launches(t, "fc_longest_window") != max(b - a for a, b in zip(win, win[1:])):
                bad.append(f"{g['name']}: fc_longest_window {_launches(t, 'fc_longest_window')}")
            if "k_fc_cuts" not in t:
                bad.append(f"{g['name']}: no k_fc_cuts row")
    assert not bad, "\n".join(bad[:20])


def test_a_hub_in_a_middle_window_hands_the_whole_graph_back(built, no_env):
    by_name = {g["name"]: g for g in fw.hand_graphs()}
    with squid_amd.Context() as ctx:
        ctx.compress_windows_on_device()
        for k, fallback in ((256, 0), (257, 1)):
            g = by_name[f"hub_{k}_in_a_middle_window"]
            dev = library_route(ctx, g, 1, first=4)
            host = library_route(ctx, g, 0, first=4)
            assert dev["fallback"] == fallback and host["fallback"] == 0
            assert not _differences(host, dev, g["name"])


END_TO_END = [
    ("T2", (), (), {}, False),
    ("C1", (), (), {}, False),
    ("C5", ("--records", "300000", "--tsv", "1500", "--support", "2,8"), (), {}, False),
    ("T2", (), (), {}, True),
]


@pytest.mark.parametrize("cfg,gen,flags,params,bwa", END_TO_END)
def test_end_to_end_against_the_oracle(built, synth, tmp_path, cfg, gen, flags, params, bwa, no_env, monkeypatch):
    """the route on: every stage dump, the orders, the breakpoints and _sv.txt against the oracle, as the parity tests compare them"""
    from test_bwa import _oracle_bwa
    from test_gpu_parity import _compare

    if bwa:
        pre = synth(cfg, "--bwa", *gen)
        sv_path, dump = _oracle_bwa(built, pre, tmp_path, *flags)
        ctx = squid_amd.Context(star_mapq=False, min_mapqual=1, **params)
    else:
        monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")  # (the stage dumps are compared with Support / AvgDepth, as the parity tests do)
        pre = synth(cfg, *gen)
        sv_path, dump = ou.run_oracle(built, pre, tmp_path, *flags)
        ctx = squid_amd.Context(**params)
    with ctx:
        ctx.compress_windows_on_device()
        if bwa:
            ctx.load_bwa(f"{pre}.bam")
        else:
            ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.build_graph()
        sv = _compare(ctx, dump, sv_path)
        assert sv.count("\n") > 1
        t = ctx.timing()
        chroms = len({n[0] for n in ou.read_nodes(dump / "nodes_compress.txt")})
        assert _launches(t, "fc_windows") >= chroms and "k_fc_cuts" in t, sorted(t)
        if cfg == "C5":
            assert _launches(t, "fc_windows") > chroms, (_launches(t, "fc_windows"), chroms)
        ctx.compress_windows_on_device(False)
        ctx.reset()
        ctx.build_graph()
        ctx.order()
        assert ctx.sv_text() == sv and "fc_windows" not in ctx.timing()


@pytest.mark.parametrize("env,call,on", [("0", True, False), ("1", False, True), (None, False, False), (None, True, True)])
def test_environment_switch_forces_and_forbids(built, monkeypatch, env, call, on):
    if env is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, env)
    g = fw.hand_graphs()[0]
    with squid_amd.Context() as ctx:
        ctx.compress_windows_on_device(call)
        library_route(ctx, g, 1, first=4)
        assert ("fc_windows" in ctx.timing()) == on


def test_command_line_flag(built, synth, tmp_path, no_env):
    pre = synth("T2")
    for out, extra in (("p", ()), ("q", ("--device-compress-windows",))):
        subprocess.check_call([str(built / "squid"), *extra, "-b", f"{pre}.bam", "-c", f"{pre}.chim.bam", "-o", str(tmp_path / out)], stdout=subprocess.DEVNULL)
    assert (tmp_path / "p_sv.txt").read_text() == (tmp_path / "q_sv.txt").read_text() != ""
    assert "--device-compress-windows" in subprocess.run([str(built / "squid"), "--help"], capture_output=True, text=True).stdout
