"""The chimeric graph stages of the device route (squid_amd/csrc/sq_chim_stage.inc: RawEdgesChim, ExactBreakpoint + CountTop -- what
sq_chimeric_on_device switches on) on the CPU: the kernel source itself, lane by lane and CountTop's wave as 64 coroutines (sq_wave.h with
SQ_WAVE_EMU, tools/chim_stage_emu.cpp), against the library's host functions on the same fragments -- the reduced raw-edge list, the trimmed
blocks of every fragment behind each stage and the per-edge breakpoint lists in order.  The one thing carried from fragment to fragment is
LocateRead's start position; a fragment whose first block depends on it is *soft* (first_block_fit of sq_graph.cpp is the definition) and
the harness counts those with the host's classification: a sample without a soft fragment would prove nothing about the chain.  The GPU
suite runs the same source on the device (tests/test_chim_stage_gpu.py)."""
import re
import subprocess

import pytest

import oracle_util as ou


@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    exe = tmp_path_factory.mktemp("chim_emu") / "chim_stage_emu"
    root = built.parent
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-DSQ_WAVE_EMU", "-I", str(root / "include"), "-o", str(exe), str(root / "tools" / "chim_stage_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    return exe


# (sample, generator flags, soft fragments of stage 1 the sample must at least have)
SAMPLES = [
    ("T2", (), 5),
    ("C2", (), 5),
    ("C5", ("--records", "300000", "--tsv", "1500", "--support", "2,8"), 0),
]


@pytest.mark.parametrize("cfg,gen,min_soft", SAMPLES)
def test_emulated_stages_equal_the_host_stages_on_the_samples(emu, built, synth, tmp_path, cfg, gen, min_soft):
    pre = synth(cfg, *gen)
    _, dump = ou.run_oracle(built, pre, tmp_path)
    out = subprocess.run([str(emu), f"{pre}.chim.bam", str(dump)], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    m = re.search(r"soft fragments by first_block_fit: stage 1 (\d+), stage 2 (\d+); chim_soft_fragments of the emulated run: stage 1 (\d+), stage 2 (\d+)", out.stdout)
    assert m, out.stdout
    host1, host2, emu1, emu2 = (int(x) for x in m.groups())
    assert (emu1, emu2) == (host1, host2)
    assert host1 >= min_soft, (cfg, host1)
    n = re.search(r"(\d+) final edges, (\d+) raw edges after the reduction, (\d+) edges with breakpoint lists", out.stdout)
    assert n and int(n.group(2)) > 0 and int(n.group(3)) > 0, out.stdout  # (both stages had something to compare)


def test_emulated_stages_on_fuzzed_tables(emu):
    """random node tables that tile a few chromosomes (nodes shorter than 5 bases included), one per stage, random key-sorted final edges, fragments
    whose blocks lie on, within 5 bases of, across and outside node boundaries: no difference; at least a quarter of ALL fuzzed fragments are
    soft in each stage; a hit group of more than 64 pairs (CountTop's wave loop wraps); cases on which the host route reports the reference's
    assert report the same code by the emulated route (a different code is a difference)"""
    out = subprocess.run([str(emu), "--fuzz", "60", "20261016"], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    m = re.search(r"(\d+) cases, (\d+) fragments, chim_soft_fragments stage 1: (\d+) \(share ([0-9.]+)\), stage 2: (\d+) \(share ([0-9.]+)\), (\d+) cases trip the reference's assert "
                  r"on both routes, largest hit group (\d+) pairs", out.stdout)
    assert m, out.stdout
    cases, frags, s1, share1, s2, share2, asserts, biggest = m.groups()
    assert int(frags) > 2000
    assert 4 * int(s1) >= int(frags) and 4 * int(s2) >= int(frags), (s1, s2, frags)
    assert int(biggest) > 64
    assert 0 < int(asserts) < int(cases) // 2
