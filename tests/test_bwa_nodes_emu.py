"""BuildNode_BWA's record automaton of the `--bwa` device route (squid_amd/csrc/sq_bwa_nodes.inc -- what sq_bwa_nodes_on_device switches on: the
stream cut at every gap in the coverage by tile-local prefix maxima, the discordant records compacted into a list, one wave per stretch running
the automaton from a fresh state on the host's guesses) on the CPU: the kernel source itself (sq_wave.h with SQ_WAVE_EMU,
tools/bwa_nodes_emu.cpp) and the library's walk over the stretch reports against the library's host automaton in one go on the same batch --
the seeds in order, the final read length, the records that feed Reads, the flushes that emitted a node, the marks the zero-coverage rule
closed.  What the restatement is about is what crosses a gap: the harness counts the stretches, those of a single record and those that had
to be run again from the real state, and a sample without more than one stretch would prove nothing.  The GPU suite runs the same source on
the device (tests/test_bwa_nodes_gpu.py)."""
import re
import struct
import subprocess

import pytest

import bamwriter as bw
import shapes
from test_bwa_stage_gpu import A, B_, FIRST, MATE_REV, MATE_UNMAPPED, PAIRED, PROPER, REV, SECOND, handmade_records


@pytest.fixture(scope="module")
def nodes_emu(built, tmp_path_factory):
    exe = tmp_path_factory.mktemp("bwa_nodes_emu") / "bwa_nodes_emu"
    root = built.parent
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-DSQ_WAVE_EMU", "-I", str(root / "include"), "-o", str(exe), str(root / "tools" / "bwa_nodes_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    return exe


SAMPLE_LINE = (r"(\d+) records, seeds (\d+), Reads records (\d+), stretches (\d+), run again (\d+), single-record stretches (\d+), longest stretch (\d+), flushes that emitted a node (\d+), "
               r"marks closed by the zero-coverage rule (\d+), cover tests failed (\d+), read length (\d+), (\d+) differences")
SAMPLE_KEYS = ("records", "seeds", "reads", "stretches", "again", "single", "longest", "flush_nodes", "marks_closed", "cover_fails", "read_len", "differences")


def sample_summary(text):
    m = re.search(SAMPLE_LINE, text)
    assert m, text[-2000:]
    return dict(zip(SAMPLE_KEYS, (int(x) for x in m.groups())))


FUZZ = ("60", "20261018")  # cases, seed (tests/test_bwa_nodes_gpu.py runs the same tables on the device)
FUZZ_LINE = (r"(\d+) cases, (\d+) records, seeds (\d+), Reads records (\d+), stretches (\d+), run again (\d+), single-record stretches (\d+), longest stretch (\d+), flushes that emitted a node (\d+), "
             r"marks closed by the zero-coverage rule (\d+), cover tests failed (\d+), fallback cases (\d+) \(planted unsorted (\d+)\), tables of 0 1 63 64 65 129 records (\d+), "
             r"islands that end in a discordant run (\d+), discordant runs longer than 64 records (\d+), cuts at record 8 (\d+), records without a block at a chromosome change (\d+), "
             r"clipped reads forward (\d+) reverse (\d+), stale rightmost tables (\d+), (\d+) differences")
FUZZ_KEYS = ("cases", "records", "seeds", "reads", "stretches", "again", "single", "longest", "flush_nodes", "marks_closed", "cover_fails", "fallbacks", "planted", "named_sizes", "run_at_end", "long_runs",
             "cut_at_8", "zero_blocks", "clipped_fwd", "clipped_rev", "stale", "differences")


def fuzz_summary(text):
    m = re.search(FUZZ_LINE, text)
    assert m, text[-2000:]
    return dict(zip(FUZZ_KEYS, (int(x) for x in m.groups())))


def run_emu(exe, *args):
    out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    return out.stdout


@pytest.mark.parametrize("cfg,gen", [("T2", ()), ("T2", ("--seed", "4242")), ("C2", ())])
def test_emulated_kernels_equal_the_host_automaton_on_the_samples(nodes_emu, synth, cfg, gen):
    pre = synth(cfg, "--bwa", *gen)
    s = sample_summary(run_emu(nodes_emu, f"{pre}.bam"))
    assert s["differences"] == 0
    assert s["seeds"] > 0 and s["stretches"] > 1 and s["flush_nodes"] >= 1 and s["reads"] > 0, s


# ---- the hand-made BAM of tests/test_bwa_stage_gpu.py plus what makes a guess wrong
def handmade_node_records():
    """handmade_records() plus `early`: a concordant pair at the start of contig B, in front of a gap.  The gap record behind it (`before0`,
    B:300) starts a stretch on the guess that it finds zero coverage; in the stream it does not -- the end of the discordant run of contig A
    (3066) outlives the chromosome, and 300 is not more than a read length behind it -- so that stretch is run again from the real state.  The
    dense discordant runs of the base file (A:3000.., B:2000..) each end in a node whose mark the zero-coverage rule closes."""
    extra = [
        bw.record("early", B_, 20, 60, PAIRED | PROPER | MATE_REV | FIRST, "60M", B_, 60),
        bw.record("early", B_, 60, 60, PAIRED | PROPER | REV | SECOND, "60M", B_, 20),
    ]
    return sorted(handmade_records() + extra, key=lambda r: (struct.unpack_from("<i", r, 4)[0] & 0x7fffffff, struct.unpack_from("<i", r, 8)[0]))  # (stable: equal places keep their order)


def write_handmade_nodes(path):
    bw.write_bam(str(path), [("chrA", 20000), ("chrB", 10000)], handmade_node_records())


def test_emulated_kernels_on_the_hand_made_bam(nodes_emu, tmp_path):
    write_handmade_nodes(tmp_path / "hand.bam")
    s = sample_summary(run_emu(nodes_emu, tmp_path / "hand.bam"))
    assert s["differences"] == 0
    assert s["again"] >= 1 and s["marks_closed"] >= 1 and s["flush_nodes"] >= 2 and s["seeds"] >= 2 and s["stretches"] >= 4, s
    # without `early` no guess is wrong
    bw.write_bam(str(tmp_path / "base.bam"), [("chrA", 20000), ("chrB", 10000)], handmade_records())
    t = sample_summary(run_emu(nodes_emu, tmp_path / "base.bam"))
    assert t["again"] == 0 and t["stretches"] == s["stretches"] - 1, (s, t)


def check_fuzz_summary(s):
    assert s["cases"] == 60 and s["differences"] == 0
    assert s["again"] > 0 and s["single"] > 0, s
    assert 1 <= s["planted"] <= 15 and s["fallbacks"] == s["planted"], s  # (the harness also checks case by case that exactly the planted tables fall back)
    assert s["named_sizes"] >= 6, s
    assert min(s["run_at_end"], s["long_runs"], s["cut_at_8"], s["zero_blocks"], s["clipped_fwd"], s["clipped_rev"], s["stale"], s["cover_fails"], s["flush_nodes"], s["marks_closed"], s["seeds"]) > 0, s


def test_emulated_kernels_on_the_fuzz_tables(nodes_emu):
    """random record tables: islands of coverage with gaps that cut the stream, gaps that only clear the coverage and none; tables of 0, 1, 63,
    64, 65 and 129 records; stretches of a single record; a discordant run that ends on the last record of a stretch; runs of more than 64
    discordant records; a cut at record 8 with the read length still rising over records 0-4; records without a block at a chromosome change; a
    discordant run far to the right on chromosome 0 whose end decides the zero-coverage test on chromosome 1 (stretches are run again); clipped
    reads on both strands next to a run; concordant cover deep enough to fail the support test; a few tables with two passing records out of
    order, which the kernels hand back"""
    check_fuzz_summary(fuzz_summary(run_emu(nodes_emu, "--fuzz", *FUZZ)))


# four of the 16 random --bwa shapes: the 50-base reads, the 250-base reads, the longest Reads list, the most odd pairs
SHAPE_SEEDS = [14, 2, 6, 12]


def test_the_four_shape_seeds_are_what_they_are_named_for():
    drawn = {s: shapes.draw_bwa(s)[0] for s in shapes.BWA_SEEDS}
    assert shapes.read_len(drawn[14]) == 50 == min(shapes.read_len(g) for g in drawn.values())
    assert shapes.read_len(drawn[2]) == 250 == max(shapes.read_len(g) for g in drawn.values())
    odd = {s: float(g[g.index("--odd-pair-frac") + 1]) for s, g in drawn.items() if "--odd-pair-frac" in g}
    assert max(odd, key=odd.get) == 12


@pytest.mark.parametrize("seed", SHAPE_SEEDS)
def test_emulated_kernels_on_the_shape_seeds(built, nodes_emu, tmp_path, seed):
    gen, _, _ = shapes.draw_bwa(seed)
    rc, _ = shapes.generate(built, tmp_path / "s", gen)
    assert rc == 0, (seed, gen)
    s = sample_summary(run_emu(nodes_emu, tmp_path / "s.bam"))
    assert s["differences"] == 0 and s["seeds"] > 0 and s["stretches"] > 1, (seed, s)
