"""BuildNode_STAR's segmentation automaton of the device route (squid_amd/csrc/sq_segment_stage.inc -- what sq_segment_on_device switches on: one
wave per active stretch from a fresh state on the guess that a node exists in front and is too far away to matter, a report of what the guess
rested on) on the CPU: the kernel source itself (sq_wave.h with SQ_WAVE_EMU, tools/segment_emu.cpp) and the library's walk over the stretch
reports against the library's host automaton in one go on the same tables -- the seeds in order and the nodes extended, place by place.  What
the restatement is about is what crosses a stretch boundary, so the harness counts the stretches, those run again behind the real last node and
those it kept, and every shape at which the kernel can go wrong; a fuzz without one of them would prove less than it says.  The GPU suite
runs the same source and the same tables on the device (tests/test_segment_gpu.py)."""
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def segment_emu(built, tmp_path_factory):
    exe = tmp_path_factory.mktemp("segment_emu") / "segment_emu"
    root = built.parent
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-DSQ_WAVE_EMU", "-I", str(root / "include"), "-o", str(exe), str(root / "tools" / "segment_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    return exe


FUZZ = ("240", "20261019")  # cases, seed (tests/test_segment_gpu.py runs the same tables on the device)
FUZZ_LINE = (r"(\d+) cases, (\d+) records, (\d+) blocks, (\d+) clusters, seeds (\d+), stretches (\d+), run again (\d+), kept with a node (\d+), kept with no node in front (\d+), longest stretch (\d+), "
             r"sens values (\d+), sens hits (\d+), nodes extended (\d+) (\d+) (\d+), margin lists of 2 63 64 65 cap cap\+1 entries (\d+) (\d+) (\d+) (\d+) (\d+) (\d+), flagged stretches (\d+) \(planted (\d+)\), "
             r"windows of 0 1 64 65 live elements (\d+) (\d+) (\d+) (\d+), clusters of more than 64 blocks (\d+), clusters split (\d+), single-record stretches (\d+), stretches the stream ends in (\d+), "
             r"clusters never passed (\d+), cases without a block (\d+), run again across a gap at read length 50 (\d+), chromosome changes (\d+) (\d+), clipped reads forward (\d+) reverse (\d+), "
             r"ConcordRest turned a candidate down (\d+), disCount rule fired (\d+) held back by a split (\d+), (\d+) differences")
FUZZ_KEYS = ("cases", "records", "blocks", "clusters", "seeds", "stretches", "again", "kept_with_nodes", "leading_kept", "longest", "sens", "sens_hits", "ext0", "ext1", "ext2", "m2", "m63", "m64", "m65", "mcap",
             "mover", "flagged", "planted", "w0", "w1", "w64", "w65", "big_clusters", "split_clusters", "single", "ends_inside", "never_passed", "no_block", "near_gap_again", "chr_mark", "chr_walk", "clip_fwd",
             "clip_rev", "rest_fail", "dense_fired", "dense_split", "differences")


def fuzz_summary(text):
    m = re.search(FUZZ_LINE, text)
    assert m, text[-2000:]
    return dict(zip(FUZZ_KEYS, (int(x) for x in m.groups())))


def check_fuzz_summary(s):
    assert s["cases"] == int(FUZZ[0]) and s["differences"] == 0, s
    assert s["again"] > 0 and s["kept_with_nodes"] > 0 and s["again"] < s["stretches"], s
    assert s["planted"] > 0 and s["flagged"] == s["planted"] == s["mover"], s  # (the harness also checks case by case that exactly the planted stretches are flagged)
    every = set(FUZZ_KEYS) - {"cases", "differences"}
    assert not [k for k in every if s[k] <= 0], {k: s[k] for k in every if s[k] <= 0}


def run_emu(exe, *args):
    out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    return out.stdout


def test_emulated_kernel_on_the_fuzz_tables(segment_emu):
    """240 random tables, seed 20261019 (harness build plus run: about half a minute on the build machine, the run itself under ten seconds):
    islands of concordant records with a discordant cluster in or next to them on one to four chromosomes, gaps that are zero coverage, just
    wider than a read, or none.  Every twelfth case plants one of: no discordant block at all; margin lists of 63, 64 and 65 entries; of
    exactly the cap; of one more (the stretch is flagged and run again on the host -- planted == flagged); windows of 64, 65 and 1 live
    elements; read length 50 with a break candidate 52..58 bases behind the last node of the stretch in front (guess wrong, run again); a
    pending node start equal to the end of the node in front on another chromosome (the comparison without a chromosome test: a sens hit)
    and one equal to nothing (a sens value of a kept stretch); ConcordRest cover that turns a candidate down only once its term is added;
    stretches of a single record and leading stretches that emit nothing (kept with no node in front); a record that passes clusters of
    two chromosomes with a node start pending; clusters no record passes; a stream that ends inside a stretch.  Counted besides: margin
    lists of a single block (2 entries -- a list cannot have 1: every block gives its start and its end), clusters of more than 64 blocks,
    clusters split into sub-clusters, clipped reads of both strands feeding the margin list, each of the three places that extend a node,
    the disCount rule firing and held back by a split.  Every counter must be positive, with 0 differences"""
    check_fuzz_summary(fuzz_summary(run_emu(segment_emu, "--fuzz", *FUZZ)))


def test_another_seed_has_no_difference_either(segment_emu):
    s = fuzz_summary(run_emu(segment_emu, "--fuzz", "120", "7"))
    assert s["differences"] == 0 and s["again"] > 0 and s["kept_with_nodes"] > 0, s
