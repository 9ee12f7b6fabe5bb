"""The `--bwa` stages of the device route (squid_amd/csrc/sq_bwa_stage.inc: the class byte of every record and the node depth loop of
BuildNode_BWA as a prefix maximum -- what sq_bwa_on_device switches on) on the CPU: the kernel source itself, the class kernel lane by lane
and the depth kernels as waves of 64 coroutines (sq_wave.h with SQ_WAVE_EMU, tools/bwa_stage_emu.cpp), against the library's host loops on
the same batch -- both class bits of every record, Support and the integer sum of every node.  What the restatement is about are the blocks
the one-way cursor holds in front of a later node than their own (ledger W6): the harness counts them (against a count by the definition),
and a sample without one would prove nothing.  The GPU suite runs the same source on the device (tests/test_bwa_stage_gpu.py)."""
import random
import re
import subprocess

import pytest

import squid_amd


@pytest.fixture(scope="module")
def emu(built, tmp_path_factory):
    exe = tmp_path_factory.mktemp("bwa_emu") / "bwa_stage_emu"
    root = built.parent
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-DSQ_WAVE_EMU", "-I", str(root / "include"), "-o", str(exe), str(root / "tools" / "bwa_stage_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    return exe


FUZZ = ("60", "20261017")  # cases, seed (tests/test_bwa_stage_gpu.py runs the same tables on the device)
FUZZ_LINE = (r"(\d+) cases, (\d+) blocks, held (\d+) \(share [0-9.]+\), counted (\d+), (\d+) of (\d+) list lengths, one node per chromosome (\d+), nodes of 1-4 bases (\d+), "
             r"one node takes every block (\d+), empty chromosome between used ones (\d+), most nodes under one wave (\d+), exact end (\d+), one beyond (\d+), one before (\d+), "
             r"far block holds two tiles (\d+), block beyond the last node (\d+), fallback cases (\d+)")
FUZZ_KEYS = ("cases", "blocks", "held", "counted", "lengths", "lengths_of", "one_per_chr", "tiny", "single", "empty_chr", "dense", "exact_end", "one_beyond", "one_before", "far_tile",
             "dead_tail", "fallbacks")


def fuzz_summary(text):
    m = re.search(FUZZ_LINE, text)
    assert m, text[-2000:]
    return dict(zip(FUZZ_KEYS, (int(x) for x in m.groups())))


@pytest.mark.parametrize("cfg,gen", [("T2", ()), ("C2", ()), ("T2", ("--seed", "4242"))])
def test_emulated_stages_equal_the_host_loops_on_the_samples(emu, synth, cfg, gen):
    pre = synth(cfg, "--bwa", *gen)
    out = subprocess.run([str(emu), f"{pre}.bam"], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    m = re.search(r"(\d+) records, (\d+) blocks, READS records (\d+) \((\d+) blocks in Reads\), breakpoint-support records (\d+), records named like a rebuilt fragment (\d+) of (\d+) names, "
                  r"(\d+) nodes, held blocks (\d+)", out.stdout)
    assert m, out.stdout
    records, blocks, reads, reads_blocks, p3, named, names, nodes, held = (int(x) for x in m.groups())
    assert 0 < reads < records and 0 < p3 < reads and reads_blocks > reads  # (both filters drop something; spliced reads are there)
    assert named > 0 and names > 0  # (the name test had something to decide)
    assert held > 0, "no block held by the cursor on this sample: exchange the sample"


def test_emulated_depth_kernels_on_fuzzed_tables(emu):
    """node tables and Reads lists made to order (tools/bwa_stage_emu.cpp, make_case): no difference in any Support or sum, the fallback flag exactly
    on the cases whose chromosomes go down along Reads; the generator's guarantees, which the harness checks on the tables and prints"""
    out = subprocess.run([str(emu), "--fuzz", *FUZZ], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    s = fuzz_summary(out.stdout)
    assert s["cases"] >= 60
    assert s["lengths"] == s["lengths_of"] >= 14  # 0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025 and a few thousand
    assert min(s["one_per_chr"], s["tiny"], s["single"], s["empty_chr"]) > 0
    assert s["dense"] > 64
    assert min(s["exact_end"], s["one_beyond"], s["one_before"]) > 100
    assert s["far_tile"] > 0 and s["dead_tail"] > 0
    assert 4 * s["held"] >= s["blocks"] and s["counted"] > 1000
    assert 0 < s["fallbacks"] < s["cases"] // 2


def _literal_depth_loop(nodes, reads):
    """SegmentGraph.cpp:1180-1200 as it stands: one cursor into Reads that never goes back"""
    support, sums, it = [0] * len(nodes), [0] * len(nodes), 0
    for i, (chrom, pos, length) in enumerate(nodes):
        while it < len(reads):
            c, p, m = reads[it]
            if c == chrom and p >= pos and p + m <= pos + length:
                support[i] += 1
                sums[i] += m
            elif p >= pos + length or c != chrom:
                break
            it += 1
    return support, sums


def _read_cases(path):
    toks = path.read_text().split()
    at, cases = 0, []
    while at < len(toks):
        assert toks[at] == "case"
        nn, nr = int(toks[at + 1]), int(toks[at + 2])
        v = [int(x) for x in toks[at + 3:at + 3 + 3 * (nn + nr)]]
        at += 3 + 3 * (nn + nr)
        cases.append(([tuple(v[3 * i:3 * i + 3]) for i in range(nn)], [tuple(v[3 * (nn + j):3 * (nn + j) + 3]) for j in range(nr)]))
    return cases


def test_literal_loop_equals_route_0(emu, built, tmp_path):
    """the loop of the reference, a dozen lines of Python, against route 0 of sq_debug_bwa_depth (the library's host loop, no device) on the fuzz
    tables, the ones with chromosomes out of order included, and on a few lists in random order"""
    out = subprocess.run([str(emu), "--fuzz", *FUZZ, "--write", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    cases = _read_cases(tmp_path / "cases.txt")
    assert len(cases) == 60
    rng = random.Random(7)
    for nodes, reads in cases[:6]:
        shuffled = list(reads)
        rng.shuffle(shuffled)
        cases.append((nodes, shuffled))
    counted = 0
    for k, (nodes, reads) in enumerate(cases):
        r = squid_amd.debug_bwa_depth(nodes, reads, route=0)
        assert (r["support"], r["sums"]) == _literal_depth_loop(nodes, reads), k
        counted += sum(r["support"])
    assert counted > 1000
