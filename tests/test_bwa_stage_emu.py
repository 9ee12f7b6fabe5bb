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


SAMPLE_LINE = (r"(\d+) records, (\d+) blocks, READS records (\d+) \((\d+) blocks in Reads\), breakpoint-support records (\d+), records named like a rebuilt fragment (\d+) of (\d+) names, "
               r"(\d+) nodes, held blocks (\d+), left-hand READS records (\d+), READS records below -mq (\d+): (\d+)")
SAMPLE_KEYS = ("records", "blocks", "reads", "reads_blocks", "p3", "named", "names", "nodes", "held", "left", "mq", "below_mq")


def sample_summary(text):
    """the harness's line about a BAM file.  reads: records that feed Reads; p3: records the breakpoint support looks at; left: left-hand records
    of a pair among the READS records of MAPQ >= -mq; below_mq: READS records of MAPQ below -mq (they feed Reads and are not looked at)"""
    m = re.search(SAMPLE_LINE, text)
    assert m, text[-2000:]
    return dict(zip(SAMPLE_KEYS, (int(x) for x in m.groups())))


@pytest.mark.parametrize("cfg,gen", [("T2", ()), ("C2", ()), ("T2", ("--seed", "4242"))])
def test_emulated_stages_equal_the_host_loops_on_the_samples(emu, synth, cfg, gen):
    pre = synth(cfg, "--bwa", *gen)
    out = subprocess.run([str(emu), f"{pre}.bam"], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    records, blocks, reads, reads_blocks, p3, named, names, nodes, held = (sample_summary(out.stdout)[k] for k in SAMPLE_KEYS[:9])
    assert 0 < reads < records and 0 < p3 < reads and reads_blocks > reads  # (both filters drop something; spliced reads are there)
    assert named > 0 and names > 0  # (the name test had something to decide)
    assert held > 0, "no block held by the cursor on this sample: exchange the sample"


def test_emulated_class_byte_on_the_hand_made_bam(emu, tmp_path):
    """the generator's files never have a multi-mapper (XA) of MAPQ other than 0, and no unmapped record with a MAPQ: there the first test of
    class_of is decided by MAPQ alone.  The hand-made BAM of tests/test_bwa_stage_gpu.py has one record failing each factor of the two filters
    (XA at MAPQ 60, IH 2, MAPQ 0, MAPQ 5 below -mq 10, duplicate, unmapped, mate to the right, both mates at one position, a rebuilt fragment's
    name); with it an unmapped record that carries MAPQ 37 and a record of MAPQ 60 without a reference, a flag or a block -- the emulated class
    byte against the host loops at -mq 10"""
    import struct

    import bamwriter as bw
    from test_bwa_stage_gpu import A, FIRST, MATE_REV, MATE_UNMAPPED, PAIRED, REV, SECOND, UNMAPPED, handmade_records

    extra = [bw.record("x_unmapped_q", A, 2916, 60, PAIRED | MATE_REV | FIRST, "60M", A, 3010),
             bw.record("x_unmapped_q", A, 3010, 37, PAIRED | UNMAPPED | REV | SECOND, [], A, 2916, lseq=60),
             bw.record("x_no_reference", -1, -1, 60, PAIRED | MATE_UNMAPPED | FIRST, [], -1, -1, lseq=60)]
    recs = sorted(handmade_records() + extra, key=lambda r: (struct.unpack_from("<i", r, 4)[0] & 0x7fffffff, struct.unpack_from("<i", r, 8)[0]))  # (RefID -1 last)
    bw.write_bam(f"{tmp_path}/hand.bam", [("chrA", 20000), ("chrB", 10000)], recs)
    out = subprocess.run([str(emu), f"{tmp_path}/hand.bam", "10"], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    s = sample_summary(out.stdout)
    assert s["records"] == len(recs) and s["mq"] == 10
    # f_xa, f_ih, f_mapq0, f_dup, the two unmapped records and the one without a reference feed nothing into Reads; f_lowmapq is the middle
    # class; split1 is named
    assert s["reads"] == s["records"] - 7 and s["below_mq"] == 1 and s["named"] >= 2 and 0 < s["p3"] < s["reads"] - s["left"]


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


LONG_SEED = "20261017"  # (tests/test_bwa_stage_gpu.py runs the same tables on the device)
LONG_LENGTHS = [65535, 65536, 65537, 131072, 131073, 131072, 65537, 65537]
LONG_FALLBACK = 7  # the table whose chromosomes go down along Reads (the kernels raise the flag, the library takes the host loop)
LONG_LINE = (r"(\d+) long cases, (\d+) blocks, held (\d+), counted (\d+), random tiling (\d+), short nodes under dense blocks (\d+), far block holds two tiles of the next round (\d+), "
             r"block beyond the last node in front of a later round (\d+) \(inside the second round (\d+)\), chromosome going down at the first block of a round (\d+)")
LONG_KEYS = ("cases", "blocks", "held", "counted", "random_tiling", "dense", "far_round", "dead_round", "dead_second", "down_round")


def long_summary(text):
    """(the summary, [(nodes, blocks, held, counted, fallback) per table])"""
    m = re.search(LONG_LINE, text)
    assert m, text[-2000:]
    per_case = [tuple(int(x) for x in c) for c in re.findall(r"long case \d+: (\d+) nodes, (\d+) blocks, held (\d+), counted (\d+), fallback (\d)", text)]
    return dict(zip(LONG_KEYS, (int(x) for x in m.groups()))), per_case


def read_long_cases(path):
    """_read_cases for tables of 100 000 rows: [(nodes, reads)] as int32 arrays of shape (n, 3)"""
    import numpy as np

    toks = path.read_text().split()
    at, cases = 0, []
    while at < len(toks):
        assert toks[at] == "case"
        nn, nr = int(toks[at + 1]), int(toks[at + 2])
        v = np.array(toks[at + 3:at + 3 + 3 * (nn + nr)], dtype=np.int64).astype(np.int32).reshape(-1, 3)
        at += 3 + 3 * (nn + nr)
        cases.append((v[:nn], v[nn:]))
    return cases


def check_long_summary(s, per_case):
    assert [c[1] for c in per_case] == LONG_LENGTHS and s["cases"] == len(LONG_LENGTHS) and s["blocks"] == sum(LONG_LENGTHS)
    assert s["random_tiling"] >= 2 and s["dense"] >= 2
    assert s["far_round"] >= 1 and s["dead_round"] >= 2 and s["dead_second"] >= 1 and s["down_round"] >= 1
    assert [k for k, c in enumerate(per_case) if c[4]] == [LONG_FALLBACK]
    for nodes, blocks, held, counted, fallback in per_case:  # (no table is all held or all counted)
        assert nodes > 1000 and (fallback or (held > blocks // 10 and counted > 1000)), per_case


def test_emulated_depth_kernels_on_long_tables(emu, tmp_path):
    """depth_prefix walks the tiles in rounds of 64 and carries its two maxima from round to round; the tables of --fuzz end at five tiles.
    tools/bwa_stage_emu.cpp --fuzz-long: lists of 65 535, 65 536, 65 537, 131 072 and 131 073 blocks, random tiling and short nodes under dense
    blocks, a far block as the last block of the first round that holds two tiles of the second, a block beyond the last node in the last
    tile of the first round and one inside the second round of a list that reaches the third (what only the carry brings across) -- no
    difference in any Support or sum or in the held count; a block of the first chromosome alone in the second round behind a round of later
    chromosomes raises the fallback flag; and the literal loop of the reference against route 0 on the same tables"""
    out = subprocess.run([str(emu), "--fuzz-long", LONG_SEED, "--write", str(tmp_path / "long.txt")], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (out.stdout[-3000:], out.stderr[-2000:])
    s, per_case = long_summary(out.stdout)
    check_long_summary(s, per_case)
    cases = read_long_cases(tmp_path / "long.txt")
    assert [len(r) for _, r in cases] == LONG_LENGTHS
    for k, (nodes, reads) in enumerate(cases):
        r = squid_amd.debug_bwa_depth(nodes, reads, route=0)
        assert (r["support"], r["sums"]) == _literal_depth_loop(nodes.tolist(), reads.tolist()), k
        assert k == LONG_FALLBACK or sum(r["support"]) == per_case[k][3], k


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
