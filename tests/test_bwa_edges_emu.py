"""RawEdges' record loop of the `--bwa` device route (squid_amd/csrc/sq_bwa_edges.inc -- what sq_bwa_edges_on_device switches on: a fragment
table made from the records, the position chain of the chimeric device stages over it, one lane per record for the edges, the three lists of
the loop compacted in record order) on the CPU: the kernel source itself (sq_wave.h with SQ_WAVE_EMU, tools/bwa_edges_emu.cpp) against the
library's host loop in one go on the same batch and the same nodes -- the summed edges, the three lists in order, the would-be edges of the
multi-aligned second mates, the position behind the last record, the number of emitted edges.  What the restatement is about is the position
LocateRead carries from record to record: the harness counts the records whose first block had to be resolved in record order (soft
fragments) and the runs of them, and a sample without either would prove nothing.  The GPU suite runs the same source on the device
(tests/test_bwa_edges_gpu.py)."""
import re
import struct
import subprocess

import pytest

import bamwriter as bw
import shapes
from test_bwa_stage_gpu import A, B_, FIRST, MATE_REV, MATE_UNMAPPED, PAIRED, REV, SECOND, handmade_records


@pytest.fixture(scope="module")
def edges_emu(built, tmp_path_factory):
    exe = tmp_path_factory.mktemp("bwa_edges_emu") / "bwa_edges_emu"
    root = built.parent
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-DSQ_WAVE_EMU", "-I", str(root / "include"), "-o", str(exe), str(root / "tools" / "bwa_edges_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    return exe


SAMPLE_LINE = (r"(\d+) records, (\d+) nodes, kind-1 (\d+), kind-2 (\d+), soft fragments (\d+), soft runs longer than one (\d+) \(longest (\d+)\), partial (\d+), first_dis (\d+), second (\d+), "
               r"-1 edges added (\d+), records of 3 and more blocks (\d+), emitted edges (\d+), final position (-?\d+), (\d+) differences")
SAMPLE_KEYS = ("records", "nodes", "kind1", "kind2", "soft", "soft_runs", "longest_run", "partial", "first_dis", "second", "added", "big", "emitted", "final_pos", "differences")


def sample_summary(text):
    m = re.search(SAMPLE_LINE, text)
    assert m, text[-2000:]
    return dict(zip(SAMPLE_KEYS, (int(x) for x in m.groups())))


FUZZ = ("60", "20261018")  # cases, seed (tests/test_bwa_edges_gpu.py runs the same tables on the device)
FUZZ_LINE = (r"(\d+) cases, (\d+) records, (\d+) block slots, kind-1 (\d+), kind-2 (\d+), soft fragments (\d+), soft runs longer than one (\d+) \(longest (\d+)\), partial (\d+), first_dis (\d+), "
             r"second (\d+), emitted edges (\d+), assert cases (\d+) \(planted (\d+)\), empty tables (\d+), tables on nodes of 1-4 bases (\d+), first blocks at a node edge (\d+), "
             r"records of 3 and more blocks (\d+), mates on another chromosome (\d+), unmapped mates (\d+), mates without a reference (\d+), (\d+) differences")
FUZZ_KEYS = ("cases", "records", "blocks", "kind1", "kind2", "soft", "soft_runs", "longest_run", "partial", "first_dis", "second", "emitted", "asserts", "planted", "empty", "tiny", "edge_near", "big",
             "other_chr", "mate_unmapped", "mate_none", "differences")


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
def test_emulated_loop_equals_the_host_loop_on_the_samples(edges_emu, synth, cfg, gen):
    pre = synth(cfg, "--bwa", *gen)
    s = sample_summary(run_emu(edges_emu, f"{pre}.bam"))
    assert s["differences"] == 0
    assert s["kind1"] > 0 and s["soft"] > 0 and s["soft_runs"] > 0 and s["partial"] > 0 and s["first_dis"] > 0, s
    assert s["emitted"] > s["first_dis"]
    # (the generator writes no multi-aligned second mate whose would-be edge is discordant: the hand-made BAM below has them)
    if s["second"]:
        assert s["kind2"] >= s["second"]


# ---- the hand-made BAM of tests/test_bwa_stage_gpu.py plus what the generator may lack
XA = b"NHC\x01XAZchrB,+100,60M,0;\x00"


def handmade_edge_records():
    """handmade_records() plus: `sec_a` -- a first mate inside the discordant cluster A:3000 <-> B:2000 (it adds a discordant pair edge) whose
    second mate is multi-aligned (XA, MAPQ 0): listed, and its -1 edge is really added; `sec_b` -- the same with a first mate of MAPQ 0, which the
    loop skips: the second mate is listed, nothing is added; `rev3` -- a reverse-strand first mate of three blocks (read offsets run against the
    CIGAR) over the cluster's node boundaries; `clip16` / `clip15` -- first mates whose first block starts at read offset 16 (locates nothing,
    goes to PartialAlign) and 15 (located)"""
    extra = [
        bw.record("sec_a", A, 3003, 60, PAIRED | MATE_REV | FIRST, "60M", B_, 2003),
        bw.record("sec_a", B_, 2003, 0, PAIRED | REV | SECOND, "60M", A, 3003, tags=XA),
        bw.record("sec_b", A, 3004, 0, PAIRED | MATE_REV | FIRST, "60M", B_, 2004),
        bw.record("sec_b", B_, 2004, 0, PAIRED | REV | SECOND, "60M", A, 3004, tags=XA),
        bw.record("rev3", A, 2960, 60, PAIRED | MATE_UNMAPPED | REV | FIRST, "20M30N20M3000N20M", -1, -1),
        bw.record("clip16", A, 2980, 60, PAIRED | MATE_UNMAPPED | FIRST, "16S44M", -1, -1),
        bw.record("clip15", A, 2981, 60, PAIRED | MATE_UNMAPPED | FIRST, "15S45M", -1, -1),
    ]
    return sorted(handmade_records() + extra, key=lambda r: (struct.unpack_from("<i", r, 4)[0] & 0x7fffffff, struct.unpack_from("<i", r, 8)[0]))  # (stable: equal places keep their order)


def write_handmade_edges(path):
    bw.write_bam(str(path), [("chrA", 20000), ("chrB", 10000)], handmade_edge_records())


def test_emulated_loop_on_the_hand_made_bam(edges_emu, tmp_path):
    """the counts are the HOST loop's (the harness prints a list only when both routes agree on it): two listed second mates of which one adds its
    -1 edge, a record of three blocks, the partial reads of the base file plus `clip16`"""
    write_handmade_edges(tmp_path / "hand.bam")
    s = sample_summary(run_emu(edges_emu, tmp_path / "hand.bam", 10))
    assert s["differences"] == 0
    assert s["second"] == 2 and s["added"] == 1 and s["kind2"] >= 2, s
    assert s["big"] == 1 and s["first_dis"] >= 8, s          # (tra0..6 and sec_a)
    assert s["partial"] >= 3 and s["kind1"] > 20, s          # (split1, zz_last, clip16 at least)
    # without `clip16` one partial read fewer and the same located first mates; without `clip15` one located first mate fewer
    base = [r for r in handmade_edge_records() if b"clip1" not in r]
    for drop, dk1, dpart in ((b"clip16", 0, 1), (b"clip15", 1, 0)):
        recs = [r for r in handmade_edge_records() if drop not in r]
        assert len(recs) == len(base) + 1
        bw.write_bam(str(tmp_path / "less.bam"), [("chrA", 20000), ("chrB", 10000)], recs)
        t = sample_summary(run_emu(edges_emu, tmp_path / "less.bam", 10))
        assert (s["kind1"] - t["kind1"], s["partial"] - t["partial"]) == (dk1, dpart), (drop, s, t)


def test_emulated_loop_on_the_fuzz_tables(edges_emu):
    """random node tilings and record tables: nodes of 1-4 bases (most first blocks soft, long soft runs), first blocks within five bases of a node
    edge, records of 1, 2, 3, 17 and 256 blocks on both strands, mates on another chromosome / unmapped / without a reference, table sizes around one
    and two blocks of 256 lanes and one and two scan tiles, empty tables; a block behind the last node, in front of the first, or hanging over the
    end of the last node makes the loop assert (the device route then hands the graph back): counted, and at most a quarter of the cases"""
    s = fuzz_summary(run_emu(edges_emu, "--fuzz", *FUZZ))
    assert s["cases"] == 60 and s["differences"] == 0
    assert 1 <= s["asserts"] <= s["cases"] // 4 and s["asserts"] == s["planted"], s
    assert s["soft"] * 10 > s["kind1"] + s["kind2"] and s["soft_runs"] > 100 and s["longest_run"] > 64, s
    assert s["tiny"] >= 5 and s["empty"] >= 2 and s["edge_near"] > 1000 and s["big"] > 1000, s
    assert min(s["other_chr"], s["mate_unmapped"], s["mate_none"], s["partial"], s["first_dis"], s["second"], s["kind2"]) > 100, s


def test_emulated_loop_on_every_bwa_seed(built, edges_emu, tmp_path_factory):
    """the 16 random --bwa shapes, each at its own -mq"""
    soft = 0
    for seed in shapes.BWA_SEEDS:
        gen, flags, params = shapes.draw_bwa(seed)
        d = tmp_path_factory.mktemp("bwa_edge_shape")
        rc, _ = shapes.generate(built, d / "s", gen)
        assert rc == 0, (seed, gen)
        s = sample_summary(run_emu(edges_emu, d / "s.bam", params["min_mapqual"]))
        print(seed, s)
        assert s["differences"] == 0 and s["kind1"] > 0 and s["partial"] > 0, (seed, s)
        soft += s["soft"]
    assert soft > 0
