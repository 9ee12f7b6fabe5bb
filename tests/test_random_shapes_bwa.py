"""Random input SHAPES for `squid --bwa`, against the oracle on both routes.  The other --bwa tests read files of one shape (the generator's
defaults in the shape `bwa mem` writes: 2 x 100 bases, inserts N(300, 30), proper pairs, clips of 16-30 bases, MAPQ 0 or 60);
shapes.draw_bwa turns a seed into the generator arguments of the STAR cases plus --bwa and, in about half the cases, MAPQ values spread over
a range that -mq cuts (--bwa-mapq), the oracle flags and the Context parameters.  What that varies is what the newest kernels branch on: the
class byte of every record (mate unmapped / on another chromosome / at the same position, duplicates, XA, MAPQ against -mq), the blocks the
one-way depth cursor holds (read length, blocks per record, overlapping mates, node density), and a Reads list beyond one round of
depth_prefix.

CPU part: every seed of the list is usable and the list covers what it is there for; the knob changes something the oracle computes; the
kernel source emulated (tools/bwa_stage_emu.cpp) against the host loops on every seed, each with its own -mq; the stretched host loops on
six seeds.
GPU part: one case per seed -- the device route against the oracle stage by stage, then the host route and the device route again on the
same context, no fallback, the two readers taking turns -- and four seeds with the host loops in stretches."""
import os
import subprocess

import pytest

import shapes
from test_bwa import _build_pieces_check
from test_bwa_stage_emu import emu, sample_summary  # noqa: F401 -- (emu: the module fixture that builds the harness)
from test_random_shapes import _named

# one block more than a round of depth_prefix (64 tiles of 1024 blocks)
ROUND_BLOCKS = 65536
# six seeds for the stretched loops on the CPU: 250-base reads, one-base clips, the longest Reads list, five contigs, odd pairs at 13 %, 50-base reads
PIECE_SEEDS = (2, 3, 6, 9, 12, 14)
# four for the stretched loops on the device side: at least 29 stretches of 1000 records each (tools/bwa_pieces_check.cpp prints the counters);
# 3 and 6 start stretches on a wrong guess and run them again, 6 and 12 have the middle MAPQ class, 16 has MAPQ 0 / 60
STRETCH_SEEDS = (3, 6, 12, 16)
# fixed case of test_mapq_knob_reaches_the_graph
KNOB_SEED, KNOB_MQ, KNOB_RANGE = shapes.KNOB_SEED, "30", "5,55"


def _fragments(dump):
    return sum(1 for line in (dump / "chimrecord.txt").read_text().splitlines() if not line.startswith("#"))


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def bwa_run(built, tmp_path_factory):
    """(gen_args, oracle flags) -> (generator status, counts, oracle status, sv path, dump dir, file prefix), once per module"""
    cache = {}

    def run(gen, flags):
        key = (tuple(gen), tuple(flags))
        if key not in cache:
            d = tmp_path_factory.mktemp("bwa_shape")
            rc, counts = shapes.generate(built, d / "s", gen)
            orc, sv_path, dump = (None, None, None) if rc else shapes.run_oracle_bwa(built, d / "s", d, flags)
            cache[key] = (rc, counts, orc, sv_path, dump, d / "s")
        return cache[key]

    return run


def _strictly_inside(gen, params):
    rng = shapes.mapq_range(gen)
    return rng is not None and rng[0] < params["min_mapqual"] < rng[1]


def test_every_bwa_seed_is_usable(built, bwa_run):
    """the inputs of the GPU cases are good: generator and oracle run through, no ordering problem is ambiguous, there is a call and a rebuilt
    fragment -- and the list covers short and long reads, every planted kind, the MAPQ knob, and a -mq inside the MAPQ range (three classes of
    records).  No GPU case may skip, so this test is where a bad seed shows."""
    seeds = shapes.BWA_SEEDS
    assert len(seeds) == len(set(seeds)) == 16
    assert set(PIECE_SEEDS) <= set(seeds) and len(set(PIECE_SEEDS)) == 6 and set(STRETCH_SEEDS) <= set(seeds) and len(set(STRETCH_SEEDS)) == 4
    assert shapes.draw(seeds[0]) == shapes.draw(seeds[0]) and shapes.draw_bwa(seeds[0]) == shapes.draw_bwa(seeds[0])
    all_counts = {}
    for seed in seeds:
        gen, flags, params = shapes.draw_bwa(seed)
        assert "--config" not in gen and "--bwa" in gen and int(gen[gen.index("--records") + 1]) <= 40000
        assert params["star_mapq"] is False and params["min_mapqual"] == (int(flags[flags.index("-mq") + 1]) if "-mq" in flags else 1)
        rng = shapes.mapq_range(gen)
        assert rng is None or (1 <= rng[0] <= 20 and 40 <= rng[1] <= 60 and params["min_mapqual"] <= rng[1])
        rc, counts, orc, sv_path, dump, pre = bwa_run(gen, flags)
        where = f"seed {seed}\n" + shapes.commands(built, "s", gen, flags)
        assert rc == 0 and orc == 0, where
        assert shapes.usable(sv_path, dump), where
        assert _fragments(dump) >= 1, where
        assert counts["read_len"] == shapes.read_len(gen)
        assert ("bwa_mapq_below_30" in counts) == (rng is not None), where
        if rng is not None and rng[0] < 30:
            assert counts["bwa_mapq_below_30"] > 0, where
        all_counts[seed] = counts
    lens = [c["read_len"] for c in all_counts.values()]
    assert min(lens) <= 75 and max(lens) >= 150
    for kind in ("short_clips", "overlapping_mates", "polya_reads", "multi", "dup"):
        assert sum(1 for c in all_counts.values() if c[kind] > 0) >= 3, kind
    for kind in shapes.ODD_KINDS:
        assert sum(1 for c in all_counts.values() if c[kind] > 0) >= 2, kind
    assert sum(1 for s in seeds if shapes.mapq_range(shapes.draw_bwa(s)[0])) >= 6
    assert sum(1 for s in seeds if _strictly_inside(shapes.draw_bwa(s)[0], shapes.draw_bwa(s)[2])) >= 4


def test_mapq_knob_needs_bwa_and_a_range(built, tmp_path):
    for args in (("--bwa-mapq", "5,55"), ("--bwa", "--bwa-mapq", "5,61"), ("--bwa", "--bwa-mapq", "30,20"), ("--bwa", "--bwa-mapq", "-1,20")):
        assert shapes.generate(built, tmp_path / "s", args)[0] == 2, args


def test_mapq_knob_reaches_the_graph(built, bwa_run):
    """a knob that changes nothing the oracle computes tests nothing: with -mq 30, MAPQ spread over 5..55 instead of 60 changes the build-stage
    nodes or the breakpoint table"""
    base = ("--seed", str(KNOB_SEED), "--bwa")
    rc0, counts0, orc0, _, dump0, _ = bwa_run(base, ("-mq", KNOB_MQ))
    rc1, counts1, orc1, _, dump1, _ = bwa_run(base + ("--bwa-mapq", KNOB_RANGE), ("-mq", KNOB_MQ))
    assert (rc0, orc0, rc1, orc1) == (0, 0, 0, 0)
    assert "bwa_mapq_below_30" not in counts0 and 0 < counts1["bwa_mapq_below_30"] < counts1["concordant_records"]
    assert any((dump0 / f).read_bytes() != (dump1 / f).read_bytes() for f in ("nodes_build.txt", "breakpoints.txt")), counts1


def test_emulated_stages_on_every_bwa_seed(built, emu, bwa_run):  # noqa: F811
    """the kernel source on the CPU (class byte lane by lane, depth kernels as waves of 64 coroutines) against the library's host loops on every
    seed's file, at the seed's own -mq: no difference; both filters drop something, the name test has something to decide, the cursor holds
    blocks; one list is longer than a round of depth_prefix.  Where -mq lies above the lowest MAPQ of a --bwa-mapq file the middle class is there: the
    harness's count `READS records below -mq` (records that feed Reads and are not looked at by the breakpoint support) is positive, and the
    breakpoint-support records are fewer than the READS records that are not the left-hand record of a pair"""
    longest, middle = 0, 0
    for seed in shapes.BWA_SEEDS:
        gen, flags, params = shapes.draw_bwa(seed)
        pre = bwa_run(gen, flags)[5]
        where = f"seed {seed}\n" + shapes.commands(built, "s", gen, flags)
        out = subprocess.run([str(emu), f"{pre}.bam", str(params["min_mapqual"])], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0 and out.stdout.strip().endswith("0 differences: same"), (where, out.stdout[-3000:], out.stderr[-2000:])
        s = sample_summary(out.stdout)
        print(seed, s)
        assert s["mq"] == params["min_mapqual"]
        assert 0 < s["p3"] < s["reads"] < s["records"], (where, s)
        assert s["named"] > 0 and s["held"] > 0, (where, s)
        rng = shapes.mapq_range(gen)
        if rng is not None and params["min_mapqual"] > rng[0]:
            assert s["below_mq"] > 0, (where, s)
            assert 0 < s["p3"] < s["reads"] - s["left"], (where, s)
        else:
            # (MAPQ 0 never feeds Reads, and MAPQ 60 or a whole range at or above -mq passes it.  The inequality is not asked here: a record whose
            # blocks are all poly-A has none left and feeds nothing into Reads, but the breakpoint support still looks at it)
            assert s["below_mq"] == 0, (where, s)
        middle += s["below_mq"] > 0
        longest = max(longest, s["reads_blocks"])
    assert longest > ROUND_BLOCKS
    assert middle >= 4


@pytest.mark.parametrize("seed", PIECE_SEEDS)
def test_stretched_loops_on_bwa_seeds(built, bwa_run, tmp_path_factory, seed):
    """host only (tools/bwa_pieces_check.cpp): the record loops cut into stretches of 37 and of 300 records give the nodes with their Support /
    AvgDepth, the raw edges and the rebuilt fragments of the loops run in one go"""
    exe = _build_pieces_check(built, tmp_path_factory)
    gen, flags, _ = shapes.draw_bwa(seed)
    pre = bwa_run(gen, flags)[5]
    for piece in ("37", "300"):
        out = subprocess.run([str(exe), f"{pre}.bam", piece, "5"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().endswith("same"), (seed, piece, " ".join(gen), out.stdout[-2000:])


# ---------------------------------------------------------------------------------------------------------------- GPU
def _case(built, synth, tmp_path, seed):
    gen, flags, params = shapes.draw_bwa(seed)
    pre = synth("T2", *gen)
    where = f"seed {seed}, SQUID_BWA_GPU={os.environ.get('SQUID_BWA_GPU')}, SQUID_BWA_PIECE={os.environ.get('SQUID_BWA_PIECE')}\n" + shapes.commands(built, pre, gen, flags)
    orc, sv_path, dump = shapes.run_oracle_bwa(built, pre, tmp_path, flags)
    assert orc == 0 and shapes.usable(sv_path, dump), where
    return pre, params, sv_path, dump, where


@pytest.mark.gpu
@pytest.mark.parametrize("seed", shapes.BWA_SEEDS)
def test_random_bwa_shape_against_the_oracle(built, synth, tmp_path, monkeypatch, seed):
    """device route: every stage snapshot, the orders, the breakpoints and _sv.txt equal the oracle's, without a fallback to the host loops (a sorted
    BAM never sends the chromosomes down along Reads, and no shape makes a record of 256 blocks); then the host route and the device route again
    on the same context: same text, stage-1 nodes, breakpoint table and record counts; the rebuilt fragments are the oracle's"""
    import squid_amd
    from test_bwa_stage_gpu import _both_routes, _launches

    # the readers take turns: odd positions through the device reader (what a --bwa file of 1 GiB and more gets), even positions the host decoder
    through_gpu = shapes.BWA_SEEDS.index(seed) % 2
    monkeypatch.setenv("SQUID_BWA_GPU", str(through_gpu))
    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    monkeypatch.delenv("SQUID_BWA_PIECE", raising=False)
    pre, params, sv_path, dump, where = _case(built, synth, tmp_path, seed)
    with squid_amd.Context(**params) as ctx:
        ctx.load_bwa(f"{pre}.bam")
        with _named(where, "reader"):
            assert ctx.counts()["chimeric_through_gpu_reader"] == through_gpu
        with _named(where, "device route, then host route and device route again"):
            sv, t = _both_routes(ctx, dump, sv_path)
            assert sv.count("\n") > 1
            assert _launches(t, "bwa_device_fallback") == 0 and _launches(t, "bwa_depth_held_blocks") > 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", STRETCH_SEEDS)
def test_random_bwa_shape_with_stretched_host_loops(built, synth, tmp_path, monkeypatch, seed):
    """SQUID_BWA_PIECE (read per call) at 97 and at 1000 records: every stage, the rebuilt fragments and _sv.txt equal the oracle's, and both loops
    really ran in stretches"""
    import squid_amd
    from test_gpu_parity import _compare

    monkeypatch.delenv("SQUID_BWA_STAGES_GPU", raising=False)
    monkeypatch.delenv("SQUID_BWA_GPU", raising=False)
    for piece in ("97", "1000"):
        monkeypatch.setenv("SQUID_BWA_PIECE", piece)
        pre, params, sv_path, dump, where = _case(built, synth, tmp_path / piece, seed)
        with squid_amd.Context(**params) as ctx:
            ctx.load_bwa(f"{pre}.bam")
            ctx.build_graph()
            with _named(where, f"stretches of {piece} records"):
                sv = _compare(ctx, dump, sv_path)
                assert sv.count("\n") > 1
                assert ctx.counts()["n_chim_fragments"] == _fragments(dump)
                t = ctx.timing()
                stretches = (t.get("bwa_raw_edge_stretches", {}).get("launches", 0), t.get("bwa_seed_node_stretches", {}).get("launches", 0))
                assert stretches[0] > 3 and stretches[1] > 3, stretches
                assert "bwa_bp_support_stretches_walked_again" in t
