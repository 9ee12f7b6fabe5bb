"""One place that turns a seed into a test case for the random-shape tests (tests/test_random_shapes.py and the shape cases of the
literal-loop tests): generator arguments that vary what the generator's defaults keep fixed (read length, insert size, clip lengths on
both sides of the 15-base threshold, pair flags, poly-A blocks, filter rates, contig lists), oracle flags, and the matching
squid_amd.Context keyword arguments.  draw_bwa does the same for `squid --bwa` (tests/test_random_shapes_bwa.py).

A plain module, not a conftest: nothing here changes how the suite runs."""
import gzip
import hashlib
import json
import math
import random
import subprocess
from pathlib import Path

READ_LENS = (50, 75, 100, 125, 150, 200, 250)
FRACTION_KNOBS = ("--clip-frac", "--multi-frac", "--dup-frac", "--lowq-frac", "--pcrcopy-frac", "--polya-frac", "--odd-pair-frac")
ODD_KINDS = ("odd_unproper", "odd_same_strand", "odd_near_gene", "odd_far", "odd_other_chr", "odd_mate_unmapped", "odd_same_pos")
PLANTED_COUNTS = ("short_clips", "long_clips", "polya_reads", "overlapping_mates") + ODD_KINDS + ("multi", "dup", "lowq", "pcrcopy")


def _fraction(r):
    """log-uniform in [0.002, 0.2]"""
    return round(math.exp(r.uniform(math.log(0.002), math.log(0.2))), 4)


def draw(seed):
    """seed -> (gen_args, oracle_flags, context_params); config T2, at most 40 000 records"""
    r = random.Random(seed)
    n = r.choice(READ_LENS)
    mean = round(r.uniform(1.2 * n, 4.0 * n))
    lo = r.randint(2, 10)
    gen = ["--seed", str(seed), "--records", str(r.randint(6000, 40000)), "--read-len", str(n), "--insert", f"{mean},{r.randint(10, 80)}",
           "--support", f"{lo},{lo + r.randint(4, 40)}"]
    for knob in FRACTION_KNOBS:
        if r.random() < 0.65:
            gen += [knob, str(_fraction(r))]
    # about half the cases include clips of 15 bases or fewer (the `part` threshold of k_pass1w and whetherbuildedge of RawEdgesOther)
    kind = r.random()
    if kind < 0.5:
        a = r.randint(1, 15)
        gen += ["--clip-len", f"{a},{r.randint(max(a, 14), 30)}"]
    elif kind < 0.8:
        a = r.randint(16, 20)
        gen += ["--clip-len", f"{a},{r.randint(a, 40)}"]
    if r.random() < 0.4:
        a = r.randint(20, 40)
        gen += ["--split-anchor", f"{a},{r.randint(a, 80)}"]
    if r.random() < 0.3:
        gen += ["--interleave", str(r.randint(1, 3))]
    if r.random() < 0.3:
        gen += ["--indel-frac", str(round(r.uniform(0.05, 0.3), 3))]
    if r.random() < 0.4:
        # three to six contigs, one or two of them too short to receive a gene, long ones first or last or in between
        lens = [r.randint(900000, 3000000) for _ in range(r.randint(2, 4))] + [r.randint(20000, 80000) for _ in range(r.randint(1, 2))]
        r.shuffle(lens)
        gen += ["--contigs", ",".join(str(x) for x in lens)]
    flags, params = _draw_flags(r, lambda: r.randint(1, 4))
    return tuple(gen), flags, params


def _draw_flags(r, mapqual, p_mapqual=0.3):
    """(oracle flags, Context keywords), each flag with probability 0.3 (-mq: p_mapqual)"""
    flags, params = [], {}
    # (flag, keyword, draw): between the reference's default and the value PARAM_SETS of tests/test_gpu_parity.py uses
    for flag, kw, val in (("-w", "min_edge_weight", lambda: r.randint(1, 5)), ("-r", "discordant_ratio", lambda: r.choice([1.5, 2.0, 4.0, 8.0])),
                          ("-a", "max_allowed_degree", lambda: r.choice([5, 10, 50])), ("-dp", "concord_dist_pos", lambda: r.choice([2000, 10000, 50000])),
                          ("-di", "concord_dist_idx", lambda: r.choice([3, 10, 20])), ("-mq", "min_mapqual", mapqual),
                          ("-pl", "max_lowphred_len", lambda: r.choice([5, 10])), ("-pm", "min_phred", lambda: r.choice([4, 10]))):
        if r.random() < (p_mapqual if flag == "-mq" else 0.3):
            v = val()
            flags += [flag, str(v)]
            params[kw] = v
    return tuple(flags), params


BWA_MQ = (1, 10, 30, 45, 60)


def draw_bwa(seed):
    """seed -> (gen_args, oracle_flags, context_params) for `--bwa`: the generator arguments of draw(seed) in the shape `bwa mem` writes, in about
    half the cases with MAPQ spread over [LO, HI] (LO 1-20, HI 40-60) instead of 60; the flags from a stream of their own (draw() and its 24
    cases stay what they are), -mq from BWA_MQ so that it cuts inside that range -- with the spread twice as often as the other flags, since
    that is where it separates three classes of records, and never above HI, where no record would be left for the breakpoint support; the
    keywords as every --bwa test passes them"""
    gen = list(draw(seed)[0])
    r = random.Random(f"bwa {seed}")
    gen += ["--bwa"]
    hi = None
    if r.random() < 0.5:
        hi = r.randint(40, 60)
        gen += ["--bwa-mapq", f"{r.randint(1, 20)},{hi}"]
    flags, params = _draw_flags(r, lambda: r.choice([q for q in BWA_MQ if hi is None or q <= hi]), 0.6 if hi else 0.3)
    params.setdefault("min_mapqual", 1)
    params["star_mapq"] = False
    return tuple(gen), flags, params


def mapq_range(gen_args):
    """(LO, HI) of --bwa-mapq, or None"""
    if "--bwa-mapq" not in gen_args:
        return None
    lo, hi = gen_args[gen_args.index("--bwa-mapq") + 1].split(",")
    return int(lo), int(hi)


def insert_mean(gen_args):
    return float(gen_args[gen_args.index("--insert") + 1].split(",")[0])


def read_len(gen_args):
    return int(gen_args[gen_args.index("--read-len") + 1])


def generate(build_dir, prefix, gen_args, config="T2"):
    """run the generator; returns (exit status, the counts of its JSON line or None)"""
    p = subprocess.run([str(Path(build_dir) / "gen_synth_bam"), "--config", config, "--out", str(prefix), *gen_args], capture_output=True, text=True)
    return p.returncode, (json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else None)


def commands(build_dir, prefix, gen_args, flags, config="T2"):
    """the two command lines that rebuild a case on the CPU (for assertion messages); the `--bwa` form when the generator gets --bwa"""
    b = Path(build_dir)
    files = ["--bwa", "-b", f"{prefix}.bam"] if "--bwa" in gen_args else ["-b", f"{prefix}.bam", "-c", f"{prefix}.chim.bam"]
    return (" ".join([str(b / "gen_synth_bam"), "--config", config, "--out", str(prefix), *gen_args]) + "\n" +
            " ".join([str(b / "squid_oracle"), *files, "-o", "oracle", "--dump", "dump", *flags]))


def run_oracle_bwa(build_dir, prefix, outdir, flags):
    """squid_oracle --bwa with stage dumps -> (exit status, sv path, dump dir)"""
    outdir = Path(outdir)
    dump = outdir / "dump"
    dump.mkdir(parents=True, exist_ok=True)
    rc = subprocess.call([str(Path(build_dir) / "squid_oracle"), "--bwa", "-b", f"{prefix}.bam", "-o", str(outdir / "oracle"), "--dump", str(dump), *flags],
                         stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return rc, outdir / "oracle_sv.txt", dump


def usable(sv_path, dump):
    """the oracle ran through, no ordering problem of the input is ambiguous, and there is at least one call"""
    if not sv_path.exists() or not (dump / "order_stats.txt").exists():
        return False
    stats = dict(line.split("\t") for line in (dump / "order_stats.txt").read_text().splitlines())
    return stats["ambiguous"] == "0" and sv_path.read_text().count("\n") > 1


# ---- the 24 cases of the random-shape tests.  Found on the CPU by running generator and oracle over the candidate seeds 1..N in order
# (tests/golden/make_shape_seeds.py): a seed is kept when the generator exits 0, the oracle exits 0 (4 = a reference assert), no
# ordering problem is ambiguous and _sv.txt has a call.  test_every_seed_is_usable repeats the conditions.
SEEDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24]

# ---- the 16 cases of tests/test_random_shapes_bwa.py, found the same way (make_shape_seeds.py --bwa: draw_bwa and squid_oracle --bwa, and at
# least one rebuilt fragment); test_every_bwa_seed_is_usable repeats the conditions.  Seed 6 has more than 65 536 blocks in Reads.
BWA_SEEDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]

# six of them for the literal-loop readings: together they hold odd pairs, short clips, overlapping mates, poly-A blocks and read
# lengths other than 100
LITERAL_SEEDS = [2, 7, 8, 10, 15, 19]

# (config, gen_args, oracle flags) as the literal-loop tests parametrise: the oracle's default flags, which is what the literal loops restate
LITERAL_CASES = [("T2", draw(s)[0], ()) for s in LITERAL_SEEDS]
LITERAL_IDS = [f"shape{s}" for s in LITERAL_SEEDS]

# one fixed case per knob: (name, seed, gen_args with only that knob set); the oracle's build-stage graph must differ from the same seed's
# run without the knob (test_each_knob_reaches_the_graph)
KNOB_SEED = 7
KNOB_CASES = [
    ("read-len", KNOB_SEED, ("--read-len", "75")),
    ("insert", KNOB_SEED, ("--insert", "150,30")),
    ("clip-frac", KNOB_SEED, ("--clip-frac", "0.3")),
    ("clip-len", KNOB_SEED, ("--clip-len", "1,15")),
    ("multi-frac", KNOB_SEED, ("--multi-frac", "0.2")),
    ("dup-frac", KNOB_SEED, ("--dup-frac", "0.2")),
    ("lowq-frac", KNOB_SEED, ("--lowq-frac", "0.2")),
    ("pcrcopy-frac", KNOB_SEED, ("--pcrcopy-frac", "0.2")),
    ("polya-frac", KNOB_SEED, ("--polya-frac", "0.2")),
    ("odd-pair-frac", KNOB_SEED, ("--odd-pair-frac", "0.1")),
    ("split-anchor", KNOB_SEED, ("--split-anchor", "20,24")),
    ("contigs", KNOB_SEED, ("--contigs", "1500000,40000,2500000,1000000")),
]
KNOB_ORACLE_FLAGS = {}  # knob name -> oracle flags its case needs (none does)


# ---- the pin of the generator's defaults
PIN_SAMPLES = [
    ("C1", ()),
    ("T2", ()),
    ("T2", ("--indel-frac", "0.2")),
    ("T2", ("--interleave", "3")),
    ("T2", ("--bwa",)),
    ("C2", ("--support", "2,6")),
    ("C5", ("--records", "300000", "--tsv", "1500")),
]


def pin_key(config, extra):
    return " ".join((config,) + tuple(extra))


def file_digests(prefix):
    """sha256 of the INFLATED content of .bam / .chim.bam (the compressed bytes depend on the zlib build) and of .bam.bai / .truth.txt"""
    out = {}
    for suffix, inflate in ((".bam", True), (".chim.bam", True), (".bam.bai", False), (".truth.txt", False)):
        p = Path(f"{prefix}{suffix}")
        if p.exists():
            data = p.read_bytes()
            out[suffix] = hashlib.sha256(gzip.decompress(data) if inflate else data).hexdigest()
    return out
