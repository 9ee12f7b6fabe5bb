"""Random input SHAPES against the oracle.  Every other parity test reads files of one shape (2 x 100 bases, inserts N(300, 30), proper
pairs, clips of 16-30 bases, no poly-A, half a percent of filtered records); tests/shapes.py turns a seed into generator arguments that vary
exactly those fields, the oracle flags and the Context parameters.

CPU part: the generator's defaults still write the files they always wrote (the benchmark's input among them), every seed of the list is
usable and the list as a whole covers what it is there for, and every knob changes something the oracle computes.
GPU part: one case per seed -- all stage snapshots, orders, breakpoints and _sv.txt against the oracle in the exact-depth mode and in the
production depth mode, the device route of the chimeric stages against the host route, the two readers taking turns -- and the five
staging sizes of the record parse on three read lengths."""
import json
import os
import subprocess
import sys
from contextlib import contextmanager
from pathlib import Path

import pytest

import oracle_util as ou
import shapes

GOLD = Path(__file__).resolve().parent / "golden"

# seeds whose device route of the chimeric stages hands a stage back to the host for a reason DESIGN.md documents: {seed: reason}; at most 2
FALLBACK_OK = {}
# three seeds of different read lengths for the staging sizes of k_parse_records
LDS_SEEDS = (14, 17, 2)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_default_files_are_unchanged(built, tmp_path):
    """without a shape knob the generator writes, byte for byte after inflation, what it wrote before the knobs existed"""
    want = json.loads((GOLD / "synth_default_sha256.json").read_text())
    assert sorted(want) == sorted(shapes.pin_key(c, e) for c, e in shapes.PIN_SAMPLES)
    for k, (config, extra) in enumerate(shapes.PIN_SAMPLES):
        pre = tmp_path / f"s{k}"
        subprocess.check_call([str(built / "gen_synth_bam"), "--config", config, "--out", str(pre), *extra], stdout=subprocess.DEVNULL)
        got = shapes.file_digests(pre)
        assert set(got) == ({".bam", ".bam.bai", ".truth.txt"} if "--bwa" in extra else {".bam", ".chim.bam", ".bam.bai", ".truth.txt"})
        assert got == want[shapes.pin_key(config, extra)], (config, extra)


@pytest.fixture(scope="module")
def shape_run(built, tmp_path_factory):
    """(gen_args, oracle flags) -> (generator status, counts, oracle status, sv path, dump dir), once per module"""
    cache = {}

    def run(gen, flags):
        key = (tuple(gen), tuple(flags))
        if key not in cache:
            d = tmp_path_factory.mktemp("shape")
            rc, counts = shapes.generate(built, d / "s", gen)
            orc, sv_path, dump = None, d / "oracle_sv.txt", d / "dump"
            if rc == 0:
                dump.mkdir()
                orc = subprocess.call([str(built / "squid_oracle"), "-b", f"{d / 's'}.bam", "-c", f"{d / 's'}.chim.bam", "-o", str(d / "oracle"), "--dump", str(dump), *flags],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            cache[key] = (rc, counts, orc, sv_path, dump)
        return cache[key]

    return run


def test_every_seed_is_usable(built, shape_run):
    """the inputs of the GPU cases are good: generator and oracle run through (the oracle ends with 4 where the reference would assert), no
    ordering problem is ambiguous, there is a call -- and the list covers every planted kind, both sides of the clip threshold, short and long
    reads and overlapping mates.  No GPU case may skip, so this test is where a bad seed shows."""
    assert len(shapes.SEEDS) == len(set(shapes.SEEDS)) == 24
    assert set(shapes.LITERAL_SEEDS) <= set(shapes.SEEDS) and len(shapes.LITERAL_SEEDS) == 6
    assert set(LDS_SEEDS) <= set(shapes.SEEDS) and len({shapes.read_len(shapes.draw(s)[0]) for s in LDS_SEEDS}) == 3
    assert len(FALLBACK_OK) <= 2 and set(FALLBACK_OK) <= set(shapes.SEEDS)
    assert set(SHARDED_SEEDS) <= set(shapes.SEEDS) and all("--contigs" in shapes.draw(s)[0] for s in SHARDED_SEEDS)
    all_counts = {}
    for seed in shapes.SEEDS:
        gen, flags, params = shapes.draw(seed)
        assert "--config" not in gen and int(gen[gen.index("--records") + 1]) <= 40000
        rc, counts, orc, sv_path, dump = shape_run(gen, flags)
        where = f"seed {seed}\n" + shapes.commands(built, "s", gen, flags)
        assert rc == 0 and orc == 0, where
        assert shapes.usable(sv_path, dump), where
        assert counts["read_len"] == shapes.read_len(gen)
        all_counts[seed] = counts
    for kind in shapes.PLANTED_COUNTS:
        assert sum(1 for c in all_counts.values() if c[kind] > 0) >= 3, kind
    lens = [c["read_len"] for c in all_counts.values()]
    assert min(lens) <= 75 and 100 in lens and max(lens) >= 150
    assert sum(1 for s in shapes.SEEDS if shapes.insert_mean(shapes.draw(s)[0]) < 2 * all_counts[s]["read_len"]) >= 3
    assert sum(1 for c in all_counts.values() if c["short_clips"] > 0) >= 4
    assert sum(1 for c in all_counts.values() if c["long_clips"] > 0) >= 4
    # the six cases of the literal-loop tests run at the oracle's default flags, and hold what they were chosen for
    lit = [shape_run(shapes.draw(s)[0], ()) for s in shapes.LITERAL_SEEDS]
    for s, (rc, counts, orc, sv_path, dump) in zip(shapes.LITERAL_SEEDS, lit):
        assert rc == 0 and orc == 0 and shapes.usable(sv_path, dump), s
    for kind in ("short_clips", "overlapping_mates", "polya_reads") + shapes.ODD_KINDS:
        assert any(c[kind] > 0 for _, c, _, _, _ in lit), kind
    assert any(c["read_len"] != 100 for _, c, _, _, _ in lit)


@pytest.mark.parametrize("name,seed,knob", shapes.KNOB_CASES, ids=[k[0] for k in shapes.KNOB_CASES])
def test_each_knob_reaches_the_graph(built, shape_run, name, seed, knob):
    """a knob that changes nothing the oracle computes tests nothing: with only that knob set, the build-stage nodes or edges differ from
    the same seed's run without it"""
    base = ("--seed", str(seed))
    flags = shapes.KNOB_ORACLE_FLAGS.get(name, ())
    rc0, _, orc0, _, dump0 = shape_run(base, flags)
    rc1, counts, orc1, _, dump1 = shape_run(base + tuple(knob), flags)
    assert (rc0, orc0, rc1, orc1) == (0, 0, 0, 0)
    assert any((dump0 / f).read_bytes() != (dump1 / f).read_bytes() for f in ("nodes_build.txt", "edges_build.txt")), (name, counts)


# ---------------------------------------------------------------------------------------------------------------- GPU
@contextmanager
def _named(where, what):
    """an assertion that fails inside carries the seed and the command lines that rebuild the case on the CPU"""
    try:
        yield
    except AssertionError as e:
        raise AssertionError(f"{what}: {where}\n{e}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("seed", shapes.SEEDS)
def test_random_shape_against_the_oracle(built, synth, tmp_path, monkeypatch, seed):
    import squid_amd
    from test_chim_stage_gpu import _route
    from test_gpu_parity import _compare

    gen, flags, params = shapes.draw(seed)
    # the readers take turns: even positions the suite's default (device reader), odd positions the host BGZF reader + dev_parse_append,
    # the production route of every file below 1 GiB
    if shapes.SEEDS.index(seed) % 2:
        monkeypatch.setenv("SQUID_GPU_INFLATE", "0")
    monkeypatch.delenv("SQUID_CHIM_STAGES_GPU", raising=False)
    pre = synth("T2", *gen)
    where = f"seed {seed}, SQUID_GPU_INFLATE={os.environ.get('SQUID_GPU_INFLATE')}\n" + shapes.commands(built, pre, gen, flags)
    sv_path, dump = ou.run_oracle(built, pre, tmp_path, *flags, check=False)
    assert shapes.usable(sv_path, dump), where
    monkeypatch.setenv("SQUID_EXACT_DEPTH", "1")
    with squid_amd.Context(**params) as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.build_graph()
        with _named(where, "exact depth, host route"):
            sv = _compare(ctx, dump, sv_path)
        bps = ctx.breakpoints()
        assert _route(ctx.timing()) == ("host", 0), where
        ctx.reset()
        ctx.chimeric_on_device()
        ctx.build_graph()
        ctx.order()
        with _named(where, "device route of the chimeric stages"):
            assert ctx.sv_text() == sv
            assert ctx.breakpoints() == bps
            route, fallbacks = _route(ctx.timing())
            assert route == "device"
            assert (fallbacks > 0) == (seed in FALLBACK_OK), (fallbacks, FALLBACK_OK.get(seed))
    monkeypatch.delenv("SQUID_EXACT_DEPTH")
    with squid_amd.Context(**params) as ctx:
        ctx.load(f"{pre}.bam", f"{pre}.chim.bam")
        ctx.build_graph()
        with _named(where, "production depth mode"):
            _compare(ctx, dump, sv_path, depth_exact=False)


# four seeds with four or five contigs (empty ones in front, in between and at the end) for a three-rank run
SHARDED_SEEDS = (5, 8, 9, 14)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SHARDED_SEEDS)
def test_random_shape_sharded_over_three_ranks(built, synth, tmp_path, monkeypatch, seed):
    """one context per virtual rank, each with the records of its chromosomes only (plan_shards over the case's own contig list), the
    exchanges carried in-process: every rank ends with the oracle's stages, orders, breakpoints and _sv.txt"""
    import squid_amd
    from squid_amd.dist import VirtualWorld, plan_shards
    from test_gpu_parity import _compare, _ShardView

    monkeypatch.delenv("SQUID_EXACT_DEPTH", raising=False)
    gen, flags, params = shapes.draw(seed)
    assert len(gen[gen.index("--contigs") + 1].split(",")) >= 3
    pre = synth("T2", *gen)
    where = f"seed {seed}\n" + shapes.commands(built, pre, gen, flags)
    sv_path, dump = ou.run_oracle(built, pre, tmp_path, *flags, check=False)
    assert shapes.usable(sv_path, dump), where
    _, lens = squid_amd.read_header(f"{pre}.bam")
    plan = plan_shards(lens, 3)
    ctxs = [squid_amd.Context(rank=r, world_size=3, **params) for r in range(3)]
    try:
        for r, c in enumerate(ctxs):
            c.load(f"{pre}.bam", f"{pre}.chim.bam", shard=plan[r])
        vw = VirtualWorld(ctxs)
        vw.build_graph()
        for c in ctxs:
            c.order()
        rows = vw.call_sv()
        for r, c in enumerate(ctxs):
            with _named(where, f"rank {r} of 3, plan {plan}"):
                _compare(_ShardView(c, rows[r]), dump, sv_path, depth_exact=False)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.gpu
def test_record_parse_staging_sizes_on_three_read_lengths(built, synth):
    """k_parse_records stages the 64 records of a workgroup in 18 / 22 / 28 / 40 / 63 KB of LDS, picked by the mean record length, and parses
    in place what does not fit: each size forced (SQUID_PARSE_LDS_KB is read once per process) on reads of 50, 150 and 250 bases, against
    the host decoder's arrays"""
    pres = [str(synth("T2", *shapes.draw(s)[0])) for s in LDS_SEEDS]
    code = ("import sys, json, hashlib; sys.path.insert(0, %r); import squid_amd\n"
            "out = []\n"
            "for pre in sys.argv[1:]:\n"
            "    with squid_amd.Context() as ctx:\n"
            "        ctx.load(pre + '.bam', pre + '.chim.bam'); r = ctx.records()\n"
            "    out.append({k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in r.items()})\n"
            "print(json.dumps(out))") % str(Path(__file__).resolve().parent.parent)

    def run(env):
        p = subprocess.run([sys.executable, "-c", code, *pres], env=dict(os.environ, **env), capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, env, LDS_SEEDS, p.stderr[-4000:])
        if env.get("SQUID_GPU_INFLATE") == "1":
            assert p.stderr.count("GPU inflate+parse path") >= len(pres) and "(rc 0)" in p.stderr, p.stderr[-4000:]
        return json.loads(p.stdout.strip().splitlines()[-1])

    want = run({"SQUID_GPU_INFLATE": "0", "SQUID_HOST_PARSE": "1"})
    assert len(want) == 3 and len({w["totlen"] for w in want}) == 3
    for kb in ("18", "22", "28", "40", "63"):
        got = run({"SQUID_GPU_INFLATE": "1", "SQUID_INGEST_TIMING": "1", "SQUID_PARSE_LDS_KB": kb})
        for s, g, w in zip(LDS_SEEDS, got, want):
            assert g == w, (kb, s, [k for k in w if g[k] != w[k]], " ".join(shapes.draw(s)[0]))
