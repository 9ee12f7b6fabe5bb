"""The protocol of a chromosome-sharded run (squid_amd/csrc/sq_shard.h) on the CPU, without N ranks and without a device: the bytes of the six
exchange payloads against struct.pack of the documented layout, their round trip and what is refused, and the decisions a rank takes from the
gathered payloads -- dedup mask, stream merge, seed resolution, graph sum, cursor check -- on hand-made tables (tools/shard_emu.cpp, linked
against the library).  The expected values are literals worked out from the rank loops build_graph / call_sv had before the decisions became
functions; one line says why for each.  The GPU suite runs the same functions inside whole sharded runs (the sharded tests of
tests/test_gpu_parity.py)."""
import re
import struct
import subprocess

import pytest

INT64_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def shard_emu(built, tmp_path_factory):
    exe = tmp_path_factory.mktemp("shard_emu") / "shard_emu"
    root = built.parent
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-I", str(root / "include"), "-o", str(exe), str(root / "tools" / "shard_emu.cpp"),
                           "-L", str(built), "-lsquid_hip", f"-Wl,-rpath,{built}", "-lpthread"], stderr=subprocess.DEVNULL)
    return exe


def run(exe, *args):
    out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    return out.stdout


def decision(exe, *args):
    """`key=value key=value ...` of one decision; a list is comma-separated, an error is the whole line"""
    text = run(exe, *args).strip()
    if text.startswith("error="):
        return {"error": text[len("error="):]}
    return dict(kv.split("=", 1) for kv in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


# ---- a. the bytes on the wire
def i32(*xs):
    return struct.pack(f"<{len(xs)}i", *xs)


def i64(*xs):
    return struct.pack(f"<{len(xs)}q", *xs)


def vec(fmt, xs):  # a vector: an int64 count, then the elements
    return struct.pack("<q", len(xs)) + struct.pack(f"<{len(xs)}{fmt}", *xs)


def edge_key(a, b, ha, hb):  # a <= b
    return (a << 32) | (b << 2) | (ha << 1) | hb


def test_wire_bytes_of_every_payload(shard_emu):
    """the instances of wire() in tools/shard_emu.cpp, the same numbers here, laid out as the table of DESIGN.md says"""
    want = {
        "X_DEDUP": i32(0x51a0, 1, 0, 1, 1),
        "X_STREAM": i32(0x51a1) + i64(5000000000) + i32(3, 123456) + i64((7 << 32) | 99, -1),
        "X_SEEDS": i32(0x51a2) + vec("i", [0, 100, 50, 0, 400, 30]) + i32(1) + vec("i", [1, 20, 5]) + vec("i", [150, 151, 152, 153]) + i32(1) + i32(0, 100, 50)
                   + vec("i", [0, 100, 80, 0, 300, 10, 2, 7, 9]),
        "X_GRAPH": i32(0x51a3, 2, 5) + i64(77) + i32(1) + vec("i", [1, 2, 3]) + vec("i", [100, 200, 300]) + vec("i", [4, 5, 6]) + vec("i", [40, 50, 60]) + vec("i", [0, 1, 0])
                   + vec("i", [2, 0, -1]) + vec("Q", [edge_key(2, 4, 1, 0), edge_key(3, 3, 0, 1), edge_key(5, 1000000, 1, 1)]) + vec("i", [11, 7, 1]) + i64(123456789012),
        "X_BPSUP": i32(0x51a4, 6, 9, 1, 0) + i64(1234567890123, 5) + vec("i", [1, -1, 0, 2, -2]),
        "X_OTHER": i32(0x51a5) + vec("i", [0, 0, 3]) + vec("i", [10, 20, 30]) + vec("i", [76, 3, 1]),
    }
    got = dict(line.split() for line in run(shard_emu, "wire").splitlines())
    assert set(got) == set(want)
    for name, b in want.items():
        assert got[name] == b.hex(), name


# ---- b. round trip and refusal
def test_round_trip_prefixes_tags_and_huge_counts(shard_emu):
    """300 random instances of each payload (a vector is empty one time in four): unpacking the packed bytes gives the instance back, every
    proper prefix is refused, the bytes under each of the five other tags are refused by the tag rule of take_exchange and by unpack, three
    bytes are a short payload, and a first vector count of 2^62, 2^61, 2^63 - 1 or -1 is refused (by the count: a product would wrap to 0 for
    2^62 and the vector would be allocated)"""
    text = run(shard_emu, "fuzz", 300, 20261020)
    m = re.search(r"(\d+) instances, (\d+) bytes, empty first vectors (\d+), prefixes refused (\d+), other tags refused (\d+), huge counts refused (\d+), (\d+) differences", text)
    assert m and text.strip().endswith("0 differences: same"), text
    instances, nbytes, empty, prefixes, tags, huge, diff = (int(x) for x in m.groups())
    assert instances == 6 * 300 and prefixes == nbytes and tags == 5 * instances and huge == 4 * 4 * 300 and empty > 0 and diff == 0


# ---- c. decisions
def test_dedup_mask(shard_emu):
    # rank 0 has a pass-1 record with lists (bit 0 on) and no pass-2 record; rank 1 has no pass-1 record (bit 0 stays) and a pass-2 record with empty lists (bit 1 off)
    assert decision(shard_emu, "dedup", 2, "1,0,0,0", "0,0,1,1", "1,1,1,1")["dedup_mask"] == "1"
    # rank 0 sets both bits, rank 1's pass-1 record with empty lists clears bit 0 again; rank 2 is the caller itself and is not read
    assert decision(shard_emu, "dedup", 2, "1,0,1,0", "1,1,0,0", "1,0,1,0")["dedup_mask"] == "2"
    assert decision(shard_emu, "dedup", 0, "1,0,1,0", "1,0,1,0")["dedup_mask"] == "0"  # nobody in front of rank 0


def streams(exe, me, own, triggers, kept=(5, 0, 7)):
    first = ((3, 100), (9, 9), (4, 200))
    other_max = (77, 99, 88)
    ranks = [f"{kept[r]},{first[r][0]},{first[r][1]},{other_max[r]},{triggers[r]}" for r in range(3)]
    return decision(exe, "streams", me, own, *ranks)


def test_merge_streams(shard_emu):
    d = streams(shard_emu, 1, 0, (9, 0, 3))
    assert d["n_break_global"] == "10"  # 9 is not inside rank 0's 5 records, 0 not inside rank 1's none: the first trigger inside is rank 2's, at 5 + 0 + 3 = 8, plus 2
    assert d["kept_before"] == "5" and d["kept_total"] == "12" and d["prior_kept"] == "1"  # rank 0 has kept 5 records
    assert d["other_seed"] == "77"  # rank 0's running maximum (the caller's own 99 and rank 2's 88 lie behind)
    assert d["has_terminal"] == "1" and d["term"] == "4,200"  # rank 2's first kept record
    assert d["first_chr"] == "3,-1,4"  # rank 1 has kept nothing
    assert streams(shard_emu, 1, 0, (4, 0, 3))["n_break_global"] == "6"    # rank 0's trigger 4 lies inside its 5 records: 4 + 2
    assert streams(shard_emu, 1, 0, (5, 0, 7))["n_break_global"] == "12"   # no trigger inside any stream: the total 12 (14 is capped)
    assert streams(shard_emu, 1, -1, (4, 0, 3))["n_break_global"] == "1"   # this shard saw no discordant cluster at all: min(total, 1)
    assert streams(shard_emu, 1, -1, (4, 0, 3), kept=(0, 0, 0))["n_break_global"] == "0"  # ... of an empty stream
    d = streams(shard_emu, 0, 0, (9, 0, 3))
    assert d["prior_kept"] == "0" and d["kept_before"] == "0" and d["other_seed"] == str(INT64_MIN)  # nobody in front
    assert d["has_terminal"] == "1" and d["term"] == "4,200"  # rank 1 has kept nothing: the first later record is rank 2's


R0 = "0,100,50;0;;;0;0,0,0;"  # rank 0: A = [(0,100,50)], starts the stream (hasB 0)


def seeds_rank1(sens="", has_c=0, seed_c="0,0,0", c=""):
    return f"1,10,5;1;1,20,5;{sens};{has_c};{seed_c};{c}"  # rank 1: A = [(1,10,5)], B = [(1,20,5)]


def test_resolve_seeds(shard_emu):
    d = decision(shard_emu, "seeds", "0,1", R0, seeds_rank1())
    assert d["all"] == "0,100,50,1,20,5" and d["redo"] == "-1"  # the node in front lies on chromosome 0 < 1 and no start was compared with its end: B holds
    d = decision(shard_emu, "seeds", "0,1", R0, seeds_rank1(sens="150"))
    assert d["redo"] == "1" and d["last"] == "0,100,50"  # a pending start was compared with 100 + 50 without a chromosome test: the exact past is needed
    d = decision(shard_emu, "seeds", "0,0", R0, seeds_rank1())
    assert d["redo"] == "1" and d["last"] == "0,100,50"  # the node in front lies on the shard's own first chromosome
    d = decision(shard_emu, "seeds", "0,0", R0, seeds_rank1(has_c=1, seed_c="0,100,50", c="0,100,80,0,300,10"))
    assert d["all"] == "0,100,80,0,300,10" and d["redo"] == "-1"  # replayed behind exactly that node: C's first node replaces it (extended), the rest follows
    d = decision(shard_emu, "seeds", "-1,1", R0, seeds_rank1())
    assert d["all"] == "1,10,5" and d["redo"] == "-1"  # rank 0 has kept nothing and emits nothing: nothing in front of rank 1, its A is taken
    for seed_c in ("1,100,50", "0,101,50", "0,100,51"):  # a replay behind another node than the real last one does not count
        d = decision(shard_emu, "seeds", "0,0", R0, seeds_rank1(has_c=1, seed_c=seed_c, c="0,100,80,0,300,10"))
        assert d["redo"] == "1" and d["last"] == "0,100,50", seed_c


C0 = "0;4;1;1;3;0;1,0,2,0,-1,0,0,-2"  # rank 0 over 7 breakpoints: pass-3 records, one moved the cursor, from 0 to 4


def test_check_cursors(shard_emu):
    d = decision(shard_emu, "cursors", 7, C0, "4;6;1;1;2;0;0,0,0,0,1,1,-1,-1")
    assert d["bad"] == "-1" and d["truth"] == "6" and d["total"] == "1,0,2,0,0,1,-1,-3"  # rank 1 assumed what rank 0 left: the arrays add up
    d = decision(shard_emu, "cursors", 7, C0, "6;7;1;1;2;1;0,0,0,0,1,1,-1,-1")
    assert d["bad"] == "1" and d["truth"] == "4"  # two entries behind the guess, only one record to catch up with
    assert decision(shard_emu, "cursors", 7, C0, "3;7;1;1;2;9;0,0,0,0,1,1,-1,-1")["bad"] == "1"  # the real cursor is already beyond the guess
    d = decision(shard_emu, "cursors", 7, "0;4;0;1;3;0;1,0,2,0,-1,0,0,-2", "2;2;1;0;1;5;0,0,0,0,1,1,-1,-1")
    # rank 0 has no pass-3 record: the cursor passes through at 0 and its array is not added; rank 1 is 2 behind with 5 records to catch up
    # in, and without an event the cursor ends at min(2, 0 + 1)
    assert d["bad"] == "-1" and d["truth"] == "1" and d["total"] == "0,0,0,0,1,1,-1,-1"
    assert decision(shard_emu, "cursors", 7, C0, "4;6;1;1;2;0;0,0,0,0,1,1,-1")["error"] == "sharded run: malformed breakpoint payload"


G0 = "0;2;3;0;1,2;10,20;3,4;30,40;0,1;1,0;0:1:0:1:5,1:0:1:1:2;10"
G1 = "2;5;4;1;1,1,1;2,2,2;3,3,3;4,4,4;5,5,5;6,6,6;4:2:1:0:9;20"


def test_merge_graph(shard_emu):
    d = decision(shard_emu, "graph", 5, G0, G1)
    assert d["sup"] == "1,2,1,1,1,3,4,3,3,3,7"  # main support of nodes 0..4, other support of nodes 0..4, |ReadsOther| = 3 + 4
    assert d["sl"] == "10,20,2,2,2,30,40,4,4,4" and d["amb_plus"] == "0,1,5,5,5" and d["amb_minus"] == "1,0,6,6,6"
    assert d["tiny"] == "1" and d["n_raw"] == "30"  # one shard saw a tiny boundary block; raw edges add up
    assert d["conc"] == "0:1:0:1:5:0,0:1:1:1:2:0,2:4:0:1:9:0"  # (a, b, head a, head b, weight, group weight 0) with a <= b as make_edge orders them
    malformed = {"error": "sharded run: malformed graph payload"}
    assert decision(shard_emu, "graph", 5, G0, "2;6;4;1;1,1,1,1;2,2,2,2;3,3,3,3;4,4,4,4;5,5,5,5;6,6,6,6;;20") == malformed  # hi > nn
    assert decision(shard_emu, "graph", 5, G0, "3;2;4;1;;;;;;;;20") == malformed                                        # lo > hi
    assert decision(shard_emu, "graph", 5, G0, "2;5;4;1;1,1,1;2,2,2;3,3,3;4,4;5,5,5;6,6,6;;20") == malformed             # a vector that is not hi - lo long


def test_gather_other(shard_emu):
    assert decision(shard_emu, "other", "0,1;10,20;76,3", ";;", "0;5;9")["other"] == "0:10:76,1:20:3,0:5:9"  # rank order, which is the stream order
    assert decision(shard_emu, "other", "0,1;10,20;76,3", "0;5,6;9")["error"] == "sharded run: malformed ReadsOther payload"
