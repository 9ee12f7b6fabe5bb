#!/usr/bin/env python3
"""sq_compress_windows_on_device against the per-chromosome route of FurtherCompressNode: one ingest, then resident graph passes of one
context with the route off and on, interleaved.  One JSON line per pass: the k_further_compress row (it brackets the
whole stage, k_fc_cuts included), k_fc_cuts, fc_windows, fc_longest_window, the wall time of sq_build_graph and a hash of _sv.txt; then one
line with the window lengths of the graph as it enters the stage (sq_debug_fc_windows on stage snapshot 5).
usage: fc_windows_ab.py <prefix> [passes of each route] [min_edge_weight=1 max_allowed_degree=50 ...]"""
import hashlib
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import squid_amd

pre = sys.argv[1]
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 5
params = {k: (float(v) if "." in v else int(v)) for k, v in (a.split("=") for a in sys.argv[3:])}
with squid_amd.Context(**params) as ctx:
    ctx.load(f"{pre}.bam", f"{pre}.chim.bam", threads=16)
    ctx.build_graph(); ctx.order(); ctx.sv_text()  # (warm-up: buffers, code objects)
    for k in range(2 * passes):
        on = k % 2 == 1
        ctx.compress_windows_on_device(on)
        ctx.reset()
        t0 = time.perf_counter()
        ctx.build_graph()
        wall = (time.perf_counter() - t0) * 1e3
        ctx.order()
        text = ctx.sv_text()
        t = ctx.timing()
        row = lambda name, field: t[name][field] if name in t else None
        print(json.dumps({"input": Path(pre).name, "route": "windows" if on else "per chromosome", "k_further_compress_ms": row("k_further_compress", "ms"), "k_fc_cuts_ms": row("k_fc_cuts", "ms"),
                          "fc_windows": row("fc_windows", "launches"), "fc_longest_window": row("fc_longest_window", "launches"), "build_graph_wall_ms": round(wall, 3),
                          "records": ctx.counts()["n_concordant"], "sv_rows": text.count("\n") - 1, "sv_sha256_16": hashlib.sha256(text.encode()).hexdigest()[:16]}), flush=True)
    g = ctx.graph(5)
    chroms = len({v[0] for v in g["nodes"]})
    win = ctx.debug_fc_windows([v[:4] for v in g["nodes"]], g["edges"])
    lens = sorted(b - a for a, b in zip(win, win[1:]))
    at = lambda q: lens[min(len(lens) - 1, int(q * len(lens)))]
    print(json.dumps({"input": Path(pre).name, "nodes_entering_the_stage": len(g["nodes"]), "edges": len(g["edges"]), "chromosomes": chroms, "windows": len(lens), "window_nodes": {"median": at(0.5), "p90": at(0.9),
                      "p99": at(0.99), "p999": at(0.999), "largest_ten": lens[-10:]}, "nodes_in_windows_of_at_least": {str(k): sum(x for x in lens if x >= k) for k in (64, 256, 1024, 4096)}}), flush=True)
