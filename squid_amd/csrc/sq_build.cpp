// The pipelines behind sq_build_graph and sq_call_sv, stage by stage.  Each is resumable (GraphBuild::stage, SvBuild::stage): in a
// chromosome-sharded run a stage first takes what the previous exchange gathered (sq_shard.h), runs its step of the single-GPU pipeline
// and packs the next payload; an unsharded run walks the same stages in one call.
#include <algorithm>
#include <future>

#include "sq_shard.h"
#include "sq_parsort.h"

namespace sq {

// CompressNode .. MultiplyDisEdges of the constructor (SegmentGraph.cpp:117-122), shared by the STAR and the --bwa path
// SQUID_HOST_FILTERS: the edge filters and the node compression on the host (cross-check of the device route)
static bool host_filters_env() { static const bool v = env_set("SQUID_HOST_FILTERS"); return v; }

static int finish_graph(sq_ctx* c, bool host_filters) {
    int rc;
    {
        HostClock hc(c, host_filters ? "host_compress" : "wall_compress");
        rc = host_filters ? compress_nodes(c) : dev_compress_nodes(c);
        if (rc) return rc;
        if (c->keep_stages) c->snap[5].take(c->nodes, c->edges, nullptr);
        rc = host_filters ? further_compress(c) : dev_further_compress(c);
        if (rc == 2) rc = further_compress(c);  // a node with more discordant edges than the kernel's lists hold
        if (rc) return rc;
    }
    rc = dev_connected_components(c, (int)c->nodes.size(), c->edges, c->label);
    if (rc) return rc;
    multiply_discordant(c, false);
    c->snap[0].take(c->nodes, c->edges, &c->label);
    c->graph_built = true;
    c->gb.reset();
    // ExactBreakpoint only needs the final graph and the trimmed fragments: start it now, sq_call_sv collects it
    c->chim_s2_pending = false;
    if (c->chim_s1_device) {  // the trimmed blocks are in HBM: the stage is queued on the stream behind the graph (sq_chim_stage.inc)
        bool fb = false;
        rc = dev_exact_breakpoints_start(c, fb);
        if (rc) return rc;
        if (!fb) { c->chim_s2_pending = true; return SQ_OK; }
        c->timer.add("chim_device_fallback", 0, 0, 1);
        if ((rc = dev_chim_download_trimmed(c))) return rc;  // (the host stage continues from the blocks as stage 1 left them)
        c->chim_s1_device = false;
    }
    c->bp_early = std::make_shared<BPMap>();
    c->bp_future = c->pool->submit([c]() {
        const auto t0 = std::chrono::steady_clock::now();
        const int r2 = exact_breakpoints(c, *c->bp_early);
        c->bp_early_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return r2;
    });
    return SQ_OK;
}

// FilterbyWeight, FilterbyInterleaving, FilterEdges: K6 / K7 on the device (sq_graph_kernels.inc); SQUID_HOST_FILTERS=1 takes the host
// restatements of sq_graph.cpp instead (kept as a cross-check: tests compare the two stage by stage).  before (may be null): the edges in
// front of FilterEdges
static int run_filters(sq_ctx* c, bool host_filters, std::vector<uint8_t>& keep, std::vector<Edge>* before) {
    int rc;
    if (host_filters) filter_by_weight(c); else if ((rc = dev_filter_by_weight(c))) return rc;
    if (c->keep_stages) c->snap[3].take(c->nodes, c->edges, nullptr);
    if (host_filters) filter_by_interleaving(c, keep); else if ((rc = dev_filter_by_interleaving(c, keep))) return rc;
    if (before) *before = c->edges;
    if (host_filters) filter_edges(c, keep); else if ((rc = dev_filter_edges(c, keep))) return rc;
    return SQ_OK;
}

// `squid --bwa`: BuildNode_BWA and RawEdges on the host over the decoded batch (sq_bwa.cpp), then the same edge reduction, filters,
// compression and component labelling as the STAR path (SegmentGraph.cpp:104-124 with UsingSTAR == false).  Node depths are exact
// here (no unstable sort in this mode's depth sweep), so the coverage-ratio test needs no bounds.
int build_graph_bwa(sq_ctx* c) {
    HostClock wall(c, "wall_build_graph");
    if (c->shard.on) return fail(c, SQ_E_ARG, "--bwa input is not chromosome-sharded");
    c->graph_built = false; c->ordered = false;
    c->depth_bounds = false; c->depth_ambiguous = false;
    c->chim_s1_device = false;
    std::vector<Edge> raw;
    int rc = bwa_nodes_and_edges(c, raw);
    if (rc) return rc;
    // (counts.n_raw_edges: set by bwa_raw_edges -- the edges as the loop emitted them; `raw` arrives summed per stretch)
    c->edges.clear();
    { HostClock hc(c, "host_edge_reduce"); reduce_edges(raw, c->edges, c->pool ? std::min(c->pool->size() + 1, 32) : 1); }
    c->counts.n_unique_edges = (int64_t)c->edges.size();
    if (c->keep_stages) c->snap[2].take(c->nodes, c->edges, nullptr);
    const bool host_filters = host_filters_env();
    {
        HostClock hc(c, host_filters ? "host_filters" : "wall_filters");
        std::vector<uint8_t> keep;
        if ((rc = run_filters(c, host_filters, keep, nullptr))) return rc;
        if (c->keep_stages) c->snap[4].take(c->nodes, c->edges, nullptr);
    }
    return finish_graph(c, host_filters);
}

// ---- stage 0: the cluster table beside the record classification; packs exchange 1
static int stage_classify(sq_ctx* c, GraphBuild& g) {
    c->graph_built = false;
    c->ordered = false;
    // the cluster table only needs the chimeric fragments: build it on a second thread next to the record kernels
    // (the table is a function of the chimeric fragments and ReadLen alone: built beside the ingest by sq_ingest_files, or by the first pass,
    // and KEPT by the context until the fragments change -- a later pass over the same records, sq_reset and a new set of -w/-r/-a, takes
    // it as it is; everything a pass writes into the plan is written again by the next one)
    if (c->clusters_early_ms >= 0 && c->plan_early) {
        g.plan = c->plan_early; g.disc = c->disc_early;
        std::promise<double> done;
        done.set_value(c->clusters_early_ms);
        g.clusters = done.get_future();
        c->clusters_early_ms = 0;  // (a second use costs nothing)
    } else g.clusters = c->pool->submit([c, &g]() { const double ms = segment_clusters(c, g.plan, g.disc); c->plan_early = g.plan; c->disc_early = g.disc; c->clusters_early_ms = 0; return ms; });
    XDedup x;
    const int rc = dev_classify(c, c->shard.on ? x.last : nullptr);
    if (rc) { (void)g.clusters.get(); return rc; }
    g.stage = 1;
    if (!c->shard.on) return SQ_OK;
    x.pack(c->xbuf);
    return need_exchange(c);
}

// ---- stage 1: the dedup mask from exchange 1; the stream scans that need nothing from other shards; packs exchange 2
static int stage_scan(sq_ctx* c, GraphBuild& g) {
    int rc;
    if (c->shard.on) {
        std::vector<XDedup> got;
        if ((rc = take_payloads(c, got, "dedup"))) return rc;
        c->shard.dedup_mask = dedup_mask(got, c->P.rank);
    }
    const double cl_ms = g.clusters.get();  // (k_pass1 needs the cluster table up front: it reads the records once, for everything)
    c->timer.add("host_cluster_table", cl_ms);
    XStream x;
    int32_t first_kept[2] = {0, 0};
    long long other_max = INT64_MIN;
    {
        HostClock hc(c, "host_segment_prepare");
        rc = segment_scan(c, *g.plan, c->shard.on, g.trigger_last, other_max, first_kept);
        if (rc) return rc;
    }
    g.stage = 2;
    if (!c->shard.on) return SQ_OK;
    x.kept = c->counts.n_kept_p1; x.first_refid = first_kept[0]; x.first_pos = first_kept[1]; x.other_max = other_max; x.trigger_last = g.trigger_last;
    x.pack(c->xbuf);
    return need_exchange(c);
}

// ---- stage 2: where this shard's stream lies in the whole one, from exchange 2; the stretches to replay and their replay, on the device or
// on the host (a shard that does not start the stream replays under both pasts, side by side); packs exchange 3
static int stage_replay(sq_ctx* c, GraphBuild& g) {
    const Shard& sh = c->shard;
    int rc;
    if (sh.on) {
        std::vector<XStream> got;
        if ((rc = take_payloads(c, got, "stream"))) return rc;
        merge_streams(got, c->P.rank, g.trigger_last, c->shard, g.first_chr);
    }
    {
        HostClock hc(c, "host_segment_prepare");
        rc = segment_prepare(c, *g.plan, g.n_break);
        if (rc) return rc;
    }
    c->counts.n_break = g.n_break;
    g.seedsB.clear(); g.sensB.clear(); g.hasC = false;
    bool seg_on_device = false;
    if (c->seg_dev_on()) {  // (sq_segment_on_device: one wave per stretch, the host walks the reports; a plan too large comes back)
        SegWalk W;
        bool fb = false;
        c->timer.add("segment_device_fallback", 0, 0, 0);
        rc = segment_replay_device(c, *g.plan, g.seeds, W, fb);
        if (rc) return rc;
        if (fb) c->timer.add("segment_device_fallback", 0, 0, 1);
        else {
            seg_on_device = true;
            c->timer.add("segment_stretches", 0, 0, W.stretches); c->timer.add("segment_stretches_run_again", 0, 0, W.again); c->timer.add("segment_longest_stretch", 0, 0, W.longest);
        }
    }
    if (!seg_on_device) {
        HostClock hc(c, "host_segment_replay");
        std::future<int> hypB;  // (captures g: joined below, before any return)
        if (sh.on && sh.prior_kept) hypB = c->pool->submit([c, &g]() { return segment_replay(c, *g.plan, g.seedsB, true, &g.sensB, nullptr); });
        rc = segment_replay(c, *g.plan, g.seeds, false, nullptr, nullptr);
        if (hypB.valid()) { const int rb = hypB.get(); if (!rc) rc = rb; }
    }
    if (rc) return rc;
    g.seedsA = g.seeds;
    g.stage = 3;
    if (!sh.on) return SQ_OK;
    pack_seeds(c, g);
    return need_exchange(c);
}

// exchange 4 carries the accumulators of the shard's own nodes only: nothing may have been counted anywhere else
static int pack_graph_slice(sq_ctx* c, const GraphBuild& g) {
    const std::vector<Node>& N = c->nodes;
    const int nn = (int)N.size();
    XGraph x;
    while (x.lo < nn && N[x.lo].chr < c->shard.first_ref) ++x.lo;
    x.hi = x.lo;
    while (x.hi < nn && N[x.hi].chr < c->shard.end_ref) ++x.hi;
    for (int i = 0; i < nn; ++i)
        if ((i < x.lo || i >= x.hi) && (g.sup[i] || g.sup[nn + i] || g.sl[i] || g.sl[nn + i] || g.amb_plus[i] || g.amb_minus[i]))
            return fail(c, SQ_E_ARG, "internal: a record of this shard was counted for a node of another shard");
    x.n_other = (int64_t)g.sup[2 * nn];
    x.tiny = g.tiny_boundary ? 1 : 0;
    for (int i = x.lo; i < x.hi; ++i) {
        x.v[0].push_back(g.sup[i]); x.v[1].push_back((int32_t)g.sl[i]); x.v[2].push_back(g.sup[nn + i]); x.v[3].push_back((int32_t)g.sl[nn + i]);
        x.v[4].push_back(g.amb_plus[i]); x.v[5].push_back(g.amb_minus[i]);
    }
    for (const Edge& e : g.conc) { x.keys.push_back(edge_pack(e)); x.ws.push_back(e.w); }
    x.n_raw = c->counts.n_raw_edges;
    x.pack(c->xbuf);
    return SQ_OK;
}

// ---- stage 3: the seed nodes of all shards from exchange 3 (a shard that has to replay again behind the real last node does, and
// everybody exchanges once more); the nodes; chimeric edges beside the depth and edge kernels over the concordant stream; packs exchange 4
static int stage_nodes_and_edges(sq_ctx* c, GraphBuild& g) {
    int rc;
    if (c->shard.on) {
        std::vector<XSeeds> got;
        if ((rc = take_payloads(c, got, "seed"))) return rc;
        std::vector<Node> all;
        int redo = -1;
        Node last{0, 0, 0, 0, 0.0};
        resolve_seeds(got, g.first_chr, all, redo, last);
        if (redo == c->P.rank) {
            HostClock hc(c, "host_segment_replay");
            g.seedC = last; g.hasC = true;
            rc = segment_replay(c, *g.plan, g.seedsC, false, nullptr, &g.seedC);
            if (rc) return rc;
        }
        if (redo >= 0) { pack_seeds(c, g); return need_exchange(c); }
        g.seeds.swap(all);
    }
    {
        HostClock hc(c, "host_tile_genome");
        std::vector<Node> seedcopy = g.seeds;
        rc = tile_genome(c, seedcopy, c->nodes);
    }
    if (rc) return rc;
    rc = dev_upload_nodes(c, c->nodes);
    if (rc) return rc;
    c->edges.clear();
    // (sq_chimeric_on_device: RawEdgesChim as kernels on this stream, in front of the depth stage; a stage with more soft fragments than
    // the bound comes back and takes the host route below)
    c->chim_s1_device = false;
    if (c->chim_dev_on()) {
        bool fb = false;
        c->timer.add("chim_device_fallback", 0, 0, 0);
        rc = dev_chimeric_edges(c, g.raw, fb);
        if (rc) return rc;
        if (fb) c->timer.add("chim_device_fallback", 0, 0, 1); else c->chim_s1_device = true;
    }
    // the chimeric edges are host work on the (small) fragment list: do them on a second thread while this one
    // drives the depth and edge kernels over the concordant stream
    double chim_ms = 0;
    std::future<int> chim;  // (captures g and chim_ms: joined below, before any return)
    if (!c->chim_s1_device) chim = c->pool->submit([c, &g, &chim_ms]() {
        const auto t0 = std::chrono::steady_clock::now();
        const int r2 = chimeric_edges(c, g.raw);
        chim_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return r2;
    });
    std::vector<int32_t> unused;
    rc = dev_node_depth(c, c->nodes, g.n_break, g.sup, g.sl, g.tiny_boundary, g.amb_plus, g.amb_minus, unused);
    const int rc_edges = rc ? rc : dev_concordant_edges(c, c->nodes, g.conc);
    const int rc_chim = chim.valid() ? chim.get() : SQ_OK;
    if (!c->chim_s1_device) c->timer.add("host_chimeric_edges", chim_ms);
    if (rc_chim) return rc_chim;
    if (rc_edges) return rc_edges;
    g.stage = 4;
    if (!c->shard.on) return SQ_OK;
    if ((rc = pack_graph_slice(c, g))) return rc;
    return need_exchange(c);
}

// ---- per-node Support / AvgDepth (SegmentGraph.cpp:766-826): discordant blocks on the host, stream blocks from the GPU.
// ReadsOther (non-first blocks) is sorted with an unstable std::sort in the reference (SegmentGraph.cpp:781) and a
// block of <= 3 bases right behind a node boundary is counted for whichever node the sweep cursor is on, which
// depends on that sort's tie order.  Node depths only feed the coverage-ratio test of FilterEdges, so by default
// the GPU reports canonical depths plus bounds over all tie orders and FilterEdges checks that no decision can
// change inside the bounds; only then (or when SQUID_EXACT_DEPTH is set, as the stage-parity tests do) is the
// reference's sort repeated on the host and the sweep walked exactly.
struct NodeDepths {
    std::vector<int32_t> dis_cnt, dis_sum;  // per node: discordant blocks inside it, their bases
    std::vector<int32_t> ocnt, osum;        // per node: ReadsOther blocks and bases, canonical (the device's) or from the exact sweep
    std::vector<OtherR> other;              // the ReadsOther list of the exact sweep, sorted as the reference sorts it
};
static void discordant_depths(const std::vector<Node>& N, const std::vector<Blk>& disc, NodeDepths& d) {
    const int nn = (int)N.size();
    d.dis_cnt.assign(nn, 0); d.dis_sum.assign(nn, 0);
    size_t it = 0;
    for (int i = 0; i < nn; ++i) {
        int cnt = 0, sum = 0;
        for (; it != disc.size() && disc[it].refid == N[i].chr && disc[it].refpos < N[i].pos + N[i].len; ++it)
            if (disc[it].refpos >= N[i].pos && disc[it].refpos + disc[it].matchref <= N[i].pos + N[i].len) { ++cnt; sum += disc[it].matchref; }
        d.dis_cnt[i] = cnt; d.dis_sum[i] = sum;
    }
}
static void sort_other(std::vector<OtherR>& other) {
    std::sort(other.begin(), other.end(), [](const OtherR& a, const OtherR& b) { return a.chr != b.chr ? a.chr < b.chr : a.pos < b.pos; });
}
// always: fetch the list even when no block sits in a corner (the forced retry of the tests)
static int fetch_other(sq_ctx* c, int64_t n_break, bool always, std::vector<OtherR>& other) {
    std::vector<int32_t> ochr, opos, olen;
    bool has_tiny = false;
    const int rc = dev_gather_other(c, n_break, has_tiny, ochr, opos, olen, always);
    if (rc) return rc;
    other.resize(has_tiny || always ? ochr.size() : 0);
    for (size_t i = 0; i < other.size(); ++i) other[i] = OtherR{ochr[i], opos[i], olen[i]};
    sort_other(other);
    return SQ_OK;
}
static void exact_sweep(const std::vector<Node>& N, NodeDepths& d) {
    const int nn = (int)N.size();
    d.ocnt.assign(nn, 0); d.osum.assign(nn, 0);
    size_t it = 0;
    for (int i = 0; i < nn; ++i)
        for (; it != d.other.size(); ++it) {
            const OtherR& r = d.other[it];
            if (r.chr == N[i].chr && r.pos >= N[i].pos - 3 && r.pos + r.len <= N[i].pos + N[i].len + 3) { d.ocnt[i]++; d.osum[i] += r.len; }
            else if (r.pos >= N[i].pos + N[i].len || r.chr != N[i].chr) break;
        }
}
// combine in the reference's order: discordant, ReadsMain, ReadsOther, then the division (only when ReadsOther is non-empty, ledger B13)
static void set_depths(sq_ctx* c, const GraphBuild& g, const NodeDepths& d, bool bounds) {
    std::vector<Node>& N = c->nodes;
    const int nn = (int)N.size();
    const int64_t n_other = g.sup[2 * nn];
    c->depth_bounds = bounds;
    for (int i = 0; i < nn; ++i) {
        N[i].support = d.dis_cnt[i] + g.sup[i];
        double v = d.dis_sum[i];
        v += (int32_t)g.sl[i];
        double lo = v, hi = v;
        if (n_other != 0) {
            N[i].support += d.ocnt[i];
            v += d.osum[i];
            lo = v; hi = v;
            if (bounds) { lo = v - g.amb_minus[i]; hi = v + g.amb_plus[i]; }
            v = 1.0 * v / N[i].len; lo = 1.0 * lo / N[i].len; hi = 1.0 * hi / N[i].len;
        }
        N[i].depth = v; N[i].depth_lo = lo; N[i].depth_hi = hi;
    }
}

// Some coverage-ratio decision depends on the tie order: repeat the reference's sort and sweep, then redo the filter with the exact
// depths.  A sharded run needs every shard's ReadsOther for that (the tie order of the unstable sort depends on the whole list): one more
// exchange (5) -- the lists, in rank order, are the unsharded stream order
static int exact_depth_retry(sq_ctx* c, GraphBuild& g, NodeDepths& d, bool resumed, bool host_filters) {
    HostClock hc(c, "host_depth_exact_retry");
    int rc;
    if (c->shard.on && !resumed) {
        XOther x;
        bool has_tiny = false;
        rc = dev_gather_other(c, g.n_break, has_tiny, x.chr, x.pos, x.len, true);
        if (rc) return rc;
        x.pack(c->xbuf);
        g.stage = 5;
        return need_exchange(c);
    }
    if (c->shard.on) {
        std::vector<XOther> got;
        if ((rc = take_payloads(c, got, "ReadsOther"))) return rc;
        if (const char* err = gather_other(got, d.other)) return fail(c, SQ_E_ARG, err);
        sort_other(d.other);
    } else if ((rc = fetch_other(c, g.n_break, true, d.other))) return rc;  // (with nothing fetched the sweep below would zero every ReadsOther contribution)
    exact_sweep(c->nodes, d);
    set_depths(c, g, d, false);
    c->depth_ambiguous = false;
    c->edges = g.before;
    if (host_filters) filter_edges(c, g.keep); else if ((rc = dev_filter_edges(c, g.keep))) return rc;
    return SQ_OK;
}

// ---- stage 4: the summed accumulators and edges from exchange 4; node depths; edge reduction; the filters, repeated with exact depths when
// a decision was ambiguous (a sharded run packs exchange 5 for that and comes back as stage 5, which recomputes the depths from g)
static int stage_depths_and_filters(sq_ctx* c, GraphBuild& g) {
    const Shard& sh = c->shard;
    const int nn = (int)c->nodes.size();
    const bool resumed = g.stage == 5;
    int rc;
    if (sh.on && !resumed) {
        std::vector<XGraph> got;
        if ((rc = take_payloads(c, got, "graph"))) return rc;
        if (const char* err = merge_graph(got, nn, g.sup, g.sl, g.amb_plus, g.amb_minus, g.tiny_boundary, g.conc, c->counts.n_raw_edges)) return fail(c, SQ_E_ARG, err);
    }
    NodeDepths d;
    { HostClock hc(c, "host_depth_discordant"); discordant_depths(c->nodes, g.disc, d); }
    d.ocnt.resize(nn); d.osum.resize(nn);
    for (int i = 0; i < nn; ++i) { d.ocnt[i] = g.sup[nn + i]; d.osum[i] = (int32_t)g.sl[nn + i]; }
    // (a sharded run cannot repeat the reference's sort by itself -- its tie order depends on the whole list: see exact_depth_retry)
    const bool exact_mode = env_set("SQUID_EXACT_DEPTH") && !sh.on;
    c->depth_ambiguous = false;
    if (exact_mode && g.tiny_boundary) {
        HostClock hc(c, "host_depth_exact_sweep");
        if ((rc = fetch_other(c, g.n_break, false, d.other))) return rc;
        if (!d.other.empty()) exact_sweep(c->nodes, d);
        set_depths(c, g, d, false);
    } else set_depths(c, g, d, g.tiny_boundary);
    const bool host_filters = host_filters_env();
    if (!resumed) {
        if (c->keep_stages) c->snap[1].take(c->nodes, c->edges, nullptr);
        {
            HostClock hc(c, "host_edge_reduce");
            g.raw.insert(g.raw.end(), g.conc.begin(), g.conc.end());
            reduce_edges(g.raw, c->edges, c->pool ? std::min(c->pool->size() + 1, 32) : 1);
        }
        if (c->keep_stages) c->snap[2].take(c->nodes, c->edges, nullptr);
    }
    {
        HostClock hc(c, host_filters ? "host_filters" : "wall_filters");
        if (!resumed) {
            if ((rc = run_filters(c, host_filters, g.keep, &g.before))) return rc;
            if (env_set("SQUID_FORCE_DEPTH_RETRY")) c->depth_ambiguous = true;  // (tests: take the exact sweep whatever the bounds say)
        }
        if ((c->depth_ambiguous || resumed) && (rc = exact_depth_retry(c, g, d, resumed, host_filters))) return rc;
        if (c->keep_stages) c->snap[4].take(c->nodes, c->edges, nullptr);
    }
    return finish_graph(c, host_filters);
}

int build_graph(sq_ctx* c) {
    HostClock wall(c, "wall_build_graph");
    if (!c->gb) c->gb = std::make_shared<GraphBuild>();
    GraphBuild& g = *c->gb;
    for (;;) {  // a stage that packed a payload returns SQ_NEED_EXCHANGE; the next call resumes at g.stage
        int rc;
        switch (g.stage) {
        case 0: rc = stage_classify(c, g); break;
        case 1: rc = stage_scan(c, g); break;
        case 2: rc = stage_replay(c, g); break;
        case 3: rc = stage_nodes_and_edges(c, g); break;
        case 4: case 5: return stage_depths_and_filters(c, g);  // (ends in finish_graph, which drops g)
        default: return fail(c, SQ_E_ARG, "internal: bad build stage");
        }
        if (rc) return rc;
    }
}

// ---- sq_call_sv
// [lo, hi) pieces on the context's host threads
static void par(sq_ctx* c, size_t n, const std::function<void(size_t, size_t)>& f) {
    const int np = (c->pool && n > 20000) ? 4 * (c->pool->size() + 1) : 1;
    if (np <= 1) { f(0, n); return; }
    c->pool->parallel_for(np, 1 << 20, [&](int k) { f(n * (size_t)k / (size_t)np, n * ((size_t)k + 1) / (size_t)np); });
}

// breakpoint list of every edge (SegmentGraph.cpp:3091-3109): the pairs ExactBreakpoint found, else the node ends the edge touches;
// then all of them as one sorted list
static int sv_breakpoints(sq_ctx* c, SvBuild& v) {
    const std::vector<Node>& N = c->nodes;
    const std::vector<Edge>& E = c->edges;
    BPMap& bpmap = v.bpmap;
    int rc;
    if (c->chim_s2_pending || c->chim_s1_device) {  // (chim_s1_device without a pending stage: a second sq_call_sv on the same graph)
        if (!c->chim_s2_pending) { bool fb = false; rc = dev_exact_breakpoints_start(c, fb); if (rc) return rc; if (fb) return fail(c, SQ_E_ARG, "internal: the breakpoint stage of this graph ran on the device before and does not now"); }
        c->chim_s2_pending = false;
        rc = dev_exact_breakpoints_collect(c, bpmap);
        if (rc) return rc;
    } else if (c->bp_future.valid()) {
        rc = c->bp_future.get();
        c->timer.add("host_exact_breakpoints", c->bp_early_ms);
        if (rc) return rc;
        bpmap.swap(*c->bp_early);
        c->bp_early.reset();
    } else {
        HostClock hc(c, "host_exact_breakpoints");
        rc = exact_breakpoints(c, bpmap);
        if (rc) return rc;
    }
    const size_t m = E.size();
    v.eoff.assign(m + 1, 0); v.eexact.assign(m, 0);
    std::vector<const std::vector<std::pair<int, int>>*> hit(m, nullptr);
    par(c, m, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            BPMap::const_iterator it = bpmap.find(edge_pack(E[i]));
            if (it != bpmap.end() && !it->second.empty()) { hit[i] = &it->second; v.eexact[i] = 1; v.eoff[i + 1] = (int32_t)it->second.size(); }
            else v.eoff[i + 1] = 1;
        }
    });
    for (size_t i = 0; i < m; ++i) v.eoff[i + 1] += v.eoff[i];
    v.ebp.resize((size_t)v.eoff[m]);
    par(c, m, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const Edge& e = E[i];
            size_t o = (size_t)v.eoff[i];
            if (hit[i]) for (const auto& p : *hit[i]) v.ebp[o++] = {{N[e.a].chr, p.first}, {N[e.b].chr, p.second}};
            else v.ebp[o] = {{N[e.a].chr, e.ha ? N[e.a].pos : N[e.a].pos + N[e.a].len}, {N[e.b].chr, e.hb ? N[e.b].pos : N[e.b].pos + N[e.b].len}};
        }
    });
    std::vector<std::pair<int, int>>& BPs = v.BPs;
    BPs.resize(2 * v.ebp.size());
    par(c, v.ebp.size(), [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; ++k) { BPs[2 * k] = v.ebp[k].first; BPs[2 * k + 1] = v.ebp[k].second; } });
    // (equal elements are indistinguishable pairs: any sort gives the reference's sorted list; the threaded introsort of sq_parsort.h)
    std_sort_parallel(BPs.begin(), BPs.end(), std::less<std::pair<int, int>>(), c->pool ? std::min(c->pool->size() + 1, 32) : 1, true);
    return SQ_OK;
}

static void pack_bpsup(sq_ctx* c, const SvBuild& v) {
    XBpSup x;
    x.assumed = v.cur_prev; x.end = v.bb.cur_end; x.has_p3 = v.bb.has_p3 ? 1 : 0; x.has_event = v.bb.has_event ? 1 : 0;
    x.n_p3 = v.bb.n_p3; x.absorb = v.bb.absorb;
    x.diff = v.diff;
    x.pack(c->xbuf);
}
// concordant support of every breakpoint: --bwa over the host batch or the resident table, one GPU over its records, or -- sharded -- this
// shard's difference array from a guessed cursor, packed for the exchange that verifies the guess (sv_cursors)
static int sv_support(sq_ctx* c, SvBuild& v, std::vector<int32_t>& cov) {
    static const bool bp_host = env_set("SQUID_BP_HOST");  // debug cross-check of k_bp_walk
    const std::vector<std::pair<int, int>>& BPs = v.BPs;
    // (--bwa: the records and their names are on the host; sq_bwa_on_device: the records are in HBM as well)
    if (c->bwa) return c->bwa_dev_active ? bwa_breakpoint_support_device(c, BPs, cov) : bwa_breakpoint_support(c, BPs, cov);
    if (!c->shard.on) return bp_host ? dev_breakpoint_support_exact(c, BPs, cov) : dev_breakpoint_support(c, BPs, cov);
    // the cursor (SegmentGraph.cpp:3157) is carried from shard to shard: start from the usual state -- every
    // breakpoint on an earlier chromosome is behind it -- and let the exchange verify that guess
    v.cur_prev = (int)(std::lower_bound(BPs.begin(), BPs.end(), std::make_pair(c->shard.first_ref, INT32_MIN)) - BPs.begin());
    const int rc = dev_breakpoint_support(c, BPs, v.diff, v.cur_prev, &v.bb, true);
    if (rc) return rc;
    pack_bpsup(c, v);
    v.stage = 1;
    return need_exchange(c);
}
// the gathered difference arrays and cursors: summed when every guess held; else the rank that started from a wrong cursor (an earlier
// shard ended while the cursor was still catching up) recounts from the real one and everybody exchanges again
static int sv_cursors(sq_ctx* c, SvBuild& v, std::vector<int32_t>& cov) {
    std::vector<XBpSup> got;
    int rc = take_payloads(c, got, "breakpoint");
    if (rc) return rc;
    const size_t nb = v.BPs.size();
    std::vector<int64_t> total;
    int truth = 0, bad = -1;
    if (const char* err = check_cursors(got, nb, total, bad, truth)) return fail(c, SQ_E_ARG, err);
    if (bad >= 0) {
        if (bad == c->P.rank) {
            v.cur_prev = truth;
            rc = dev_breakpoint_support(c, v.BPs, v.diff, v.cur_prev, &v.bb, true);
            if (rc) return rc;
        }
        pack_bpsup(c, v);
        return need_exchange(c);
    }
    cov.assign(nb, 0);
    int64_t run = 0;
    for (size_t i = 0; i < nb; ++i) { run += total[i]; cov[i] = (int32_t)run; }
    return SQ_OK;
}

// the per-edge breakpoint table in key order (parity tests), then the rows of _sv.txt
static void sv_select(sq_ctx* c, SvBuild& v, const std::vector<int32_t>& cov) {
    const std::vector<Node>& N = c->nodes;
    std::vector<Edge>& E = c->edges;
    const std::vector<std::pair<int, int>>& BPs = v.BPs;
    const size_t m = E.size(), nbp = v.ebp.size();
    std::vector<int32_t> sup1(nbp), sup2(nbp);
    par(c, nbp, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; ++k) {
            sup1[k] = cov[(size_t)(std::lower_bound(BPs.begin(), BPs.end(), v.ebp[k].first) - BPs.begin())];
            sup2[k] = cov[(size_t)(std::lower_bound(BPs.begin(), BPs.end(), v.ebp[k].second) - BPs.begin())];
        }
    });
    c->bp_off.assign(v.eoff.begin(), v.eoff.end());
    c->bp1.resize(nbp); c->bp2.resize(nbp);
    c->bsup1 = sup1; c->bsup2 = sup2;
    par(c, m, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            for (int32_t k = v.eoff[i]; k < v.eoff[i + 1]; ++k) { c->bp1[(size_t)k] = v.eexact[i] ? v.ebp[(size_t)k].first.second : -1; c->bp2[(size_t)k] = v.eexact[i] ? v.ebp[(size_t)k].second.second : -1; }
    });
    multiply_discordant(c, true);
    // WriteBEDPE (src/WriteIO.cpp:45-124): unstable sort by weight on the key-sorted edge list (ledger B8).  What is sorted is the index of
    // every edge with the reference's comparison on the weights: libstdc++'s introsort takes the same decisions, hence the same order
    HostClock hc(c, "host_select_sv");
    std::vector<int32_t> W(m);
    for (size_t i = 0; i < m; ++i) W[i] = (int32_t)i;
    std::sort(W.begin(), W.end(), [&](int32_t a, int32_t b) { return E[(size_t)a].w > E[(size_t)b].w; });
    // rank / sign of every node in its component order
    std::vector<int> comp(N.size(), -1), rank(N.size(), -1), sign(N.size(), 1);
    par(c, c->ord_off.size() - 1, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; ++k)
            for (int j = c->ord_off[k]; j < c->ord_off[k + 1]; ++j) {
                int nd = std::abs(c->ord_nodes[j]) - 1;
                comp[nd] = (int)k; rank[nd] = j - c->ord_off[k]; sign[nd] = c->ord_nodes[j] < 0 ? -1 : 1;
            }
    });
    for (auto& col : c->sv_cols) col.clear();
    c->sv_s1.clear(); c->sv_s2.clear();
    for (const int32_t wi : W) {
        const Edge& e = E[(size_t)wi];
        const Node &a = N[e.a], &b = N[e.b];
        bool conc = a.chr == b.chr && e.ha == 0 && e.hb == 1 && (b.pos - a.pos - a.len <= c->P.concord_dist_pos || e.b - e.a <= c->P.concord_dist_idx);
        if (conc) continue;
        bool ok = false;
        if (comp[e.a] == comp[e.b] && rank[e.a] < rank[e.b] && (bool)e.ha == (sign[e.a] < 0) && (bool)e.hb == (sign[e.b] > 0)) ok = true;
        else if (comp[e.a] == comp[e.b] && rank[e.a] > rank[e.b] && (bool)e.hb == (sign[e.b] < 0) && (bool)e.ha == (sign[e.a] > 0)) ok = true;
        if (!ok) continue;
        for (int32_t k = v.eoff[(size_t)wi]; k < v.eoff[(size_t)wi + 1]; ++k) {
            int b1 = v.ebp[(size_t)k].first.second, b2 = v.ebp[(size_t)k].second.second;
            c->sv_cols[0].push_back(a.chr); c->sv_cols[1].push_back(e.ha ? b1 : a.pos); c->sv_cols[2].push_back(e.ha ? a.pos + a.len : b1);
            c->sv_cols[3].push_back(b.chr); c->sv_cols[4].push_back(e.hb ? b2 : b.pos); c->sv_cols[5].push_back(e.hb ? b.pos + b.len : b2);
            c->sv_cols[6].push_back(e.w); c->sv_cols[7].push_back(sup1[(size_t)k]); c->sv_cols[8].push_back(sup2[(size_t)k]);
            c->sv_s1.push_back(e.ha); c->sv_s2.push_back(e.hb);
        }
    }
    c->svb.reset();
}

int call_sv(sq_ctx* c) {
    HostClock wall(c, "wall_call_sv");
    if (!c->ordered) return fail(c, SQ_E_ARG, "sq_call_sv before sq_order");
    if (!c->svb) c->svb = std::make_shared<SvBuild>();
    SvBuild& v = *c->svb;
    std::vector<int32_t> cov;
    int rc;
    if (v.stage == 0) {
        if ((rc = sv_breakpoints(c, v))) return rc;
        rc = sv_support(c, v, cov);
    } else rc = sv_cursors(c, v, cov);  // (back from the exchange of the difference arrays)
    if (rc) return rc;
    sv_select(c, v, cov);
    return SQ_OK;
}

}  // namespace sq
