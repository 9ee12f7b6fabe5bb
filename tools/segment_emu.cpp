// BuildNode_STAR's segmentation automaton of the device route (squid_amd/csrc/sq_segment_stage.inc, what sq_segment_on_device switches on) on
// the CPU: the kernel source itself (sq_wave.h with SQ_WAVE_EMU: every stretch's wave runs as 64 coroutines, the stretches from the last to
// the first), then the library's own walk over the stretch reports (segment_walk: a stretch whose report does not hold behind the real last
// node, or that hit a capacity, is run again with replay_range), against the host automaton in one go (segment_seeds_debug route 0; linked
// against libsquid_hip.so, no device needed).  Compared: the seeds (chr, pos, len) in order and the nodes extended, by place.
//   segment_emu --fuzz <cases> <seed> [--write <file>]     random tables (see make_case); --write keeps the cases as numbers for the device
//                                                          test (sq_debug_segment_seeds_tables)
// The stream-sized inputs come from GPU scans in production; here they are made from the tables by their definitions (derive): the trigger
// of a cluster is the first record beyond it, a zero-coverage record is the test of SegmentGraph.cpp:616-620 on the running pair, the
// ConcordRest candidates of a cluster are blocks on its chromosome that start at or behind its start minus a read length.
#include "../squid_amd/csrc/sq_internal.h"
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
static void seg_trace(int kind, int value);
static void seg_trace_windows(const void* recs, int co, int po, int wend);
#define SGS_TRACE(kind, value) do { if (wv::lane() == 0) seg_trace((kind), (value)); } while (0)
#define SGS_TRACE_WINDOWS(S) do { if (wv::lane() == 0) seg_trace_windows((S).R, (S).co, (S).po, (S).wend); } while (0)
#include "../squid_amd/csrc/sq_segment_stage.inc"
using namespace sq;

namespace {
struct Trace {
    long m2 = 0, m63 = 0, m64 = 0, m65 = 0, mcap = 0, mover = 0, w0 = 0, w1 = 0, w64 = 0, w65 = 0, big = 0, split = 0, dense_fired = 0, dense_split = 0, rest_fail = 0, chr_mark = 0, chr_walk = 0, clip_fwd = 0,
         clip_rev = 0;
} T_;
}  // namespace
static void seg_trace(int kind, int v) {
    switch (kind) {
    case sgs::T_MARGIN: T_.m2 += v == 2; T_.m63 += v == 63; T_.m64 += v == 64; T_.m65 += v == 65; T_.mcap += v == sgs::M_CAP; T_.mover += v == sgs::M_CAP + 1; break;
    case sgs::T_SUB: T_.split += v == 1; break;
    case sgs::T_DENSE: if (v) ++T_.dense_split; else ++T_.dense_fired; break;
    case sgs::T_REST_FAIL: ++T_.rest_fail; break;
    case sgs::T_CHR_CHANGE: if (v) ++T_.chr_walk; else ++T_.chr_mark; break;
    case sgs::T_CLIP: if (v) ++T_.clip_rev; else ++T_.clip_fwd; break;
    case sgs::T_BLOCKS: T_.big += v > 64; break;
    }
}
static void seg_trace_windows(const void* recs, int co, int po, int wend) {
    const sgs::Rec* R = (const sgs::Rec*)recs;
    int nc = 0, np = 0;
    for (int q = co; q < wend; ++q) nc += (R[q].flags & sgs::W_MASK) == sgs::W_C;
    for (int q = po; q < wend; ++q) np += (R[q].flags & sgs::W_MASK) == sgs::W_P;
    for (int n : {nc, np}) { T_.w0 += n == 0; T_.w1 += n == 1; T_.w64 += n == 64; T_.w65 += n == 65; }
}

namespace {
struct WaveArg { const sgs::Tab* X; uint32_t* M; int32_t *nodes, *report; int a; };
void w_run(void* p) { const WaveArg& a = *(const WaveArg*)p; sgs::run_stretch(*a.X, a.M, a.nodes, a.report, a.a); }

// dev_segment_run, wave by wave
void emulate(const SegDevTables& T, SegDevOut& D) {
    D.report.assign((size_t)T.na * sgs::REPORT, -7); D.nodes3.assign(3 * (size_t)T.node_slots + 3, INT32_MIN);
    sgs::Tab X;
    X.recs = T.recs; X.RL = T.RL; X.nd = T.nd; X.ncl = T.ncl; X.npart = T.npart; X.na = T.na; X.K_eff = T.K_eff;
    X.d4 = T.d4.data(); X.part2 = T.part2.data(); X.cl4 = T.cl4.data(); X.rest_off = T.rest_off.data(); X.rest_pos = T.rest_pos.data(); X.rest_len = T.rest_len.data(); X.trigger = T.trigger.data();
    X.stretch = T.stretch.data();
    std::vector<uint32_t> M((size_t)sgs::M_CAP);
    WaveArg a{&X, M.data(), D.nodes3.data(), D.report.data(), 0};
    for (int k = T.na; k-- > 0;) { std::fill(M.begin(), M.end(), 0xdeadbeefu); a.a = k; wv::run_wave(w_run, &a); }
    D.nodes3.resize(3 * (size_t)T.node_slots);
}

struct Case {
    int RL = 100;
    std::vector<StreamRec> recs;
    std::vector<int32_t> disc4, part2, cl4, rest_off, rest_pos, rest_len, trigger, zero3;
    std::vector<std::array<int, 3>> rest_req;  // chr, pos, len
    long planted_over = 0, near_gap = 0;
};
// trigger, zero-coverage records, ConcordRest CSR from the tables, by their definitions
void derive(Case& cs) {
    const int RL = cs.RL, nd = (int)cs.disc4.size() / 4;
    segment_clusters_of_tables(RL, nd, cs.disc4.data(), cs.cl4);
    const int ncl = (int)cs.cl4.size() / 4, K = (int)cs.recs.size();
    auto chr = [&](int k) { return cs.cl4[4 * k + 2]; };
    auto right = [&](int k) { return cs.cl4[4 * k + 3]; };
    auto start = [&](int k) { return cs.disc4[4 * cs.cl4[4 * k] + 1]; };
    cs.trigger.assign((size_t)ncl, K);
    {
        int i = 0;
        for (int k = 0; k < ncl; ++k) {
            while (i < K && !(chr(k) < cs.recs[i].refid || (chr(k) == cs.recs[i].refid && right(k) < cs.recs[i].pos))) ++i;
            cs.trigger[k] = i;
        }
    }
    cs.zero3.clear();
    int kc = 0, disChr = 0, disright = 0, oChr = 0, oRight = 0;
    for (int i = 0; i < K; ++i) {
        const StreamRec& r = cs.recs[i];
        if (kc == ncl) break;  // (:338-339: the reference has left its loop)
        while (kc < ncl && (chr(kc) < r.refid || (chr(kc) == r.refid && right(kc) < r.pos))) { disChr = chr(kc); disright = right(kc); ++kc; }
        const int dnChr = kc < ncl ? chr(kc) : 0, dnPos = kc < ncl ? start(kc) : 0;
        const bool disLead = disChr > oChr || (disChr == oChr && disright > oRight);
        const int curRight = disLead ? disright : oRight, curChr = std::max(disChr, oChr);
        if ((r.refid != curChr || r.pos > curRight + RL) && (curChr < dnChr || (curChr == dnChr && curRight + RL < dnPos))) { cs.zero3.push_back(i); cs.zero3.push_back(oChr); cs.zero3.push_back(oRight); }
        if ((r.flags & SR_CONC) && (r.flags & SR_MATE)) {
            const int e = r.fb_refpos + r.fb_matchref;
            if (oChr == r.refid) oRight = std::max(oRight, e); else { oRight = e; oChr = r.refid; }
        }
    }
    std::vector<std::vector<std::pair<int, int>>> per((size_t)ncl);
    for (const auto& q : cs.rest_req)
        for (int k = 0; k < ncl; ++k) if (chr(k) == q[0] && q[1] >= start(k) - RL && q[1] <= right(k)) { per[(size_t)k].push_back({q[1], q[2]}); break; }
    cs.rest_off.assign(1, 0); cs.rest_pos.clear(); cs.rest_len.clear();
    for (int k = 0; k < ncl; ++k) {
        std::sort(per[(size_t)k].begin(), per[(size_t)k].end());
        for (const auto& q : per[(size_t)k]) { cs.rest_pos.push_back(q.first); cs.rest_len.push_back(q.second); }
        cs.rest_off.push_back((int32_t)cs.rest_pos.size());
    }
}

// A case is a walk along 1-4 chromosomes: islands of concordant records (plain and clipped, both strands) with a discordant cluster in or
// next to them, and gaps between the islands that are wide (zero coverage: a new stretch), just wider than a read (at read length 50 the
// next stretch's first break candidate is then within thresh * 20 of the last node) or none.  `feature` plants what the summary counts.
Case make_case(std::mt19937_64& rng, int index) {
    Case cs;
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int feature = index % 12;
    cs.RL = feature == 5 || feature == 6 ? 50 : (rnd(0, 2) == 0 ? 50 : rnd(0, 1) ? 76 : 100);
    const int RL = cs.RL;
    std::vector<std::array<int, 4>> blocks;          // chr, pos, len, rev
    std::vector<std::pair<int, int>> parts;
    auto rec = [&](int chr, int pos, int len, int readpos, bool part, bool rev, bool mate, int shift) {
        StreamRec r{};
        r.refid = chr; r.pos = pos; r.fb_refpos = pos + shift; r.fb_matchref = len; r.fb_readpos = (uint16_t)readpos;
        r.flags = (uint8_t)(SR_HASBLK | SR_CONC | (part ? SR_PART : 0) | (rev ? SR_REV : 0) | (mate ? SR_MATE : 0));
        cs.recs.push_back(r);
    };
    auto plain = [&](int chr, int pos) { rec(chr, pos, RL, 0, false, rnd(0, 1) != 0, rnd(0, 3) != 0, 0); };
    auto clipped = [&](int chr, int pos) { const bool lead = rnd(0, 1) != 0; const int cut = rnd(16, 25); rec(chr, pos, RL - cut, lead ? cut : 0, true, rnd(0, 1) != 0, rnd(0, 3) != 0, 0); };
    auto blk = [&](int chr, int pos, int len, bool rev) { blocks.push_back({chr, pos, len, rev ? 1 : 0}); };
    auto stack = [&](int chr, int pos, int len, int n) { for (int i = 0; i < n; ++i) blk(chr, pos, len, i % 2 != 0); };
    auto chain = [&](int chr, int pos, int n, int step, int len) { for (int i = 0; i < n; ++i) blk(chr, pos + step * i, len, rnd(0, 1) != 0); return pos + step * (n - 1) + len; };
    const int nchr = feature == 9 ? 3 : rnd(1, 4);
    if (feature == 6) {  // a sens hit: the last node of chromosome 0 ends at 5000; on chromosome 1 a pending node start at 5000 meets the zero-coverage rule
        for (int i = 0; i < 3; ++i) plain(0, 4700 + 10 * i);
        chain(0, 4900, 8, 5, 65);  // dense: one node 4900..5000
        plain(0, 5400);
        plain(1, 5000);
        cs.recs.back().fb_matchref = 50;
        cs.recs.back().flags |= SR_MATE;
        stack(1, 5005, 50, 4);
        plain(1, 9000);
        stack(1, 20000, 30, 2);
        plain(1, 30000);
        // the same on chromosome 2 at a place no node ends at: the value is reported and the stretch kept
        plain(2, 7000);
        cs.recs.back().fb_matchref = 50;
        cs.recs.back().flags |= SR_MATE;
        stack(2, 7005, 50, 4);
        plain(2, 11000);
        stack(2, 20000, 30, 2);
        plain(2, 30000);
    }
    int p5 = 0;
    if (feature == 5) {  // read length 50: a node ends at X, behind a gap of zero coverage the next stretch's first candidate lies 52..58 behind X
        for (int i = 0; i < 3; ++i) plain(0, 1000 + 7 * i);
        const int X = chain(0, 1030, 8, 5, 40), q = X + rnd(52, 58);
        plain(0, q + 1);  // more than a read behind X, with the next cluster more than a read behind X too: zero coverage
        stack(0, q, 30, 5);
        plain(0, q + 400);
        p5 = q + 900;
        ++cs.near_gap;
    }
    if (feature == 9) {  // a record on chromosome 1 passes the last cluster of chromosome 0, which leaves a node start pending, and a cluster of its own (:361)
        plain(0, 1000);
        stack(0, 1010, 40, 5);
        stack(1, 500, 40, 5);
        plain(1, 2000);
    }
    for (int chr = feature == 9 ? 2 : 0; chr < nchr && feature != 0 && feature != 6; ++chr) {
        int p = feature == 5 && chr == 0 ? p5 : rnd(100, 3000);
        const int islands = feature == 2 || feature == 3 ? 2 : rnd(1, 6);
        for (int is = 0; is < islands; ++is) {
            int kind = rnd(0, 9);
            int npre = rnd(0, 9) < 6 ? rnd(0, 6) : rnd(7, 30);
            bool allow_part = true;
            if (feature == 1 && is < 3) { kind = 10 + is; allow_part = false; npre = rnd(0, 3); }
            if (feature == 2 && is == 0 && chr == 0) { kind = 13; allow_part = false; npre = 2; }
            if (feature == 3 && is == 0 && chr == 0) { kind = 14; allow_part = false; npre = 2; }
            if (feature == 4 && is < 3) { npre = is == 0 ? 64 : is == 1 ? 65 : 1; allow_part = false; }
            if (feature == 8 && is < 2) { npre = 1; kind = 0; allow_part = false; }
            if (feature == 7 && is == 0) { kind = 15; npre = 2; allow_part = false; }
            const bool exact = kind >= 10 && kind <= 14;  // a margin list of a planted size: no clip position of a neighbour may reach it
            if (exact) p += 3 * RL;
            const int first = p;
            for (int i = 0; i < npre; ++i) {
                if (allow_part && rnd(0, 5) == 0) clipped(chr, p); else if (rnd(0, 30) == 0) rec(chr, p, 20, 0, false, true, true, rnd(10, 60)); else plain(chr, p);
                p += npre > 40 ? rnd(0, 1) : rnd(0, RL / 3);
            }
            // the cluster: inside the island's cover, or behind it
            int q = npre ? std::max(first + rnd(3, RL - 5), p - rnd(0, RL - 10)) : p;
            if (feature == 8 && is < 2) q = p + 2 * RL + rnd(10, 50);  // an isolated cluster between two isolated records: a stretch of one record
            int right = q;
            switch (kind) {
            case 0: case 1: blk(chr, q, rnd(15, RL), rnd(0, 1) != 0); right = q + RL; break;                 // a single block: nothing comes of it
            case 2: case 3: stack(chr, q, rnd(20, RL), rnd(4, 7)); right = q + RL; break;                    // equal starts and ends: strong candidates
            case 4: right = chain(chr, q, rnd(6, 12), rnd(1, 6), rnd(30, RL)); break;                        // a dense run
            case 5: stack(chr, q, 30, rnd(4, 6)); stack(chr, q + 30 + rnd(4, RL - 2), 30, rnd(1, 5)); right = q + 2 * RL + 30; break;  // split into sub-clusters
            case 6: stack(chr, q, 40, 4); stack(chr, q + 100 + rnd(0, 40), 40, 5); stack(chr, q + 41, 20, 2); right = q + 300; break;
            case 7: right = chain(chr, q, rnd(66, 90), rnd(0, 2), rnd(30, 60)); break;                       // more than 64 blocks
            case 8: stack(chr, q, 35, 5); for (int i = 0; i < 4; ++i) parts.push_back({chr, q + rnd(-2, 2)}); right = q + 40; break;
            case 9: stack(chr, q, rnd(25, 45), 5); blk(chr, q + rnd(1, 2), 80, false); right = q + 90; break;
            case 10: right = chain(chr, q, 31, 2, 40); parts.push_back({chr, q + 5}); break;                   // 63 entries
            case 11: right = chain(chr, q, 32, 2, 40); break;                                                  // 64
            case 12: right = chain(chr, q, 32, 2, 40); parts.push_back({chr, q + 5}); break;                   // 65
            case 13: right = chain(chr, q, sgs::M_CAP / 2, 2, 40); break;                                      // the cap
            case 14: right = chain(chr, q, sgs::M_CAP / 2, 2, 40); parts.push_back({chr, q + 5}); ++cs.planted_over; break;  // one more
            case 15: stack(chr, q, 40, 4); for (int i = 0; i < rnd(6, 9); ++i) cs.rest_req.push_back({chr, q - rnd(10, 30), rnd(60, 90)}); right = q + 40; break;  // deep ConcordRest cover
            }
            if (rnd(0, 3) == 0) for (int i = 0; i < rnd(1, 6); ++i) cs.rest_req.push_back({chr, q - rnd(0, RL), rnd(20, 2 * RL)});
            if (!exact && rnd(0, 2) == 0) for (int i = 0; i < rnd(1, 3); ++i) parts.push_back({chr, q + rnd(-RL, RL)});
            // records over and behind the cluster
            p = std::max(p, q);
            const int npost = feature == 8 && is < 2 ? 0 : rnd(0, 4);
            for (int i = 0; i < npost; ++i) { p += rnd(1, RL / 2); if (allow_part && rnd(0, 3) == 0) clipped(chr, p); else plain(chr, p); }
            p = std::max(p, right);
            const int gap = rnd(0, 9);
            p += gap < 5 || exact ? 3 * RL + rnd(20, 900) : gap < 7 ? RL + rnd(1, 9) : rnd(0, RL - 1);
            if (feature == 8 && is < 2) { plain(chr, p + RL + 5); p += 3 * RL + 50; }
        }
        if (feature != 9 || chr == nchr - 1) if (rnd(0, 3) != 0) { plain(chr, p + rnd(0, 50)); }  // a closing record
    }
    if (feature == 10) {  // clusters no record ever passes
        const int chr = nchr - 1, p = (cs.recs.empty() ? 1000 : cs.recs.back().pos) + 5000;
        stack(chr, p, 40, 5); stack(chr, p + 2000, 40, 3);
    }
    if (feature == 11 && !cs.recs.empty()) {  // the stream ends on a record that opens nothing: the last stretch has no closing record
        const StreamRec last = cs.recs.back();
        stack(last.refid, last.pos + 10, 40, 5);
        plain(last.refid, last.pos + 20); plain(last.refid, last.pos + 60 + RL);
    }
    std::stable_sort(cs.recs.begin(), cs.recs.end(), [](const StreamRec& a, const StreamRec& b) { return a.refid != b.refid ? a.refid < b.refid : a.pos < b.pos; });
    std::stable_sort(blocks.begin(), blocks.end(), [](const std::array<int, 4>& a, const std::array<int, 4>& b) { return a[0] != b[0] ? a[0] < b[0] : a[1] < b[1]; });
    std::sort(parts.begin(), parts.end());
    for (const auto& b : blocks) for (int v : b) cs.disc4.push_back(v);
    for (const auto& q : parts) { cs.part2.push_back(q.first); cs.part2.push_back(q.second); }
    derive(cs);
    return cs;
}
void write_case(std::FILE* f, const Case& cs, const SegSeedsDebug& h, long flagged) {
    std::fprintf(f, "case %d %zu %zu %zu %zu %zu %zu %ld %zu\n", cs.RL, cs.recs.size(), cs.disc4.size() / 4, cs.part2.size() / 2, cs.trigger.size(), cs.rest_pos.size(), cs.zero3.size() / 3, flagged, h.seeds3.size() / 3);
    for (const StreamRec& r : cs.recs) std::fprintf(f, "%d %d %d %d %d %d\n", r.refid, r.pos, r.fb_refpos, r.fb_matchref, (int)r.fb_readpos, (int)r.flags);
    auto line = [&](const std::vector<int32_t>& v) { for (int32_t x : v) std::fprintf(f, "%d ", x); std::fprintf(f, "\n"); };
    line(cs.disc4); line(cs.part2); line(cs.rest_off); line(cs.rest_pos); line(cs.rest_len); line(cs.trigger); line(cs.zero3);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 4 || std::strcmp(argv[1], "--fuzz")) { std::fprintf(stderr, "usage: segment_emu --fuzz <cases> <seed> [--write <file>]\n"); return 2; }
    sq_ctx c;
    sq_default_params(&c.P);
    c.pool.reset(new HostPool(3));
    c.ref_len.assign(8, 1 << 28);
    const int cases = std::atoi(argv[2]);
    std::mt19937_64 rng((uint64_t)std::strtoull(argv[3], nullptr, 10));
    std::FILE* out = argc > 5 && !std::strcmp(argv[4], "--write") ? std::fopen(argv[5], "w") : nullptr;
    long bad = 0, records = 0, blocks = 0, clusters = 0, seeds = 0, stretches = 0, again = 0, kept_nodes = 0, longest = 0, sens = 0, sens_hits = 0, ext[3] = {0, 0, 0}, flagged = 0, planted = 0, single = 0, ends_inside = 0,
         never = 0, no_block = 0, near_again = 0, leading = 0;
    for (int k = 0; k < cases; ++k) {
        Case cs = make_case(rng, k);
        SegTablesIn in;
        in.read_len = cs.RL; in.n_recs = (int64_t)cs.recs.size(); in.recs = cs.recs.data(); in.n_disc = (int32_t)cs.disc4.size() / 4; in.disc4 = cs.disc4.data(); in.n_part = (int32_t)cs.part2.size() / 2;
        in.part2 = cs.part2.data(); in.rest_off = cs.rest_off.data(); in.rest_pos = cs.rest_pos.data(); in.rest_len = cs.rest_len.data(); in.trigger = cs.trigger.data(); in.n_zero = (int32_t)cs.zero3.size() / 3;
        in.zero3 = cs.zero3.data();
        std::shared_ptr<SegPlan> plan;
        SegSeedsDebug h, e;
        c.read_len = cs.RL;
        if (segment_plan_from_tables(&c, in, plan)) { std::printf("case %d: tables: %s\n", k, c.err.c_str()); ++bad; continue; }
        if (segment_seeds_debug(&c, *plan, cs.RL, 0, nullptr, h)) { std::printf("case %d: host automaton: %s\n", k, c.err.c_str()); ++bad; continue; }
        const SegDevTables* T = segment_device_tables(&c, *plan);
        if (!T) { std::printf("case %d: the tables do not fit the route\n", k); ++bad; continue; }
        SegDevOut D;
        const Trace before = T_;
        if (T->na) emulate(*T, D);
        if (segment_seeds_debug(&c, *plan, cs.RL, 1, &D, e)) { std::printf("case %d: walk: %s\n", k, c.err.c_str()); ++bad; continue; }
        long d = 0;
        if (e.seeds3 != h.seeds3) { ++d; std::printf("case %d: seeds differ (host %zu, emulated %zu)\n", k, h.seeds3.size() / 3, e.seeds3.size() / 3);
            for (size_t i = 0, shown = 0; i < std::max(h.seeds3.size(), e.seeds3.size()) / 3 && shown < 4; ++i) {
                const bool hh = 3 * i + 2 < h.seeds3.size(), ee = 3 * i + 2 < e.seeds3.size();
                if (hh && ee && !std::memcmp(&h.seeds3[3 * i], &e.seeds3[3 * i], 12)) continue;
                std::printf("   seed %zu: host (%d %d %d), emulated (%d %d %d)\n", i, hh ? h.seeds3[3 * i] : -9, hh ? h.seeds3[3 * i + 1] : -9, hh ? h.seeds3[3 * i + 2] : -9, ee ? e.seeds3[3 * i] : -9, ee ? e.seeds3[3 * i + 1] : -9,
                            ee ? e.seeds3[3 * i + 2] : -9);
                ++shown;
            } }
        for (int q = 0; q < 3; ++q) if (e.walk.ext[q] != h.walk.ext[q]) { ++d; std::printf("case %d: nodes extended at place %d differ (host %lld, emulated %lld)\n", k, q, (long long)h.walk.ext[q], (long long)e.walk.ext[q]); }
        const long over = T_.mover - before.mover;
        if (over != cs.planted_over || e.walk.flagged_margins != cs.planted_over) { ++d; std::printf("case %d: planted %ld margin lists over the cap, seen %ld, flagged stretches %lld\n", k, cs.planted_over, over, (long long)e.walk.flagged_margins); }
        if (e.walk.flagged != e.walk.flagged_margins) { ++d; std::printf("case %d: a stretch hit a capacity nobody planted\n", k); }
        bad += d;
        if (out) write_case(out, cs, h, (long)e.walk.flagged);
        const int K = (int)cs.recs.size(), ncl = (int)cs.trigger.size();
        records += K; blocks += in.n_disc; clusters += ncl; seeds += (long)h.seeds3.size() / 3; stretches += (long)e.walk.stretches; again += (long)e.walk.again; kept_nodes += (long)e.walk.kept_with_nodes;
        longest = std::max(longest, (long)e.walk.longest); sens += (long)e.walk.sens; sens_hits += (long)e.walk.sens_hits; flagged += (long)e.walk.flagged; planted += cs.planted_over; leading += (long)e.walk.leading_kept;
        for (int q = 0; q < 3; ++q) ext[q] += (long)h.walk.ext[q];
        no_block += in.n_disc == 0;
        for (int q = 0; q < ncl; ++q) never += cs.trigger[(size_t)q] >= K;
        for (int a = 0; a < T->na; ++a) { const int32_t* r = T->stretch.data() + (size_t)a * sgs::STRETCH; single += r[sgs::S_HI] - r[sgs::S_LO] == 1; ends_inside += r[sgs::S_HI] == K; }
        if (cs.near_gap) near_again += (long)e.walk.again;
    }
    if (out) std::fclose(out);
    std::printf("%d cases, %ld records, %ld blocks, %ld clusters, seeds %ld, stretches %ld, run again %ld, kept with a node %ld, kept with no node in front %ld, longest stretch %ld, sens values %ld, sens hits %ld, "
                "nodes extended %ld %ld %ld, margin lists of 2 63 64 65 cap cap+1 entries %ld %ld %ld %ld %ld %ld, flagged stretches %ld (planted %ld), windows of 0 1 64 65 live elements %ld %ld %ld %ld, "
                "clusters of more than 64 blocks %ld, clusters split %ld, single-record stretches %ld, stretches the stream ends in %ld, clusters never passed %ld, cases without a block %ld, "
                "run again across a gap at read length 50 %ld, chromosome changes %ld %ld, clipped reads forward %ld reverse %ld, ConcordRest turned a candidate down %ld, disCount rule fired %ld held back by a split %ld, "
                "%ld differences\n",
                cases, records, blocks, clusters, seeds, stretches, again, kept_nodes, leading, longest, sens, sens_hits, ext[0], ext[1], ext[2], T_.m2, T_.m63, T_.m64, T_.m65, T_.mcap, T_.mover, flagged, planted, T_.w0, T_.w1,
                T_.w64, T_.w65, T_.big, T_.split, single, ends_inside, never, no_block, near_again, T_.chr_mark, T_.chr_walk, T_.clip_fwd, T_.clip_rev, T_.rest_fail, T_.dense_fired, T_.dense_split, bad);
    std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
    return bad ? 1 : 0;
}
