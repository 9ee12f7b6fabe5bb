// `squid --bwa`: the single-file mode of the reference.  With BWA-MEM input there is no separate
// chimeric BAM: split reads are supplementary records of the one coordinate-sorted file, and the reference swaps three functions --
//   BuildNode_BWA             src/SegmentGraph.cpp:833-1205   (for BuildNode_STAR)
//   RawEdges                  src/SegmentGraph.cpp:1698-1930  (for RawEdgesChim + RawEdgesOther; it also REBUILDS Chimrecord from the
//                                                              partially aligned reads, :1883-1926)
//   the BAM loops' filters    MapQuality == 0 instead of < Min_MapQual (:871,1723), first mates only (:1723-1726)
// -- and shares everything from BuildEdges' sort on.  Division of labour here: the records are decoded WITH their QNAMEs (RawEdges
// sorts, merges and matches reads by name) -- by the GPU reader for files of 1 GiB and more (K-1 + K0 with sq_ctx::capture_names: the
// names kept next to the records on the device and copied back with them, round 5; 0.3-0.6 s for 50.8 M records where sixteen host
// threads took 3.3-4.5 s), on host threads otherwise --, the two order-dependent loops run on the host over that batch, and the graph from the edge reduction on takes the same kernels as the STAR
// path (filters, compression, components, ordering).  The breakpoint support (ExactBPConcordantSupport, mode-independent in the
// reference) is counted on the host, over the same batch.  With sq_bwa_on_device the batch is also made resident in HBM (DeviceRecords, the
// layout of the STAR path) and the two loops that are not automata run there: the node depth as a prefix maximum (sq_bwa_stage.inc) and
// the breakpoint support on the kernels of the STAR path (dev_breakpoint_support), behind a class byte per record.  Not the path
// BASELINE.json measures; built for drop-in completeness and held to the same parity bar (tests/test_bwa.py, tests/test_bwa_stage_gpu.py).
//
// Quirks of the reference reproduced (ledger W1-W6): capacity-driven window compaction, front() for [offset],
// the last Qname group never flushed, LocateRead hint left over from the BAM loop, weight -1 edges of multi-aligned second mates, the
// one-way depth cursor.
#include <algorithm>
#include <cstdint>
#include <chrono>
#include <cstring>

#include "sq_internal.h"
#include "sq_parsort.h"

namespace sq {

namespace {

struct RecRef {  // one record of the host batch, in the reference's vocabulary
    const HostBatch& hb; size_t i;
    int refid() const { return hb.refid[i]; }
    int pos() const { return hb.pos[i]; }
    int mrefid() const { return hb.mrefid[i]; }
    int mpos() const { return hb.mpos[i]; }
    int flag() const { return hb.flag[i]; }
    bool mapped() const { return !(flag() & 0x4); }
    bool mate_mapped() const { return !(flag() & 0x8); }
    bool rev() const { return flag() & 0x10; }
    bool mate_rev() const { return flag() & 0x20; }
    bool first() const { return flag() & 0x40; }
    bool proper() const { return flag() & 0x2; }
    bool dup() const { return flag() & 0x400; }
    bool multi() const { return hb.aux[i] & SQ_AUX_MULTI; }       // HasTag("XA") || IH > 1
    bool lowphred() const { return hb.aux[i] & SQ_AUX_LOWPHRED; } // of the record's own mate side
    int totlen() const { return hb.totlen[i]; }
    size_t nblk() const { return hb.blk_off[i + 1] - hb.blk_off[i]; }
    Blk blk(size_t k) const {
        const size_t b = hb.blk_off[i] + k;
        return Blk{refid(), hb.b_refpos[b], hb.b_readpos[b], hb.b_matchref[b], hb.b_matchread[b], rev(), first()};
    }
    std::string raw_name() const { return std::string(hb.names.data() + hb.name_off[i], hb.names.data() + hb.name_off[i + 1]); }
    std::string qname() const {  // ReadRec.cpp:11-13
        std::string q = raw_name();
        if (q.size() >= 2 && (q.compare(q.size() - 2, 2, "/1") == 0 || q.compare(q.size() - 2, 2, "/2") == 0)) q.resize(q.size() - 2);
        return q;
    }
    // the pair is "concordant" for the node builder (:1037-1040)
    bool pair_concordant() const {
        if (!(mapped() && mate_mapped() && mrefid() != -1 && refid() == mrefid() && proper())) return false;
        if (rev() && !mate_rev()) return pos() >= mpos() && pos() - mpos() <= 750000;
        if (!rev() && mate_rev()) return mpos() >= pos() && mpos() - pos() <= 750000;
        return false;
    }
};

// more than 15 bases of the read hang over at either end of its aligned blocks, and its qualities are fine (:1050-1065, :1730-1737)
inline bool clipped_end(const BlkList& r, int totlen, bool low) {
    if (r.empty() || low) return false;
    return r.front().readpos > 15 || totlen - r.back().readpos - r.back().matchread > 15;
}

// a sliding window of BuildNode_BWA: storage, front offset and the capacity the reference's compaction test looks at (W1)
struct Window {
    std::vector<Blk> v;
    int off = 0;
    size_t cap = 65536;
    bool none() const { return off == (int)v.size(); }
    const Blk& head() const { return v[(size_t)off]; }
    int end_of(size_t k) const { return v[k].refpos + v[k].matchref; }
    void drop_left_of(int refid, int pos, int read_len) { while (!none() && (head().refid != refid || head().refpos + head().matchref + read_len < pos)) ++off; }
    // chromosome of the oldest of the (at most four) newest elements, if there is one (:1002-1013)
    void vote_chr(int& chr) const { for (int i = (int)v.size() - 1; i >= off && (int)v.size() - i < 5; --i) chr = v[(size_t)i].refid; }
};

}  // namespace

// ---- BuildNode_BWA up to the seed nodes, plus the Reads list of :878-881
// The loop (:855-1114) is one automaton over all records, but everything it carries from record to record dies at a gap in the coverage:
// a record r that starts more than  Lmax + RL + 64  bases behind the start of the passing record in front of it (Lmax = the longest
// first block of the batch; or r opens a chromosome) finds -- after the work it triggers on the windows BEFORE it -- all three windows
// empty, the discordant run flushed, no pending mark, and every seed emitted so far more than 60 bases (thresh * 20, the only distance
// a seed is ever compared over) in front of anything it or its successors will look at.  So the stream is cut at such records: a
// stretch runs from its gap record with the state a fresh automaton has, and ends by letting the NEXT stretch's first record close it
// (the flush of the discordant window and the zero-coverage rule, :888-1026, without the record joining a window).  The one thing a
// fresh stretch does not reproduce is the fill of the windows' storage, which decides WHEN the capacity-driven compaction (W1) runs --
// not what the loop computes: the compaction only removes elements that end more than RL in front of the current record (and of the
// discordant run's head), which no later test can see: the clip-position and cover counts look at positions behind that head, emptiness
// and the voted chromosome do not change while an element that is NOT removable is still in front of them.
// SQUID_BWA_PIECE=<records> sets the stretch length (tests); samples of 200 k records and more are cut into 4 x threads stretches.
namespace {
struct SeedRun {
    int RL = 0, counted = 0, prev0 = 0, mark_start = -1, mark_chr = -1, dis_right = 0, other_right = 0;
    // what a stretch that was started on a guess must report (bwa_seed_nodes): were the two "rightmost" values assigned inside it, the
    // smallest position at which the zero-coverage test came out true by its position half while each was still the caller's, and the
    // outcome of that test for the record that closed the stretch
    bool dis_set = false, oth_set = false, closing_zero = true;
    int minpos_dis = INT32_MAX, minpos_oth = INT32_MAX;
    Window conc, dis, part;
    std::vector<Node> seeds;
    std::vector<Blk> reads;
    int64_t n_reads_records = 0;  // records that fed `reads`
    std::vector<int> margins;
    int64_t flush_nodes = 0, marks_closed = 0;  // flushes of the discordant window that emitted a node, marks the zero-coverage rule closed (sq_debug_bwa_seed_nodes)
    bool keep_reads = true;  // false: the Reads list is not wanted (the device route: the depth stage reads the table)
};
// what crosses a gap (bwa_seed_nodes)
struct Carry { int zero, prev0, mark_start, mark_chr, dis_right, other_right; };
inline bool seed_record_passes(const HostBatch& hb, size_t ri) {
    const RecRef r{hb, ri};
    return !(r.multi() || hb.mapq[ri] == 0 || r.dup() || !r.mapped() || r.refid() == -1) && r.nblk() != 0;
}
// one turn of the loop for record ri; `closing`: the record only closes the stretch in front of it (it belongs to the next one)
// opening_zero >= 0: the record's turn up to the zero-coverage rule was the closing turn of the stretch in front (which found `zero` = opening_zero)
void seed_step(SeedRun& S, const HostBatch& hb, size_t ri, bool closing, int opening_zero = -1) {
    const int thresh = 3;
    int &RL = S.RL, &prev0 = S.prev0, &mark_start = S.mark_start, &mark_chr = S.mark_chr, &dis_right = S.dis_right, &other_right = S.other_right;
    Window &conc = S.conc, &dis = S.dis, &part = S.part;
    std::vector<Node>& seeds = S.seeds;
    std::vector<int>& margins = S.margins;
    auto push_node = [&](int chr, int from, int to, int& cur_start, int& cur_end) {
        seeds.push_back(Node{chr, from, to - from, 0, 0.0});
        cur_start = to; cur_end = to; mark_start = to; mark_chr = chr;
    };
    const RecRef r{hb, ri};
    if (S.counted < 5 && !closing) { RL = std::max(RL, r.totlen()); ++S.counted; }  // :857-864 (over ALL records, in front of the filter)
    if (r.multi() || hb.mapq[ri] == 0 || r.dup() || !r.mapped() || r.refid() == -1) return;
    const bool opening = opening_zero >= 0;
    if (!opening && ((!dis.none() && r.refid() != dis.head().refid) || (!conc.none() && r.refid() != conc.head().refid) || (!part.none() && r.refid() != part.head().refid))) { other_right = 0; S.oth_set = true; }
    const size_t nb = r.nblk();
    if (nb == 0) return;
    if (!closing) { if (S.keep_reads) for (size_t k = 0; k < nb; ++k) S.reads.push_back(r.blk(k)); ++S.n_reads_records; }
    const Blk b0 = r.blk(0), blast = r.blk(nb - 1);
    if (!opening && conc.none() && part.none() && dis.none()) prev0 = r.pos();
    if (!opening && !dis.none() && (dis.v.back().refid != r.refid() || dis_right + RL < r.pos())) {
        // the discordant window is complete: decide the segment boundaries inside it (:888-998)
        int cur_end = 0, cur_start = std::max(prev0, mark_start);
        int d_start = -1, d_end = -1, d_count = -1;
        const size_t seeds_before = seeds.size();
        bool split = false;
        auto dense = [&]() { return d_start != -1 && !split && d_count > std::min(5.0, 4.0 * (d_end - d_start) / RL); };
        while (!dis.none()) {
            if (dense()) push_node(dis.head().refid, d_start, d_end, cur_start, cur_end);
            split = false;
            margins.clear();
            size_t i = (size_t)dis.off;
            for (; i < dis.v.size(); ++i) {  // the leading run of blocks that touch each other
                margins.push_back(dis.v[i].refpos); margins.push_back(dis.end_of(i));
                cur_end = std::max(cur_end, margins.back());
                if (i + 1 < dis.v.size() && dis.v[i + 1].refpos > dis.end_of(i)) break;
            }
            d_start = std::max(cur_start, dis.head().refpos);
            d_end = cur_end;
            d_count = (int)i - dis.off;
            for (++i; i < dis.v.size() && dis.v[i].refpos < cur_end + thresh; ++i) { margins.push_back(dis.v[i].refpos); margins.push_back(dis.end_of(i)); }
            const int m0 = margins.front(), dchr = dis.head().refid;
            for (size_t k = (size_t)part.off; k < part.v.size(); ++k) {  // clip positions of the partially aligned reads next to the run
                const Blk& p = part.v[k];
                if (p.refid != dchr) continue;
                const int pe = p.refpos + p.matchref;
                if (p.readpos > 15 && p.refpos > m0 - thresh && p.refpos < cur_end + thresh) margins.push_back(p.rev ? pe : p.refpos);
                else if (pe > m0 - thresh && pe < cur_end + thresh) margins.push_back(p.rev ? p.refpos : pe);
            }
            std::sort(margins.begin(), margins.end());
            int last_cursor = -1, last_support = 0;
            const int chr0 = dis.v.front().refid;  // (W2: element 0 of the storage, not the window's head)
            for (size_t at = 0; at < margins.size();) {
                const int x = margins[at];
                if (!seeds.empty() && seeds.back().chr == chr0 && x - seeds.back().pos - seeds.back().len < thresh * 20) { ++at; continue; }
                int sr = 0, left_fwd = 0, right_rev = 0;
                for (size_t q = 0; q < margins.size() && margins[q] < x + thresh; ++q) sr += std::abs(x - margins[q]) < thresh;
                for (size_t q = (size_t)dis.off; q < dis.v.size(); ++q) {
                    const int e = dis.end_of(q);
                    if (e < x && e > x - RL && !dis.v[q].rev) ++left_fwd;
                    else if (dis.v[q].refpos > x && dis.v[q].refpos < x + RL && dis.v[q].rev) ++right_rev;
                }
                bool cut_here = false;
                if (sr > 3 || sr + left_fwd > 4 || sr + right_rev > 4) {
                    int cover = 0;
                    for (size_t q = (size_t)conc.off; q < conc.v.size(); ++q) cover += conc.end_of(q) >= x + thresh && conc.v[q].refpos < x - thresh;
                    if (sr > std::max(cover - sr, 0) + 2) {
                        const int strength = sr + std::max(left_fwd, right_rev);
                        if (last_cursor == -1 && x - cur_start < thresh * 20) { mark_start = cur_start; mark_chr = chr0; }
                        else if ((last_cursor == -1 || x - last_cursor < thresh * 20) && strength > last_support) { last_cursor = x; last_support = strength; }
                        else if (x - last_cursor >= thresh * 20) { split = true; push_node(chr0, cur_start, last_cursor, cur_start, cur_end); cut_here = true; }
                    }
                }
                if (cut_here) break;
                size_t nx = at;
                while (nx < margins.size() && margins[nx] == x) ++nx;  // on to the next distinct position
                if (nx >= margins.size()) break;
                at = nx;
            }
            if (last_cursor != -1 && !split) { split = true; push_node(dis.head().refid, cur_start, last_cursor, cur_start, cur_end); }
            while (!dis.none() && dis.head().refpos + dis.head().matchref <= cur_end) ++dis.off;
        }
        if (dense()) push_node(dis.v[0].refid, d_start, d_end, cur_start, cur_end);  // (W2)
        if (dis.none()) { dis.v.clear(); dis.off = 0; }
        if (seeds.size() != seeds_before) ++S.flush_nodes;
        conc.drop_left_of(r.refid(), r.pos(), RL); part.drop_left_of(r.refid(), r.pos(), RL);
    }
    // zero coverage in front of this record (:1000-1026)
    const int rightmost = std::max(dis_right, other_right);
    int cur_chr = 0;
    conc.vote_chr(cur_chr); part.vote_chr(cur_chr); dis.vote_chr(cur_chr);
    const bool zero = opening ? opening_zero != 0 : (r.refid() != cur_chr || r.pos() > rightmost + RL);
    if (!opening && zero && r.refid() == cur_chr) {  // (true by its position half alone: a larger value handed in by the caller could have turned it)
        if (!S.dis_set) S.minpos_dis = std::min(S.minpos_dis, r.pos());
        if (!S.oth_set) S.minpos_oth = std::min(S.minpos_oth, r.pos());
    }
    if (closing) S.closing_zero = zero;
    if (!opening && zero && mark_start != -1) {
        ++S.marks_closed;
        if (rightmost > mark_start && rightmost - mark_start < thresh * 20 && !seeds.empty() && mark_start == seeds.back().pos + seeds.back().len) seeds.back().len += rightmost - mark_start;
        else if (rightmost > mark_start && rightmost - mark_start >= thresh * 20) seeds.push_back(Node{mark_chr, mark_start, rightmost - mark_start, 0, 0.0});
        mark_start = -1; mark_chr = -1;
    }
    if (closing) return;
    if (zero) prev0 = r.pos();
    if (dis.none()) { conc.drop_left_of(r.refid(), r.pos(), RL); part.drop_left_of(r.refid(), r.pos(), RL); }
    // the record joins a window (:1035-1086)
    const int e0 = b0.refpos + b0.matchref;
    if (r.pair_concordant()) {
        S.oth_set = true;  // (the first such record of a stretch finds both windows empty: assigned, not compared)
        other_right = (!conc.none() || !part.none()) ? std::max(other_right, e0) : e0;
        const bool clipped = !r.lowphred() && (b0.readpos > 15 || r.totlen() - blast.readpos - blast.matchread > 15);
        (clipped ? part : conc).v.push_back(b0);
    } else {
        S.dis_set = true;
        dis_right = !dis.v.empty() ? std::max(dis_right, e0) : e0;
        dis.v.push_back(b0);
    }
    // compaction at capacity (:1087-1112, W1)
    for (Window* w : {&conc, &part}) {
        if (w->v.size() != w->cap) continue;
        const int from = !dis.none() ? std::min(r.pos(), dis.head().refpos) : r.pos();
        std::vector<Blk> kept;
        for (size_t q = (size_t)w->off; q < w->v.size(); ++q) if (w->v[q].refid == r.refid() && w->end_of(q) + RL >= from) kept.push_back(w->v[q]);
        w->v.swap(kept); w->off = 0;
        if (w->v.size() == w->cap) w->cap *= 2;
    }
}
// one stretch [lo, hi) of the stream: from the state a fresh automaton has and the guesses (first: it opens the stream -- no guess), or from
// the real state; has_next: record hi closes it
void run_seed_stretch(SeedRun& S, const HostBatch& hb, size_t lo, size_t hi, bool has_next, bool first, int read_len, int RL_final, int dis_in, const Carry* real, bool keep_reads) {
    S = SeedRun();
    S.keep_reads = keep_reads;
    S.RL = first ? read_len : RL_final;
    S.counted = first ? 0 : 5;
    S.dis_right = dis_in;
    if (real) { S.prev0 = real->prev0; S.mark_start = real->mark_start; S.mark_chr = real->mark_chr; S.dis_right = real->dis_right; S.other_right = real->other_right; }
    if (keep_reads) {
        size_t nblk = 0;
        for (size_t ri = lo; ri < hi; ++ri) nblk += hb.blk_off[ri + 1] - hb.blk_off[ri];
        S.reads.reserve(nblk);  // (at most every block of the stretch: one allocation)
    }
    for (size_t ri = lo; ri < hi; ++ri) seed_step(S, hb, ri, false, (!first && ri == lo) ? (real ? real->zero : 1) : -1);
    if (has_next) seed_step(S, hb, hi, true);  // (the next stretch's gap record closes this one)
}
}  // namespace
// SQUID_BWA_PIECE=<records>: length of a stretch of the parallel --bwa loops (tests: short stretches and a short warm-up on small inputs); 0: by size
static long bwa_piece_env() { return (long)env_int("SQUID_BWA_PIECE", 0); }

static int bwa_seed_nodes(sq_ctx* c, const HostBatch& hb, std::vector<Node>& seeds, std::vector<std::vector<Blk>>& reads, int64_t& n_reads_records) {
    const size_t nrec = hb.size();
    // ReadLen as the loop leaves it (:857-864): the chimeric file's value, raised by the first five records
    int RL_final = c->read_len;
    for (size_t ri = 0; ri < nrec && ri < 5; ++ri) RL_final = std::max(RL_final, (int)hb.totlen[ri]);
    const long piece_env = bwa_piece_env();
    const int threads = c->pool ? c->pool->size() + 1 : 1;
    std::vector<size_t> cut{0};
    if (threads > 1 && nrec > 16 && (piece_env > 0 || nrec >= 200000)) {
        // even pieces; per piece the largest (RefID, end of the first block) of its passing records -- the records are sorted, so the
        // running maximum of that key in front of a record is "the farthest a window element of the current chromosome reaches" --,
        // then every piece looks for its first passing record that starts more than RL + 64 behind that reach (or on a later chromosome)
        const int np0 = (int)std::min<size_t>(piece_env > 0 ? std::max<size_t>(1, nrec / (size_t)piece_env) : (size_t)(4 * threads), nrec / 8);
        auto key_of = [&](size_t ri) { const uint32_t b = hb.blk_off[ri]; return ((long long)hb.refid[ri] << 32) | (uint32_t)(hb.b_refpos[b] + hb.b_matchref[b]); };
        auto lo_of = [&](int k) { return nrec * (size_t)k / (size_t)np0; };
        std::vector<long long> reach((size_t)np0 + 1, -1);
        c->pool->parallel_for(np0, 1 << 20, [&](int k) {
            long long m = -1;
            for (size_t ri = lo_of(k); ri < lo_of(k + 1); ++ri) if (seed_record_passes(hb, ri)) m = std::max(m, key_of(ri));
            reach[(size_t)k + 1] = m;
        });
        for (int k = 0; k < np0; ++k) reach[(size_t)k + 1] = std::max(reach[(size_t)k + 1], reach[(size_t)k]);  // reach[k]: of everything in front of piece k
        std::vector<size_t> found((size_t)np0, 0);
        c->pool->parallel_for(np0, 1 << 20, [&](int k) {
            if (k == 0 || reach[(size_t)k] < 0) return;  // (a stretch starts behind the first five records, and behind a passing record)
            long long run = reach[(size_t)k];
            for (size_t ri = std::max<size_t>(lo_of(k), 8); ri < lo_of(k + 1); ++ri) {
                if (!seed_record_passes(hb, ri)) continue;
                const int chr = (int)(run >> 32), end = (int)(uint32_t)run;
                if (hb.refid[ri] != chr || (long long)hb.pos[ri] > (long long)end + RL_final + 64) { found[(size_t)k] = ri; return; }
                run = std::max(run, key_of(ri));
            }
        });
        for (int k = 1; k < np0; ++k) if (found[(size_t)k] > cut.back()) cut.push_back(found[(size_t)k]);
    }
    cut.push_back(nrec);
    const int np = (int)cut.size() - 1;
    c->timer.add("bwa_seed_node_stretches", 0.0, 0.0, np);
    // A stretch is started on a GUESS of the values that do cross a gap: the outcome of the zero-coverage test for its first record (guess:
    // true -- then prev0 and the mark are reset by that record itself) and the two "rightmost" values the test compares with (the
    // discordant one: computed in advance, above; the other one: 0).
    // They are stale whenever they matter -- the end of the last discordant / concordant run in front, possibly on an EARLIER CHROMOSOME:
    // the reference compares positions of different chromosomes there (DiscordantRightmost outlives the chromosome, :1002-1013) -- and
    // neither depends on anything the test decides, so every stretch reports what it assigned, the stretches are then walked in order
    // with the real values, and a stretch whose guess was wrong where it counted is run again from the real state.
    // DiscordantRightmost is known in advance: it follows a rule of its own -- a discordant record assigns it (or raises it while the
    // discordant window holds something), and the window is emptied by the first record on another chromosome or more than RL behind it --
    // that a pass over (filter, pair type, end of the first block) reproduces, stretch by stretch, each from an empty window (a gap
    // record finds it empty or empties it).  A stretch without a discordant record hands on what it was given.
    std::vector<int> dis_in((size_t)np + 1, 0);
    if (np > 1) {
        std::vector<std::pair<bool, int>> sum((size_t)np, std::make_pair(false, 0));
        c->pool->parallel_for(np, 1 << 20, [&](int k) {
            bool nonempty = false, has = false;
            int dr = 0, last = -1, RL = k == 0 ? c->read_len : RL_final;
            for (size_t ri = cut[(size_t)k]; ri < cut[(size_t)k + 1]; ++ri) {
                if (k == 0 && ri < 5) RL = std::max(RL, (int)hb.totlen[ri]);
                if (!seed_record_passes(hb, ri)) continue;
                const RecRef r{hb, ri};
                if (nonempty && (last != r.refid() || dr + RL < r.pos())) nonempty = false;
                if (!r.pair_concordant()) { const Blk b0 = r.blk(0); const int e0 = b0.refpos + b0.matchref; dr = nonempty ? std::max(dr, e0) : e0; nonempty = true; last = r.refid(); has = true; }
            }
            sum[(size_t)k] = std::make_pair(has, dr);
        });
        for (int k = 0; k < np; ++k) dis_in[(size_t)k + 1] = sum[(size_t)k].first ? sum[(size_t)k].second : dis_in[(size_t)k];
    }
    std::vector<SeedRun> runs((size_t)np);
    const int read_len0 = c->read_len;
    auto work = [&](int k, const Carry* real) { run_seed_stretch(runs[(size_t)k], hb, cut[(size_t)k], cut[(size_t)k + 1], k + 1 < np, k == 0, read_len0, RL_final, dis_in[(size_t)k], real, true); };
    if (np > 1) c->pool->parallel_for(np, 1 << 20, [&](int k) { work(k, nullptr); }); else work(0, nullptr);
    int again = 0;
    for (int k = 1; k < np; ++k) {
        const SeedRun& P = runs[(size_t)k - 1];  // (final: run from the real state, or checked)
        const Carry real{P.closing_zero ? 1 : 0, P.prev0, P.mark_start, P.mark_chr, P.dis_right, P.other_right};
        SeedRun& S = runs[(size_t)k];
        // with `zero` true the first record resets prev0 and the mark by itself; the rightmost values only enter through the position half
        // of later tests, and only until the stretch assigns them (smaller than every position a test came out true at: same outcomes)
        const bool fine = real.zero && real.dis_right == dis_in[(size_t)k] &&
                          (real.other_right == 0 || S.minpos_oth == INT32_MAX || (long)real.other_right + RL_final < (long)S.minpos_oth);
        if (fine) {  // (what the stretch did not assign stays the caller's)
            if (!S.oth_set) S.other_right = real.other_right;
            continue;
        }
        if (env_set("SQUID_BWA_DEBUG")) std::fprintf(stderr, "stretch %d (%d, %d) again: zero %d, rightmost values %d / %d against first true tests at %d / %d\n", k, hb.refid[cut[(size_t)k]], hb.pos[cut[(size_t)k]], real.zero, real.dis_right, real.other_right, S.minpos_dis, S.minpos_oth);
        work(k, &real);
        ++again;
    }
    c->timer.add("bwa_seed_node_stretches_run_again", 0.0, 0.0, again);
    if (env_set("SQUID_BWA_DEBUG")) {
        for (int k = 0; k < np; ++k) {
            std::fprintf(stderr, "stretch %d: records [%zu, %zu) first (%d, %d); seeds:", k, cut[(size_t)k], cut[(size_t)k + 1], hb.refid[cut[(size_t)k]], hb.pos[cut[(size_t)k]]);
            for (const Node& n : runs[(size_t)k].seeds) std::fprintf(stderr, " (%d %d %d)", n.chr, n.pos, n.len);
            std::fprintf(stderr, "\n");
        }
    }
    reads.clear();
    n_reads_records = 0;
    for (SeedRun& S : runs) { seeds.insert(seeds.end(), S.seeds.begin(), S.seeds.end()); reads.push_back(std::move(S.reads)); n_reads_records += S.n_reads_records; }
    c->read_len = runs.back().RL;
    return SQ_OK;
}

// ---- the same loop by the kernels of sq_bwa_nodes.inc (sq_bwa_nodes_on_device): the device cuts the stream at every gap record and runs
// one wave per stretch on the same guesses; here the reports are walked in order with the real values, as above, and a stretch whose
// guess was wrong where it counted is run again with seed_step from the real state.  No Reads list is built (the depth stage reads the
// table).  fallback: the kernels raised a flag (or the table is not there) -- nothing was done
namespace {
void first_five(const sq_ctx* c, const HostBatch& hb, int32_t rl5[5]) {
    int rl = c->read_len;
    for (size_t i = 0; i < 5; ++i) { if (i < hb.size()) rl = std::max(rl, (int)hb.totlen[i]); rl5[i] = rl; }
}
}  // namespace
int bwa_seed_nodes_walk(sq_ctx* c, const HostBatch& hb, const int32_t rl5[5], const BwaNodesOut& D, std::vector<Node>& seeds, int64_t& n_reads_records, int& read_len_out, BwaNodesWalk& W) {
    const int RL_final = rl5[4];
    const int np = (int)D.cut.size() - 1;
    W = BwaNodesWalk();
    W.stretches = np;
    n_reads_records = 0;
    read_len_out = np > 0 ? c->read_len : RL_final;
    Carry last{1, 0, -1, -1, 0, 0};  // (what the stretch in front left behind: final)
    SeedRun again;
    for (int k = 0; k < np; ++k) {
        const int32_t* R = D.report.data() + (size_t)bwn::REPORT * (size_t)k;
        const size_t lo = (size_t)D.cut[(size_t)k], hi = (size_t)D.cut[(size_t)k + 1];
        W.single += hi - lo == 1; W.longest = std::max<int64_t>(W.longest, (int64_t)(hi - lo));
        bool fine = true;
        int other_right = R[bwn::R_OTHER_RIGHT];
        if (k > 0) {
            fine = last.zero && last.dis_right == D.dis_in[(size_t)k] &&
                   (last.other_right == 0 || R[bwn::R_MINPOS_OTH] == INT32_MAX || (long)last.other_right + RL_final < (long)R[bwn::R_MINPOS_OTH]);
            if (fine && !(R[bwn::R_BITS] & bwn::B_OTH_SET)) other_right = last.other_right;  // (what the stretch did not assign stays the caller's)
        }
        if (fine) {
            const int32_t* s3 = D.seeds3.data() + 3 * (size_t)R[bwn::R_SPARE];
            for (int i = 0; i < R[bwn::R_SEEDS]; ++i) seeds.push_back(Node{s3[3 * i], s3[3 * i + 1], s3[3 * i + 2], 0, 0.0});
            n_reads_records += R[bwn::R_READS];
            W.flush_nodes += R[bwn::R_FLUSH_NODES]; W.marks_closed += R[bwn::R_MARKS_CLOSED];
            read_len_out = R[bwn::R_RL];
            last = Carry{(R[bwn::R_BITS] & bwn::B_CLOSING_ZERO) ? 1 : 0, R[bwn::R_PREV0], R[bwn::R_MARK_START], R[bwn::R_MARK_CHR], R[bwn::R_DIS_RIGHT], other_right};
            continue;
        }
        if (env_set("SQUID_BWA_DEBUG")) std::fprintf(stderr, "device stretch %d (%d, %d) again: zero %d, rightmost values %d / %d against %d and first true tests at %d / %d\n", k, hb.refid[lo], hb.pos[lo], last.zero, last.dis_right, last.other_right, D.dis_in[(size_t)k], R[bwn::R_MINPOS_DIS], R[bwn::R_MINPOS_OTH]);
        run_seed_stretch(again, hb, lo, hi, k + 1 < np, k == 0, c->read_len, RL_final, D.dis_in[(size_t)k], &last, false);
        ++W.again;
        seeds.insert(seeds.end(), again.seeds.begin(), again.seeds.end());
        n_reads_records += again.n_reads_records;
        W.flush_nodes += again.flush_nodes; W.marks_closed += again.marks_closed;
        read_len_out = again.RL;
        last = Carry{again.closing_zero ? 1 : 0, again.prev0, again.mark_start, again.mark_chr, again.dis_right, again.other_right};
    }
    return SQ_OK;
}
namespace {
int bwa_seed_nodes_device(sq_ctx* c, const HostBatch& hb, std::vector<Node>& seeds, int64_t& n_reads_records, int& read_len_out, bool& fallback, BwaNodesWalk& W) {
    int32_t rl5[5];
    first_five(c, hb, rl5);
    BwaNodesOut D;
    const int rc = dev_bwa_seed_nodes(c, c->read_len, rl5, D);
    if (rc == SQ_E_CAPACITY) { fallback = true; return SQ_OK; }
    if (rc) return rc;
    fallback = D.fallback;
    if (fallback) { if (env_set("SQUID_BWA_DEBUG")) std::fprintf(stderr, "BuildNode_BWA on the device: back to the host automaton (%s)\n", D.why); return SQ_OK; }
    HostClock hc(c, "host_bwa_node_walk");
    return bwa_seed_nodes_walk(c, hb, rl5, D, seeds, n_reads_records, read_len_out, W);
}
// the Reads list of :878-881 alone, stretch by stretch (the depth stage fell back behind the device automaton)
void bwa_reads_list(sq_ctx* c, const HostBatch& hb, std::vector<std::vector<Blk>>& reads) {
    const size_t nrec = hb.size();
    const int np = c->pool && nrec > 100000 ? 8 * (c->pool->size() + 1) : 1;
    reads.assign((size_t)np, std::vector<Blk>());
    auto part = [&](int k) {
        std::vector<Blk>& v = reads[(size_t)k];
        for (size_t ri = nrec * (size_t)k / (size_t)np; ri < nrec * ((size_t)k + 1) / (size_t)np; ++ri) {
            if (!seed_record_passes(hb, ri)) continue;
            const RecRef r{hb, ri};
            for (size_t b = 0; b < r.nblk(); ++b) v.push_back(r.blk(b));
        }
    };
    if (np > 1) c->pool->parallel_for(np, 1 << 20, part); else part(0);
}
}  // namespace

// sq_debug_bwa_seed_nodes (see sq_internal.h)
int bwa_seed_nodes_debug(sq_ctx* c, const HostBatch* tables, int route, BwaNodesDebug& out) {
    if (!tables && !c->bwa) return fail(c, SQ_E_ARG, "sq_ingest_bwa_file first");
    const HostBatch& hb = tables ? *tables : *c->bwa;
    out = BwaNodesDebug();
    std::vector<Node> seeds;
    if (route == 0) {
        int32_t rl5[5];
        first_five(c, hb, rl5);
        SeedRun S;
        run_seed_stretch(S, hb, 0, hb.size(), false, true, c->read_len, rl5[4], 0, nullptr, false);
        seeds.swap(S.seeds);
        out.read_len = S.RL; out.n_reads_records = S.n_reads_records; out.stretches = 1; out.longest = (int64_t)hb.size(); out.single = hb.size() == 1;
        out.flush_nodes = S.flush_nodes; out.marks_closed = S.marks_closed;
    } else {
        if (!c->dev) return fail(c, SQ_E_ARG, "no device");
        if (tables || !c->bwa_resident) {
            const int rc = dev_bwa_upload(c, hb);
            if (rc && rc != SQ_E_CAPACITY) return rc;
            c->bwa_resident = rc == SQ_OK;
            c->bwa_dev_active = false;
        }
        BwaNodesWalk W;
        int rl = c->read_len;
        bool fallback = !c->bwa_resident;
        int rc = SQ_OK;
        if (!fallback) rc = bwa_seed_nodes_device(c, hb, seeds, out.n_reads_records, rl, fallback, W);
        if (tables) { dev_clear_records(c); c->bwa_resident = false; }
        if (rc) return rc;
        out.fallback = fallback; out.read_len = rl;
        out.stretches = W.stretches; out.again = W.again; out.single = W.single; out.longest = W.longest; out.flush_nodes = W.flush_nodes; out.marks_closed = W.marks_closed;
    }
    for (const Node& n : seeds) { out.seeds3.push_back(n.chr); out.seeds3.push_back(n.pos); out.seeds3.push_back(n.len); }
    return SQ_OK;
}

// Support / AvgDepth of the tiled nodes (:1180-1204): one pass, the cursor never goes back (W6).  The loop proper, into a count and a
// 32-bit sum per node; false: no read at all
static bool bwa_node_depth_sums(const std::vector<Node>& N, const std::vector<std::vector<Blk>>& parts, std::vector<int32_t>& cnts, std::vector<int32_t>& sums) {
    cnts.assign(N.size(), 0); sums.assign(N.size(), 0);
    size_t pi = 0, it = 0;
    auto skip_empty = [&]() { while (pi < parts.size() && it == parts[pi].size()) { ++pi; it = 0; } };
    skip_empty();
    if (pi == parts.size()) return false;
    for (size_t i = 0; i < N.size(); ++i) {
        const Node& n = N[i];
        int cnt = 0;
        uint32_t sum = 0;  // (the reference's int, with the wrap-around written out)
        for (; pi < parts.size(); ++it, skip_empty()) {
            const Blk& b = parts[pi][it];
            if (b.refid == n.chr && b.refpos >= n.pos && b.refpos + b.matchref <= n.pos + n.len) { ++cnt; sum += (uint32_t)b.matchref; }
            else if (b.refpos >= n.pos + n.len || b.refid != n.chr) break;
        }
        cnts[i] = cnt; sums[i] = (int32_t)sum;
    }
    return true;
}
void bwa_set_node_depths(std::vector<Node>& N, const std::vector<int32_t>& cnts, const std::vector<int32_t>& sums) {
    for (size_t i = 0; i < N.size(); ++i) {
        Node& n = N[i];
        n.support = cnts[i];
        n.depth = 1.0 * sums[i] / n.len;
        n.depth_lo = n.depth_hi = n.depth;
    }
}
static void bwa_node_depth(std::vector<Node>& N, const std::vector<std::vector<Blk>>& parts) {
    std::vector<int32_t> cnts, sums;
    if (!bwa_node_depth_sums(N, parts, cnts, sums)) return;  // (no read at all: the reference leaves Support / AvgDepth as constructed)
    bwa_set_node_depths(N, cnts, sums);
}
// the same loop on flat tables (sq_debug_bwa_depth route 0, tools/bwa_stage_emu.cpp): nodes3 = {chr, pos, len}, reads3 = {chr, refpos, matchref}
void bwa_node_depth_flat(int32_t n_nodes, const int32_t* nodes3, int64_t n_reads, const int32_t* reads3, std::vector<int32_t>& cnts, std::vector<int32_t>& sums) {
    std::vector<Node> N((size_t)n_nodes);
    for (int32_t i = 0; i < n_nodes; ++i) N[(size_t)i] = Node{nodes3[3 * i], nodes3[3 * i + 1], nodes3[3 * i + 2], 0, 0.0};
    std::vector<std::vector<Blk>> parts(1);
    parts[0].resize((size_t)n_reads);
    for (int64_t j = 0; j < n_reads; ++j) parts[0][(size_t)j] = Blk{reads3[3 * j], reads3[3 * j + 1], 0, reads3[3 * j + 2], 0, false, false};
    bwa_node_depth_sums(N, parts, cnts, sums);
}

static int bwa_home_node(const std::vector<Node>& N, int start, const Blk& b) {  // the two walks of :1757-1758 as binary searches
    const int n = (int)N.size();
    const int j0 = (int)(std::partition_point(N.begin(), N.end(), [&](const Node& x) { return x.chr < b.refid || (x.chr == b.refid && x.pos + x.len < b.refpos); }) - N.begin());
    const int i = std::max(start, j0);
    if (i >= n) return -2;
    const int j1 = (int)(std::partition_point(N.begin(), N.end(), [&](const Node& x) { return x.chr < b.refid || (x.chr == b.refid && x.pos <= b.refpos); }) - N.begin()) - 1;
    return std::min(i, j1);
}

// ---- RawEdges (:1698-1930): the edges of the BAM loop, the -1 edges of multi-aligned second mates, the fragments rebuilt from the
// partially aligned reads and their split edges.  Two halves that both routes share: the BAM loop (bwa_raw_edges_loop on the host,
// dev_bwa_raw_edges on the device: sq_bwa_edges.inc) and everything behind it (bwa_raw_edges_tail), with prepare / finish_prepare --
// the fragment of one record -- in front of both.
namespace {
// the fragment of record ri as the loop builds it up to its LocateRead call: 0 = the record is skipped or locates nothing,
// 1 = first mate (:1745-1806), 2 = multi-aligned second mate (:1807-1860); `part`: it also goes to PartialAlign
int prepare(const HostBatch& hb, size_t ri, Frag& f, bool& part) {
    const RecRef r{hb, ri};
    part = false;
    if (r.dup() || !r.mapped()) return 0;
    if (r.first() ? (r.multi() || hb.mapq[ri] == 0) : !r.multi()) return 0;  // :1723-1726 (W5)
    BlkList& own = r.first() ? f.a : f.b;  // (f.name: given by the caller where a list keeps it -- two std::strings per record otherwise, most of this loop's time)
    for (size_t k = 0; k < r.nblk(); ++k) own.push_back(r.blk(k));
    std::sort(own.begin(), own.end(), blk_less_readpos);
    (r.first() ? f.atot : f.btot) = r.totlen();
    (r.first() ? f.alow : f.blow) = r.lowphred();
    part = !r.multi() && (clipped_end(f.a, f.atot, f.alow) || clipped_end(f.b, f.btot, f.blow));
    return r.first() ? ((!f.a.empty() && (f.a.front().readpos <= 15 || f.alow)) ? 1 : 0) : (!f.b.empty() ? 2 : 0);
}
// (the mate stub and, for a second mate, the shortened own block: what LocateRead sees -- after the copy for PartialAlign was taken)
void finish_prepare(const HostBatch& hb, size_t ri, Frag& f, int kind) {
    const RecRef r{hb, ri};
    if (r.mate_mapped() && r.mrefid() != -1) (r.first() ? f.b : f.a).push_back(Blk{r.mrefid(), r.mpos(), 0, 15, 15, r.mate_rev(), false});
    if (kind == 2) { f.b.resize(1); f.b[0].matchref = 15; f.b[0].matchread = 15; }
}
void clear_frag(Frag& f) { f.a.clear(); f.b.clear(); f.name.clear(); f.atot = 0; f.btot = 0; f.alow = false; f.blow = false; }
// what the BAM loop (:1712-1880) leaves behind: the position LocateRead stands at, the edges (summed per key or not: BuildEdges sorts
// the list and adds the weights of equal keys up, :1943-1957), the -1 edges of the listed second mates, and the three lists -- in record
// order -- as record indices.  The tail turns them into fragments and names.
struct LoopResult {
    int hint = 0;
    std::vector<Edge> raw, second_edges;
    std::vector<uint32_t> part, first_dis, second;
    int64_t n_emitted = 0;  // edges as the loop emitted them
};
Edge edge_unpack(unsigned long long key, int w) {
    Edge e;
    e.a = (int32_t)(key >> 32); e.b = (int32_t)((key & 0xffffffffull) >> 2); e.ha = (key >> 1) & 1; e.hb = key & 1; e.w = w; e.gw = 0;
    return e;
}

// the BAM loop on the host threads.  one_go: one stretch (sq_debug_bwa_raw_edges, tools/bwa_edges_emu.cpp)
int bwa_raw_edges_loop(sq_ctx* c, const HostBatch& hb, const std::vector<Node>& N, bool one_go, LoopResult& L) {
    const int nn = (int)N.size();
    auto in_range = [&](int i) { return i >= 0 && i < nn; };
    auto discordant = [&](const Edge& e) { return edge_discordant(c, N, e); };
    // The loop carries ONE thing from record to record -- the position LocateRead starts from (`hint`: the node of the last located first
    // block) -- and appends to lists whose order is either the record order (PartialAlign: sorted by name afterwards with an unstable sort,
    // so the order going in counts) or does not matter (the edges are sorted and summed, the names of FirstDisInserted are sorted, the -1
    // edges are looked up one by one).  A stretch can therefore start behind any record whose first block lies deep inside ONE node --
    // LocateRead ends there from any start (sq_graph.cpp, frag_first_block_pins) --, and the stretches are worked on side by side and strung
    // together in order.
    struct Piece {
        int hint = 0;
        std::vector<Edge> raw, second_edges;
        std::vector<uint32_t> part, first_dis, second;
        int rc = SQ_OK; const char* err = nullptr;
    };
    auto run = [&](size_t lo, size_t hi, Piece& P) {
        std::vector<int> rn;
        int& hint = P.hint;
        auto add = [&](int i, bool hi_, int j, bool hj, int w) -> bool {
            if (!in_range(i) || !in_range(j)) { P.rc = SQ_E_ASSERT; P.err = "an edge would leave the node table (the reference asserts, SegmentGraph.cpp:1760)"; return false; }
            P.raw.push_back(make_edge(i, hi_, j, hj, w));
            return true;
        };
        auto split_edges = [&](const BlkList& r, size_t base) -> bool {
            for (size_t k = 0; k + 1 < r.size(); ++k) {
                const int i = rn[base + k], j = rn[base + k + 1];
                if (i != j && i != -1 && j != -1 && !add(i, r[k].rev, j, !r[k + 1].rev, 1)) return false;
            }
            return true;
        };
        Frag f;  // (one object for the stretch, emptied per record: its two block lists keep their storage -- a fresh Frag per record was two or three allocations per record on every thread)
        for (size_t ri = lo; ri < hi; ++ri) {
            clear_frag(f);
            bool part;
            const int kind = prepare(hb, ri, f, part);
            if (part) P.part.push_back((uint32_t)ri);  // (the tail builds the fragment again, with its name)
            if (kind == 0) continue;  // (a record that locates nothing leaves nothing else behind: its mate stub is only looked at by LocateRead)
            finish_prepare(hb, ri, f, kind);
            const size_t na = f.a.size();
            if (kind == 1) {
                locate_fragment(N, hint, f, rn);
                if (rn[0] != -1) hint = rn[0];
                for (size_t k = 0; k < rn.size(); ++k)
                    if (rn[k] == -1) {
                        const int i = bwa_home_node(N, hint, k < na ? f.a[k] : f.b[k - na]);
                        if (i == -2) { P.rc = SQ_E_ASSERT; P.err = "a block lies behind the last node (the reference reads past its node table, SegmentGraph.cpp:1757)"; return; }
                        if (!add(i, false, i + 1, true, 1)) return;
                    }
                if (!split_edges(f.a, 0) || !split_edges(f.b, na)) return;
                if (!f.b.empty() && !frag_end_discordant(f, true) && !frag_end_discordant(f, false)) {
                    const int i = rn[na - 1], j = rn.back();
                    if (i != j && i != -1 && j != -1 && !pair_overlap(f, rn, i, j)) {
                        if (!add(i, f.a.back().rev, j, f.b.back().rev, 1)) return;
                        if (discordant(P.raw.back())) P.first_dis.push_back((uint32_t)ri);
                    }
                }
            } else {
                locate_fragment(N, hint, f, rn);
                if (rn[0] != -1) hint = rn[0];
                if (!f.a.empty() && !frag_end_discordant(f, true)) {
                    const int i = rn[f.a.size() - 1], j = rn.back();
                    bool overlap = false;
                    for (size_t k = 0; k < f.a.size(); ++k) overlap |= j == rn[k];
                    overlap |= i == rn[f.a.size()];
                    if (i != j && i != -1 && j != -1 && !overlap) {
                        if (!in_range(i) || !in_range(j)) { P.rc = SQ_E_ASSERT; P.err = "an edge would leave the node table (the reference asserts, SegmentGraph.cpp:1852)"; return; }
                        const Edge e = make_edge(i, f.a.back().rev, j, f.b.back().rev, -1);
                        if (discordant(e)) { P.second.push_back((uint32_t)ri); P.second_edges.push_back(e); }
                    }
                }
            }
        }
    };
    const auto t_re0 = std::chrono::steady_clock::now();
    auto re_lap = [&](const char* what) { if (env_set("SQUID_BWA_DEBUG")) std::fprintf(stderr, "RawEdges: %-28s at %8.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_re0).count()); };
    // stretch boundaries: behind the nearest record in front of an even cut that pins the position (looked for among the 4096 records
    // in front of the cut; none there: that cut is left out).  SQUID_BWA_PIECE=<records> sets the stretch length (tests: small inputs)
    const long piece_env = bwa_piece_env();
    const size_t nrec = hb.size();
    const int threads = c->pool ? c->pool->size() + 1 : 1;
    std::vector<size_t> cut{0};
    std::vector<int> start{0};
    if (!one_go && threads > 1 && (piece_env > 0 || nrec >= 200000)) {
        const size_t want = piece_env > 0 ? std::max<size_t>(1, nrec / (size_t)piece_env) : (size_t)(4 * threads);
        for (size_t k = 1; k < want; ++k) {
            const size_t at = nrec * k / want;
            if (at <= cut.back()) continue;
            for (size_t q = at; q-- > cut.back() && at - q <= 4096;) {
                Frag f;
                bool part;
                const int kind = prepare(hb, q, f, part);
                if (kind == 0) continue;
                finish_prepare(hb, q, f, kind);
                int node = -1;
                if (frag_first_block_pins(N, f, node)) { cut.push_back(q + 1); start.push_back(node); break; }
            }
        }
    }
    cut.push_back(nrec);
    re_lap("stretches planned");
    const int np = (int)cut.size() - 1;
    if (!one_go) c->timer.add("bwa_raw_edge_stretches", 0.0, 0.0, np);  // (how many stretches the loop ran in: tests)
    std::vector<Piece> pieces((size_t)np);
    for (int k = 0; k < np; ++k) pieces[(size_t)k].hint = start[(size_t)k];
    // (the edges of a stretch are summed per key before they are strung together -- BuildEdges sorts the list and adds the weights of equal
    // keys up, :1943-1957, so neither the order nor the grouping of the addends shows; tens of millions of unit edges shrink to the
    // distinct keys of the stretch.  Nothing is dropped here: a sum <= 0 is only final when every stretch and the -1 edges are in)
    std::vector<int64_t> emitted((size_t)np, 0);
    auto presum = [](std::vector<Edge>& v) {
        std::sort(v.begin(), v.end(), edge_key_less);
        size_t o = 0;
        for (size_t i = 0; i < v.size(); ++i) { if (o && edge_key_eq(v[i], v[o - 1])) v[o - 1].w += v[i].w; else v[o++] = v[i]; }
        v.resize(o);
    };
    if (np > 1) c->pool->parallel_for(np, 1 << 20, [&](int k) { run(cut[(size_t)k], cut[(size_t)k + 1], pieces[(size_t)k]); emitted[(size_t)k] = (int64_t)pieces[(size_t)k].raw.size(); if (!pieces[(size_t)k].rc) presum(pieces[(size_t)k].raw); });
    else { run(0, nrec, pieces[0]); emitted[0] = (int64_t)pieces[0].raw.size(); }
    L.n_emitted = 0;
    for (int64_t e : emitted) L.n_emitted += e;
    re_lap("record loop");
    for (Piece& P : pieces) {
        if (P.rc) return fail(c, P.rc, P.err);  // (the first stretch in record order that ran into one: what the loop in one go would have hit first)
        L.raw.insert(L.raw.end(), P.raw.begin(), P.raw.end());
        L.part.insert(L.part.end(), P.part.begin(), P.part.end());
        L.first_dis.insert(L.first_dis.end(), P.first_dis.begin(), P.first_dis.end());
        L.second.insert(L.second.end(), P.second.begin(), P.second.end());
        L.second_edges.insert(L.second_edges.end(), P.second_edges.begin(), P.second_edges.end());
        L.hint = P.hint;
    }
    re_lap("stretches strung");
    return SQ_OK;
}

// everything behind the BAM loop (:1881-1930): the -1 edges whose first mate added a discordant pair edge, the fragments rebuilt from the
// partially aligned reads, their split edges.  `raw` holds the loop's edges and gets the tail's
int bwa_raw_edges_tail(sq_ctx* c, const HostBatch& hb, const std::vector<Node>& N, const LoopResult& L, std::vector<Edge>& raw) {
    const int nn = (int)N.size();
    auto in_range = [&](int i) { return i >= 0 && i < nn; };
    const auto t_re0 = std::chrono::steady_clock::now();
    auto re_lap = [&](const char* what) { if (env_set("SQUID_BWA_DEBUG")) std::fprintf(stderr, "RawEdges tail: %-23s at %8.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_re0).count()); };
    int hint = L.hint;
    std::vector<int> rn;
    // the listed records again, with their names: PartialAlign's fragments (as prepare leaves them), the names of the two other lists
    std::vector<Frag> partial(L.part.size());
    auto build = [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; ++k) { bool part; prepare(hb, L.part[k], partial[k], part); partial[k].name = RecRef{hb, L.part[k]}.qname(); } };
    if (c->pool && partial.size() > 100000) { const int np = 8 * (c->pool->size() + 1); c->pool->parallel_for(np, 1 << 20, [&](int k) { build(partial.size() * (size_t)k / (size_t)np, partial.size() * ((size_t)k + 1) / (size_t)np); }); }
    else build(0, partial.size());
    std::vector<std::string> first_dis, second_names;
    for (const uint32_t ri : L.first_dis) first_dis.push_back(RecRef{hb, ri}.qname());
    for (const uint32_t ri : L.second) second_names.push_back(RecRef{hb, ri}.qname());
    re_lap("fragments and names");
    const size_t raw_strung = raw.size();
    auto add = [&](int i, bool hi, int j, bool hj, int w) -> int {
        if (!in_range(i) || !in_range(j)) return fail(c, SQ_E_ASSERT, "an edge would leave the node table (the reference asserts, SegmentGraph.cpp:1760)");
        raw.push_back(make_edge(i, hi, j, hj, w));
        return SQ_OK;
    };
    auto split_edges = [&](const BlkList& r, size_t base) -> int {
        for (size_t k = 0; k + 1 < r.size(); ++k) {
            const int i = rn[base + k], j = rn[base + k + 1];
            if (i != j && i != -1 && j != -1) { const int rc = add(i, r[k].rev, j, !r[k + 1].rev, 1); if (rc) return rc; }
        }
        return SQ_OK;
    };
    std::sort(first_dis.begin(), first_dis.end());
    for (size_t k = 0; k < second_names.size(); ++k)
        if (std::binary_search(first_dis.begin(), first_dis.end(), second_names[k])) raw.push_back(L.second_edges[k]);
    // the fragments of the partially aligned reads: grouped by name (the sort of :1883 is libstdc++'s introsort on the names, ledger B8),
    // merged, stored untrimmed, located from the hint the loop above left behind (W4); the last group is dropped (W3)
    // (what is sorted is the index of every fragment with the same comparison: introsort takes the same decisions, hence the same order, without
    // moving 100-byte objects around; `name < name` is a strict weak order, so the threaded form with the split final pass applies, sq_parsort.h)
    std::vector<uint32_t> by_name(partial.size());
    for (size_t i = 0; i < by_name.size(); ++i) by_name[i] = (uint32_t)i;
    std_sort_parallel(by_name.begin(), by_name.end(), [&](uint32_t x, uint32_t y) { return partial[x].name < partial[y].name; }, c->pool ? std::min(c->pool->size() + 1, 32) : 1, true);
    re_lap("partial reads sorted by name");
    std::vector<Frag> rebuilt;
    Frag cur;
    for (const uint32_t pi : by_name) {
        const Frag& p = partial[pi];
        if (cur.a.empty() && cur.b.empty()) { cur = p; continue; }
        if (cur.name == p.name) { cur.a.insert(cur.a.end(), p.a.begin(), p.a.end()); cur.b.insert(cur.b.end(), p.b.begin(), p.b.end()); continue; }
        std::sort(cur.a.begin(), cur.a.end(), blk_less_readpos);
        std::sort(cur.b.begin(), cur.b.end(), blk_less_readpos);
        if (cur.a.size() > 1 || cur.b.size() > 1) {
            rebuilt.push_back(cur);
            locate_fragment(N, hint, cur, rn);
            int rc = split_edges(cur.a, 0);
            if (!rc) rc = split_edges(cur.b, cur.a.size());
            if (rc) return rc;
        }
        cur = p;
    }
    // ReadRec_t::FrontSmallerThan (ReadRec.cpp:90-117; not a strict weak order, kept as it is)
    std::sort(rebuilt.begin(), rebuilt.end(), [](const Frag& x, const Frag& y) {
        const Blk* p = !x.a.empty() && !y.a.empty() ? &x.a.front() : !x.b.empty() && !y.b.empty() ? &x.b.front() : !x.a.empty() && !y.b.empty() ? &x.a.front() : !x.b.empty() && !y.a.empty() ? &x.b.front() : nullptr;
        const Blk* q = !x.a.empty() && !y.a.empty() ? &y.a.front() : !x.b.empty() && !y.b.empty() ? &y.b.front() : !x.a.empty() && !y.b.empty() ? &y.b.front() : !x.b.empty() && !y.a.empty() ? &y.a.front() : nullptr;
        return p && q && blk_less_pos(*p, *q);
    });
    c->frags = rebuilt;
    c->frags0 = c->frags;
    // the name set ExactBPConcordantSupport tests raw QNAMEs against (:3113-3118; the sized-then-appended vector also holds "", ledger B9)
    c->chim_names.clear();
    if (!rebuilt.empty()) c->chim_names.push_back(std::string());
    for (const Frag& f : rebuilt) c->chim_names.push_back(f.name);
    std::sort(c->chim_names.begin(), c->chim_names.end());
    c->chim_names.erase(std::unique(c->chim_names.begin(), c->chim_names.end()), c->chim_names.end());
    c->counts.n_chim_fragments = (int64_t)rebuilt.size();
    re_lap("fragments rebuilt");
    c->counts.n_raw_edges = L.n_emitted + (int64_t)(raw.size() - raw_strung);  // (as the loops emitted them: the loop's edges arrive summed)
    return SQ_OK;
}
}  // namespace

// the host route: the loop on the host threads, then the tail
static int bwa_raw_edges(sq_ctx* c, const HostBatch& hb, std::vector<Edge>& raw) {
    LoopResult L;
    int rc = bwa_raw_edges_loop(c, hb, c->nodes, false, L);
    if (rc) return rc;
    raw.swap(L.raw);
    return bwa_raw_edges_tail(c, hb, c->nodes, L, raw);
}
// the device route (sq_bwa_edges_on_device): the loop as kernels over the resident table, the tail here.  fallback: nothing was done
static int bwa_raw_edges_device(sq_ctx* c, const HostBatch& hb, std::vector<Edge>& raw, bool& fallback) {
    BwaEdgesOut D;
    int rc = dev_bwa_raw_edges(c, c->nodes, D);
    if (rc == SQ_E_CAPACITY) { fallback = true; return SQ_OK; }
    if (rc) return rc;
    fallback = D.fallback;
    if (fallback) { if (env_set("SQUID_BWA_DEBUG")) std::fprintf(stderr, "RawEdges on the device: back to the host loop (%s)\n", D.why); return SQ_OK; }
    LoopResult L;
    L.hint = D.final_pos;
    raw.reserve(D.keys.size());
    for (size_t i = 0; i < D.keys.size(); ++i) { raw.push_back(edge_unpack(D.keys[i], (int)D.counts[i])); L.n_emitted += (int64_t)D.counts[i]; }
    L.part.swap(D.part); L.first_dis.swap(D.first_dis); L.second.swap(D.second);
    for (const unsigned long long key : D.second_keys) L.second_edges.push_back(edge_unpack(key, -1));
    c->timer.add("bwa_edge_soft_fragments", 0.0, 0.0, D.n_soft);
    c->timer.add("bwa_edge_lists", 0.0, 0.0, (int64_t)(L.part.size() + L.first_dis.size() + L.second.size()));
    HostClock hc(c, "host_bwa_raw_edges_tail");
    return bwa_raw_edges_tail(c, hb, c->nodes, L, raw);
}

// sq_debug_bwa_raw_edges (see sq_internal.h)
int bwa_raw_edges_debug(sq_ctx* c, const HostBatch* tables, const std::vector<Node>& N, int route, BwaEdgesDebug& out) {
    if (!tables && !c->bwa) return fail(c, SQ_E_ARG, "sq_ingest_bwa_file first");
    const HostBatch& hb = tables ? *tables : *c->bwa;
    out = BwaEdgesDebug();
    std::vector<std::pair<unsigned long long, int32_t>> kw;
    if (route == 0) {
        LoopResult L;
        const int rc = bwa_raw_edges_loop(c, hb, N, true, L);
        if (rc) return rc;
        for (const Edge& e : L.raw) kw.push_back(std::make_pair((unsigned long long)edge_pack(e), e.w));
        for (const Edge& e : L.second_edges) out.second_keys.push_back(edge_pack(e));
        out.part.swap(L.part); out.first_dis.swap(L.first_dis); out.second.swap(L.second);
        out.final_pos = L.hint; out.n_emitted = L.n_emitted;
    } else {
        if (!c->dev) return fail(c, SQ_E_ARG, "no device");
        if (tables || !c->bwa_resident) {
            const int rc = dev_bwa_upload(c, hb);
            if (rc && rc != SQ_E_CAPACITY) return rc;
            c->bwa_resident = rc == SQ_OK;
            c->bwa_dev_active = false;
        }
        BwaEdgesOut D;
        const int rc = dev_bwa_raw_edges(c, N, D);
        if (tables) { dev_clear_records(c); c->bwa_resident = false; }
        if (rc) return rc;
        out.fallback = D.fallback; out.n_soft = D.n_soft; out.final_pos = D.final_pos;
        for (size_t i = 0; i < D.keys.size(); ++i) { kw.push_back(std::make_pair(D.keys[i], (int32_t)D.counts[i])); out.n_emitted += (int64_t)D.counts[i]; }
        out.part.swap(D.part); out.first_dis.swap(D.first_dis); out.second.swap(D.second); out.second_keys.swap(D.second_keys);
    }
    std::sort(kw.begin(), kw.end());
    for (const auto& x : kw) {
        if (!out.keys.empty() && out.keys.back() == x.first) out.weights.back() += x.second;
        else { out.keys.push_back(x.first); out.weights.push_back(x.second); }
    }
    return SQ_OK;
}

// the device route's part of BuildNode_BWA: node table, class bytes (READS) and the depth kernels over the resident table.
// fallback: the kernels found a chromosome going down along Reads -- nothing was written, the caller takes the host loop
static int bwa_depth_on_device(sq_ctx* c, bool& fallback, int64_t& n_reads_records) {
    int rc = dev_upload_nodes(c, c->nodes);
    if (rc) return rc;
    int64_t n_p3 = 0, n_reads_blocks = 0;
    rc = dev_bwa_classify(c, nullptr, n_reads_records, n_p3, n_reads_blocks);
    if (rc) return rc;
    c->bwa_p3_ready = false;
    std::vector<int32_t> cnts, sums;
    int64_t held = 0;
    fallback = false;
    if (n_reads_blocks) {  // (no read at all: the reference leaves Support / AvgDepth as constructed)
        rc = dev_bwa_node_depth(c, (int)c->nodes.size(), cnts, sums, held, fallback);
        if (rc) return rc;
        if (!fallback) bwa_set_node_depths(c->nodes, cnts, sums);
    }
    c->timer.add("bwa_depth_held_blocks", 0.0, 0.0, fallback ? 0 : held);
    return SQ_OK;
}

// BuildNode_BWA + RawEdges: c->nodes, c->frags and the raw edge list
int bwa_nodes_and_edges(sq_ctx* c, std::vector<Edge>& raw) {
    if (!c->bwa) return fail(c, SQ_E_ARG, "sq_ingest_bwa_file first");
    const HostBatch& hb = *c->bwa;
    std::vector<Node> seeds;
    std::vector<std::vector<Blk>> reads;  // (the Reads list, stretch by stretch)
    int rc;
    // sq_bwa_on_device: the batch goes to HBM once, on a thread of its own next to the seed nodes (which need nothing from the device; a
    // task of the pool that waits for tasks of the pool can starve, segment_clusters) -- joined in front of the depth stage
    const bool route = c->dev && c->bwa_dev_on();
    c->bwa_dev_active = false;
    std::thread upload;
    int up_rc = SQ_OK;
    std::string up_err;
    double up_ms = 0;
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{upload};  // (an exception of the seed nodes must not meet a running thread)
    if (route && !c->bwa_resident)
        upload = std::thread([&]() {
            ErrSink sink(&up_err);
            const auto t0 = std::chrono::steady_clock::now();
            up_rc = dev_bwa_upload(c, hb);
            up_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
    int64_t n_reads_records = 0;
    // sq_bwa_nodes_on_device: the automaton over the resident table, so the upload cannot hide behind it (bwa_upload_wait shows all of it); a
    // graph the kernels hand back (a flag, no table, no memory) takes the host automaton -- same results
    bool nodes_on_device = false;
    auto join_upload = [&]() {
        if (!upload.joinable()) return;
        const auto t0 = std::chrono::steady_clock::now();
        upload.join();
        c->timer.add("bwa_upload", up_ms, 0.0, 1);
        c->timer.add("bwa_upload_wait", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), 0.0, 1);  // (what did not hide behind the seed nodes)
        if (up_rc == SQ_OK) c->bwa_resident = true;
    };
    rc = SQ_OK;
    if (c->dev && c->bwa_nodes_on()) {
        join_upload();
        bool fallback = !c->bwa_resident;
        if (!fallback) {
            BwaNodesWalk W;
            int rl = c->read_len;
            rc = bwa_seed_nodes_device(c, hb, seeds, n_reads_records, rl, fallback, W);
            if (!rc && !fallback) {
                c->read_len = rl;
                c->timer.add("bwa_node_stretches", 0.0, 0.0, W.stretches);
                c->timer.add("bwa_node_stretches_run_again", 0.0, 0.0, W.again);
                c->timer.add("bwa_node_longest_stretch", 0.0, 0.0, W.longest);
            }
        }
        if (!rc) c->timer.add("bwa_nodes_device_fallback", 0.0, 0.0, fallback ? 1 : 0);
        nodes_on_device = !rc && !fallback;
        if (!nodes_on_device) seeds.clear();
    }
    if (!rc && !nodes_on_device) { HostClock hc(c, "host_bwa_seed_nodes"); rc = bwa_seed_nodes(c, hb, seeds, reads, n_reads_records); }
    join_upload();
    if (rc) return rc;
    if (up_rc != SQ_OK && up_rc != SQ_E_CAPACITY) return fail(c, up_rc, up_err);  // (only a batch the table cannot hold goes back to the host loops)
    c->counts.read_len = c->read_len;
    { HostClock hc(c, "host_tile_genome"); rc = tile_genome(c, seeds, c->nodes); }
    if (rc) return rc;
    bool on_device = false;
    if (route) {
        // (a batch the device table cannot hold -- a record of more than 256 blocks -- keeps the host route for this graph)
        bool fallback = !c->bwa_resident;
        if (!fallback) {
            int64_t dev_reads = 0;
            rc = bwa_depth_on_device(c, fallback, dev_reads);
            if (rc) return rc;
            c->bwa_dev_active = true;
            on_device = !fallback;
            n_reads_records = dev_reads;
        }
        c->timer.add("bwa_device_fallback", 0.0, 0.0, fallback ? 1 : 0);
    }
    if (!on_device) {
        if (nodes_on_device) { HostClock hc(c, "host_bwa_reads_list"); bwa_reads_list(c, hb, reads); }  // (the device automaton builds no Reads list)
        HostClock hc(c, "host_bwa_node_depth"); bwa_node_depth(c->nodes, reads);
    }
    c->timer.add("bwa_reads_records", 0.0, 0.0, n_reads_records);
    c->snap[1].take(c->nodes, std::vector<Edge>(), nullptr);
    raw.clear();
    // sq_bwa_edges_on_device: RawEdges' BAM loop over the resident table; a graph it cannot take (no table, equal read offsets inside a
    // record, an assert of the reference, no memory) keeps the host loop -- same results, same error text
    if (c->dev && c->bwa_edges_on()) {
        bool fallback = !c->bwa_resident;
        if (!fallback) { rc = bwa_raw_edges_device(c, hb, raw, fallback); if (rc) return rc; }
        c->timer.add("bwa_edges_device_fallback", 0.0, 0.0, fallback ? 1 : 0);
        if (!fallback) return SQ_OK;
        raw.clear();
    }
    { HostClock hc(c, "host_bwa_raw_edges"); rc = bwa_raw_edges(c, hb, raw); }
    return rc;
}

// ---- which records ExactBPConcordantSupport's loop looks at (:3136-3142)
namespace {
// std::binary_search(names, raw QNAME of a record) without building the std::string, behind one bit per name hash -- 15 k names in 4 M
// bits; all but one record in a few thousand end there (the name test, a binary search per record, was 6.5 s of one thread for C3's 50.8 M records)
struct NameTest {
    const HostBatch& hb;
    const std::vector<std::string>& names;
    static constexpr size_t nbits = (size_t)1 << 22;
    std::vector<uint64_t> maybe;
    static unsigned long long hash_of(const char* p, size_t L) { unsigned long long h = 1469598103934665603ull; for (size_t i = 0; i < L; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ull; } h ^= h >> 29; return h; }
    NameTest(const HostBatch& hb, const std::vector<std::string>& names) : hb(hb), names(names) {
        if (names.empty()) return;
        maybe.assign(nbits / 64, 0);
        for (const std::string& nm : names) { const unsigned long long h = hash_of(nm.data(), nm.size()) & (nbits - 1); maybe[h >> 6] |= 1ull << (h & 63); }
    }
    bool in_names(size_t ri) const {
        const char* p = hb.names.data() + hb.name_off[ri];
        const size_t L = hb.name_off[ri + 1] - hb.name_off[ri];
        size_t lo = 0, hi = names.size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            const std::string& m = names[mid];
            const int cmp = std::memcmp(m.data(), p, std::min(m.size(), L));
            if (cmp < 0 || (cmp == 0 && m.size() < L)) lo = mid + 1; else hi = mid;
        }
        return lo < names.size() && names[lo].size() == L && std::memcmp(names[lo].data(), p, L) == 0;
    }
    bool in_names_fast(size_t ri) const {
        if (names.empty()) return false;
        const char* p = hb.names.data() + hb.name_off[ri];
        const unsigned long long h = hash_of(p, hb.name_off[ri + 1] - hb.name_off[ri]) & (nbits - 1);
        return ((maybe[h >> 6] >> (h & 63)) & 1) && in_names(ri);
    }
};
template <class F> void over_records(sq_ctx* c, size_t nrec, const F& f) {  // f(lo, hi) side by side on the host threads
    if (c->pool && nrec > 100000) { const int np = 8 * (c->pool->size() + 1); c->pool->parallel_for(np, 1 << 20, [&](int k) { f(nrec * (size_t)k / (size_t)np, nrec * ((size_t)k + 1) / (size_t)np); }); }
    else f(0, nrec);
}
}  // namespace
// look[r] = 1: the loop looks at record r -- its own flags, its mate's place, its QNAME against the name set of the rebuilt fragments
void bwa_look_bytes(sq_ctx* c, std::vector<uint8_t>& look) {
    const HostBatch& hb = *c->bwa;
    const NameTest nt(hb, c->chim_names);
    look.assign(hb.size(), 0);
    auto decide = [&](size_t lo, size_t hi) {
        for (size_t ri = lo; ri < hi; ++ri) {
            const RecRef r{hb, ri};
            if (r.multi() || (int)hb.mapq[ri] < c->P.min_mapqual || r.dup() || !r.mapped() || r.refid() == -1) continue;
            const bool same_chr_mate = r.mate_mapped() && r.mrefid() == r.refid();
            if (same_chr_mate && (r.mpos() > r.pos() || (r.mpos() == r.pos() && (r.flag() & 0x80)))) continue;  // only the right-hand record of a pair
            if (nt.in_names_fast(ri)) continue;
            look[ri] = 1;
        }
    };
    over_records(c, hb.size(), decide);
}
// the name test alone, one byte per record (the device route: the names are on the host, the other factors are the class kernel's)
void bwa_name_bytes(sq_ctx* c, std::vector<uint8_t>& in_names) {
    const HostBatch& hb = *c->bwa;
    const NameTest nt(hb, c->chim_names);
    in_names.assign(hb.size(), 0);
    over_records(c, hb.size(), [&](size_t lo, size_t hi) { for (size_t ri = lo; ri < hi; ++ri) in_names[ri] = nt.in_names_fast(ri) ? 1 : 0; });
}
// reads[r] = 1: record r feeds Reads (:871-881)
void bwa_reads_bytes(const HostBatch& hb, std::vector<uint8_t>& reads) {
    reads.assign(hb.size(), 0);
    for (size_t ri = 0; ri < hb.size(); ++ri) reads[ri] = seed_record_passes(hb, ri) ? 1 : 0;
}

// the same count over the resident table (sq_bwa_on_device): the class kernel sets C_P3 behind the name test, once per graph, and the
// breakpoint kernels of the STAR path walk the table
int bwa_breakpoint_support_device(sq_ctx* c, const std::vector<std::pair<int, int>>& bps, std::vector<int32_t>& cov, bool count_row) {
    if (!c->bwa || !c->bwa_dev_active) return fail(c, SQ_E_ARG, "internal: the --bwa table of this graph is not on the device");
    if (!c->bwa_p3_ready) {
        std::vector<uint8_t> in_names;
        { HostClock hc(c, "host_bwa_name_test"); bwa_name_bytes(c, in_names); }
        int64_t n_reads = 0, n_blocks = 0;
        const int rc = dev_bwa_classify(c, in_names.data(), n_reads, c->bwa_n_p3, n_blocks);
        if (rc) return rc;
        c->bwa_p3_ready = true;
    }
    if (count_row) c->timer.add("bwa_bp_records", 0.0, 0.0, c->bwa_n_p3);
    return dev_breakpoint_support(c, bps, cov);
}

// ExactBPConcordantSupport's counting loop (:3129-3166) over the host batch: `bps` sorted (chr, pos)
int bwa_breakpoint_support(sq_ctx* c, const std::vector<std::pair<int, int>>& bps, std::vector<int32_t>& cov, bool count_row) {
    if (!c->bwa) return fail(c, SQ_E_ARG, "sq_ingest_bwa_file first");
    const HostBatch& hb = *c->bwa;
    HostClock hc(c, "host_bwa_bp_support");
    cov.assign(bps.size(), 0);
    // which records the loop looks at at all is decided per record before the loop touches the one thing it carries (the cursor): decided
    // side by side on the host threads, and the loop then walks the survivors
    const size_t nrec = hb.size();
    std::vector<uint8_t> look;
    bwa_look_bytes(c, look);
    if (count_row) {
        std::atomic<int64_t> n_look{0};
        over_records(c, nrec, [&](size_t lo, size_t hi) { int64_t k = 0; for (size_t ri = lo; ri < hi; ++ri) k += look[ri]; n_look += k; });
        c->timer.add("bwa_bp_records", 0.0, 0.0, n_look.load());
    }
    if (bps.empty()) return SQ_OK;
    // The walk itself: the cursor moves one entry per record at most and never back (:3157), so where it stands depends on every record
    // before -- but it is a small number that a walk from 0 over a few ten thousand records in front of a stretch usually reproduces (two
    // cursors fed the same records never cross, and meet for good once the one behind has caught up).  Every stretch walks from such a
    // guess into counts of its own; the stretches are then checked in order -- a guess that is not the cursor the stretch in front ended
    // with: that stretch is walked again from the real one -- and the counts added up.
    auto walk = [&](size_t lo, size_t hi, size_t cur, std::vector<int32_t>* into) -> size_t {
        for (size_t ri = lo; ri < hi; ++ri) {
            if (!look[ri]) continue;
            if (cur == bps.size()) break;
            const RecRef r{hb, ri};
            const bool same_chr_mate = r.mate_mapped() && r.mrefid() == r.refid();
            const int chr = r.refid(), start = same_chr_mate ? r.mpos() : r.pos(), end = hb.endpos[ri];
            if (chr > bps[cur].first || (chr == bps[cur].first && start > bps[cur].second + c->P.concord_dist_pos)) ++cur;
            if (!into) continue;
            for (size_t k = cur; k < bps.size(); ++k) {
                if (chr == bps[k].first && start <= bps[k].second && end > bps[k].second) ++(*into)[k];
                else if (chr < bps[k].first || (chr == bps[k].first && end <= bps[k].second)) break;
            }
        }
        return cur;
    };
    const long piece_env = bwa_piece_env();  // (tests: short stretches and a short warm-up on small inputs)
    const int np = !c->pool ? 1 : piece_env > 0 ? (int)std::min<size_t>(4096, std::max<size_t>(1, nrec / (size_t)piece_env)) : (nrec > 400000 ? 4 * (c->pool->size() + 1) : 1);
    const size_t warm_len = piece_env > 0 ? (size_t)piece_env : 65536;
    if (np == 1) { walk(0, nrec, 0, &cov); return SQ_OK; }
    auto lo_of = [&](int k) { return nrec * (size_t)k / (size_t)np; };
    struct Part { size_t guess = 0, end = 0; std::vector<int32_t> cov; };
    std::vector<Part> parts((size_t)np);
    c->pool->parallel_for(np, 1 << 20, [&](int k) {
        Part& P = parts[(size_t)k];
        const size_t lo = lo_of(k), warm = lo > warm_len ? lo - warm_len : 0;
        P.guess = k == 0 ? 0 : walk(warm, lo, 0, nullptr);
        P.cov.assign(bps.size(), 0);
        P.end = walk(lo, lo_of(k + 1), P.guess, &P.cov);
    });
    int again = 0;
    for (int k = 1; k < np; ++k) {
        Part& P = parts[(size_t)k];
        const size_t real = parts[(size_t)k - 1].end;
        if (P.guess == real) continue;
        P.cov.assign(bps.size(), 0);
        P.end = walk(lo_of(k), lo_of(k + 1), real, &P.cov);
        ++again;
    }
    c->timer.add("bwa_bp_support_stretches_walked_again", 0.0, 0.0, again);
    for (const Part& P : parts) for (size_t k = 0; k < bps.size(); ++k) cov[k] += P.cov[k];
    return SQ_OK;
}

}  // namespace sq
