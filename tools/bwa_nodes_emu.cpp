// BuildNode_BWA's record automaton of the --bwa device route (squid_amd/csrc/sq_bwa_nodes.inc: class bytes, the tile-local prefix maxima
// that cut the stream at every gap record, the discordant list, the dis_right every stretch starts with, one wave per stretch) on the CPU:
// the kernel source itself (sq_wave.h with SQ_WAVE_EMU; lane-local bodies are called once per index from the last to the first, wave
// bodies run as 64 coroutines, the compacting scans of dev_bwa_seed_nodes are plain loops), then the library's own walk over the stretch
// reports (bwa_seed_nodes_walk: a stretch whose guess was wrong where it counted is run again with seed_step), against the host automaton
// in one go (bwa_seed_nodes_debug route 0; linked against libsquid_hip.so, no device needed).  Compared: the seeds (chr, pos, len) in
// order, the final read length, the records that feed Reads, the flushes that emitted a node, the marks closed by the zero-coverage rule.
//   bwa_nodes_emu <bwa.bam> [read_len]                          the file's records
//   bwa_nodes_emu --fuzz <cases> <seed> [--write <file>]        random record tables (see make_case); --write keeps the cases as numbers
//                                                               for the device test (sq_debug_bwa_seed_nodes_tables)
#include "../squid_amd/csrc/sq_internal.h"
#include "../squid_amd/csrc/sq_bwa_nodes.inc"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
using namespace sq;

namespace {
struct WaveArg {
    const bwn::Keys* K; uint8_t* cls; int64_t tile, ntiles; long long *tmax, *front; int rl_final; uint32_t* flags;
    const bwn::Tab* T; const bwn::Par* P; const int32_t* cut; int32_t np; int32_t *has, *dr, *dis_in, *margins, *seeds, *report; int64_t k;
};
void w_tile_max(void* p) { const WaveArg& a = *(const WaveArg*)p; bwn::tile_max(*a.K, a.cls, a.tile, a.tmax); }
void w_tile_prefix(void* p) { const WaveArg& a = *(const WaveArg*)p; bwn::tile_prefix(a.ntiles, a.tmax, a.front); }
void w_tile_cut(void* p) { const WaveArg& a = *(const WaveArg*)p; bwn::tile_cut(*a.K, a.cls, a.tile, a.front, a.rl_final, a.flags); }
void w_carry(void* p) { const WaveArg& a = *(const WaveArg*)p; bwn::dis_carry(a.np, a.has, a.dr, a.dis_in); }
void w_run(void* p) { const WaveArg& a = *(const WaveArg*)p; bwn::run_stretch(*a.T, *a.P, a.cut, a.np, a.dis_in, a.margins, a.seeds, a.report, a.flags, a.k); }

// dev_bwa_seed_nodes, step by step.  cover_fails: positions whose support passed the first test and failed against the concordant cover
void emulate(const HostBatch& hb, int read_len, const int32_t rl5[5], BwaNodesOut& D, long& cover_fails, uint32_t& flag_word) {
    D = BwaNodesOut();
    cover_fails = 0; flag_word = 0;
    const int64_t n = (int64_t)hb.size();
    if (n == 0) {
        D.cut = {0, 0}; D.dis_in = {0}; D.report.assign(bwn::REPORT, 0);
        bwn::empty_report(D.report.data(), read_len);
        return;
    }
    const RecCols R = hb.cols();
    std::vector<uint8_t> cls((size_t)n + 4, 0xff);
    std::vector<int32_t> p0((size_t)n, INT32_MIN), e0((size_t)n, INT32_MIN), at_cut((size_t)n + 1, -7), drank((size_t)n + 1, -7), crank((size_t)n + 1, -7);
    for (int64_t r = n; r-- > 0;) bwn::class_record(R, cls.data(), p0.data(), e0.data(), r);
    const int64_t ntiles = (n + bwn::TILE_RECS - 1) / bwn::TILE_RECS;
    std::vector<long long> tmax(2 * (size_t)ntiles, -99), front(2 * (size_t)ntiles, -99);
    uint32_t flags[16] = {0};
    const bwn::Keys K{n, hb.refid.data(), hb.pos.data(), e0.data()};
    WaveArg a{};
    a.K = &K; a.cls = cls.data(); a.ntiles = ntiles; a.tmax = tmax.data(); a.front = front.data(); a.rl_final = rl5[4]; a.flags = flags;
    for (int64_t t = ntiles; t-- > 0;) { a.tile = t; wv::run_wave(w_tile_max, &a); }
    wv::run_wave(w_tile_prefix, &a);
    for (int64_t t = ntiles; t-- > 0;) { a.tile = t; wv::run_wave(w_tile_cut, &a); }
    flag_word = flags[0];
    if (flags[0] & bwn::FLAG_UNSORTED) { D.fallback = true; D.why = "unsorted"; return; }
    int32_t n_cut = 0, nd = 0, nc = 0;
    for (int64_t r = 0; r < n; ++r) {
        at_cut[(size_t)r] = n_cut; drank[(size_t)r] = nd; crank[(size_t)r] = nc;
        n_cut += (cls[(size_t)r] & bwn::N_CUT) != 0; nd += (cls[(size_t)r] & bwn::W_MASK) == bwn::W_DIS; nc += (cls[(size_t)r] & bwn::W_MASK) == bwn::W_PART;
    }
    at_cut[(size_t)n] = n_cut; drank[(size_t)n] = nd; crank[(size_t)n] = nc;
    const int32_t np = n_cut + 1;
    const int64_t seed_slots = bwn::seed_slots(nd, nc, np), margin_slots = bwn::margin_slots(nd, nc);
    std::vector<int32_t> cut((size_t)np + 1, -7), has((size_t)np, -7), dr((size_t)np, -7), dis_in((size_t)np, -7), report((size_t)np * bwn::REPORT, -7), margins((size_t)margin_slots + 4, INT32_MIN),
        seeds(3 * (size_t)seed_slots + 4, INT32_MIN);
    std::vector<uint32_t> dlist((size_t)nd + 1, ~0u);
    for (int64_t r = n; r-- > 0;) bwn::scatter(n, cls.data(), at_cut.data(), drank.data(), n_cut, cut.data(), dlist.data(), r);
    const bwn::Tab T{n, hb.refid.data(), hb.pos.data(), hb.totlen.data(), cls.data(), p0.data(), e0.data(), dlist.data(), drank.data(), crank.data()};
    bwn::Par P;
    P.read_len = read_len; P.rl_final = rl5[4];
    for (int i = 0; i < 5; ++i) P.rl5[i] = rl5[i];
    for (int64_t k = np; k-- > 0;) bwn::dis_summary(T, P, cut.data(), np, has.data(), dr.data(), k);
    a.T = &T; a.P = &P; a.cut = cut.data(); a.np = np; a.has = has.data(); a.dr = dr.data(); a.dis_in = dis_in.data(); a.margins = margins.data(); a.seeds = seeds.data(); a.report = report.data();
    wv::run_wave(w_carry, &a);
    for (int64_t k = np; k-- > 0;) { a.k = k; wv::run_wave(w_run, &a); }
    flag_word = flags[0];
    if (flags[0]) { D.fallback = true; D.why = "a slice or a bound"; return; }
    std::vector<int32_t> at((size_t)np, 0);
    int32_t total = 0;
    for (int32_t k = 0; k < np; ++k) { at[(size_t)k] = total; total += report[(size_t)k * bwn::REPORT + bwn::R_SEEDS]; cover_fails += report[(size_t)k * bwn::REPORT + bwn::R_COVER_FAILS]; }
    D.seeds3.assign(3 * (size_t)total + 1, INT32_MIN);
    for (int64_t k = np; k-- > 0;) bwn::gather_seeds(np, report.data(), at.data(), seeds.data(), D.seeds3.data(), k);
    D.seeds3.resize(3 * (size_t)total);
    D.cut = cut; D.dis_in = dis_in; D.report = report;
}

struct Both { BwaNodesDebug h; std::vector<Node> seeds; BwaNodesWalk W; int64_t reads = 0; int read_len = 0; long cover_fails = 0; bool fallback = false; uint32_t flag_word = 0; };
// both routes on one batch.  A table the kernels hand back (fallback) is not compared
long compare(sq_ctx& c, const HostBatch& hb, Both& b, bool say) {
    long bad = 0;
    if (bwa_seed_nodes_debug(&c, &hb, 0, b.h)) { if (say) std::printf("   host automaton: %s\n", c.err.c_str()); return 1; }
    int32_t rl5[5];
    int rl = c.read_len;
    for (size_t i = 0; i < 5; ++i) { if (i < hb.size()) rl = std::max(rl, (int)hb.totlen[i]); rl5[i] = rl; }
    BwaNodesOut D;
    emulate(hb, c.read_len, rl5, D, b.cover_fails, b.flag_word);
    b.fallback = D.fallback;
    if (D.fallback) return 0;
    b.seeds.clear();
    if (bwa_seed_nodes_walk(&c, hb, rl5, D, b.seeds, b.reads, b.read_len, b.W)) { if (say) std::printf("   walk: %s\n", c.err.c_str()); return 1; }
    std::vector<int32_t> s3;
    for (const Node& nd : b.seeds) { s3.push_back(nd.chr); s3.push_back(nd.pos); s3.push_back(nd.len); }
    auto diff = [&](const char* what, bool d) { if (d) { ++bad; if (say) std::printf("   %s differ\n", what); } };
    diff("seeds", s3 != b.h.seeds3);
    diff("read lengths", b.read_len != b.h.read_len);
    diff("Reads records", b.reads != b.h.n_reads_records);
    diff("flushes that emitted a node", b.W.flush_nodes != b.h.flush_nodes);
    diff("marks closed", b.W.marks_closed != b.h.marks_closed);
    if (bad && say) {
        std::printf("   host: %zu seeds, RL %d, %lld Reads records, %lld / %lld; emulated: %zu seeds, RL %d, %lld Reads records, %lld / %lld, %lld stretches (%lld again)\n", b.h.seeds3.size() / 3, b.h.read_len,
                    (long long)b.h.n_reads_records, (long long)b.h.flush_nodes, (long long)b.h.marks_closed, b.seeds.size(), b.read_len, (long long)b.reads, (long long)b.W.flush_nodes, (long long)b.W.marks_closed,
                    (long long)b.W.stretches, (long long)b.W.again);
        for (size_t i = 0, shown = 0; i < std::max(s3.size(), b.h.seeds3.size()) / 3 && shown < 6; ++i) {
            const bool hh = 3 * i + 2 < b.h.seeds3.size(), ee = 3 * i + 2 < s3.size();
            if (hh && ee && !std::memcmp(&s3[3 * i], &b.h.seeds3[3 * i], 12)) continue;
            std::printf("   seed %zu: host (%d %d %d), emulated (%d %d %d)\n", i, hh ? b.h.seeds3[3 * i] : -9, hh ? b.h.seeds3[3 * i + 1] : -9, hh ? b.h.seeds3[3 * i + 2] : -9, ee ? s3[3 * i] : -9, ee ? s3[3 * i + 1] : -9,
                        ee ? s3[3 * i + 2] : -9);
            ++shown;
        }
    }
    return bad;
}

// ---- fuzz
constexpr int PAIRED = 1, PROPER = 2, UNMAPPED = 4, REV = 0x10, MATE_REV = 0x20, FIRST = 0x40, SECOND = 0x80, DUP = 0x400;
struct Rec { int refid, pos, mrefid, mpos, flag, totlen, mapq, aux; std::vector<int> b; /* refpos, matchref, readpos, matchread */ };
struct Case {
    HostBatch hb;
    long planted_unsorted = 0, run_at_end = 0, long_runs = 0, cut_at_8 = 0, zero_blocks_at_change = 0, clipped_fwd = 0, clipped_rev = 0, stale = 0;
};
// table sizes the issue names first, then sizes around the tiles of the cut kernels (1024 records) and larger ones
const int SIZES[] = {0, 1, 63, 64, 65, 129, 9, 300, 1023, 1024, 1025, 2049, 40, 700, 800, 1100, 16, 200, 520, 90};
// A table is a walk along 1-3 chromosomes: islands of coverage (records a few bases apart) with gaps between them that are either cuts
// (more than RL + 64 behind everything) or only zero coverage (between RL and RL + 64) or none.  Inside an island the records are
// concordant (shallow or deep cover), clipped concordant on either strand, discordant in runs (dense: many starts within three bases),
// filtered (MAPQ 0, duplicate, multi-aligned) or without a block.  plant: see the counters of Case
Case make_case(std::mt19937_64& rng, int index) {
    Case cs;
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int want = SIZES[index % (int)(sizeof SIZES / sizeof *SIZES)];
    const bool unsorted = index % 10 == 7 && want >= 16;
    const bool cut8 = index % 4 == 2 && want >= 40;
    const bool stale = index % 3 == 1 && want >= 60;
    std::vector<Rec> recs;
    const int nchr = want < 30 ? rnd(1, 2) : rnd(2, 3);
    const int read = rnd(0, 2) == 0 ? 50 : rnd(0, 1) ? 76 : 100;
    auto one = [&](int chr, int pos, int kind, bool rev) {  // kind 0 concordant, 1 clipped concordant, 2 discordant, 3 filtered, 4 no block
        Rec r;
        r.refid = chr; r.pos = pos; r.mapq = rnd(1, 60); r.aux = 0; r.totlen = read;
        int lead = 0, len = read;
        if (kind == 1) { if (rnd(0, 1)) { lead = rnd(16, 25); len = read - lead; } else len = read - rnd(16, 25); (rev ? cs.clipped_rev : cs.clipped_fwd)++; }
        else if (rnd(0, 9) == 0) { lead = rnd(0, 15); len = read - lead - rnd(0, 15 - lead); }
        if (kind == 2 && rnd(0, 3) == 0) len = rnd(20, read);
        r.b = {pos, len, lead, len};
        if (kind != 4 && rnd(0, 7) == 0) { r.b.insert(r.b.end(), {pos + len + rnd(50, 3000), rnd(5, 30), lead + len, 10}); r.totlen += 10; }  // (a spliced read: only the first block joins a window)
        if (kind == 4) r.b.clear();
        if (kind == 2) {
            const int how = rnd(0, 2);
            r.flag = PAIRED | (rev ? REV : 0) | (rnd(0, 1) ? FIRST : SECOND);
            if (how == 0) { r.mrefid = (chr + 1) % std::max(nchr, 2); r.mpos = rnd(0, 50000); r.flag |= rnd(0, 1) ? MATE_REV : 0; }
            else if (how == 1) { r.mrefid = chr; r.mpos = pos + rnd(0, 3000); r.flag |= rev ? MATE_REV : 0; }  // (same strand)
            else { r.mrefid = chr; r.mpos = pos + (rev ? 1 : -1) * rnd(10, 400); r.flag |= PROPER | (rev ? 0 : MATE_REV); if (r.mpos < 0) r.mpos = 0; if (r.mpos == pos) r.flag &= ~PROPER; }  // (the mate on the wrong side)
        } else {
            r.flag = PAIRED | PROPER | (rev ? REV : MATE_REV) | (rnd(0, 1) ? FIRST : SECOND);
            r.mrefid = chr; r.mpos = rev ? std::max(0, pos - rnd(0, 400)) : pos + rnd(0, 400);
        }
        if (kind == 3) { const int f = rnd(0, 3); if (f == 0) r.mapq = 0; else if (f == 1) r.flag |= DUP; else if (f == 2) r.aux |= SQ_AUX_MULTI; else r.flag |= UNMAPPED; }
        if (rnd(0, 19) == 0) r.aux |= SQ_AUX_LOWPHRED;
        recs.push_back(r);
    };
    int per_chr = std::max(1, want / nchr);
    for (int chr = 0; chr < nchr && (int)recs.size() < want; ++chr) {
        int p = stale && chr > 0 ? rnd(100, 400) : rnd(100, 5000);
        const int target = chr == nchr - 1 ? want : std::min(want, (int)recs.size() + per_chr);
        if (chr > 0 && rnd(0, 1) && (int)recs.size() < target) { one(chr, p, 4, false); ++cs.zero_blocks_at_change; }  // (a record without a block opens the chromosome)
        while ((int)recs.size() < target) {
            const int left = target - (int)recs.size();
            const int shape = rnd(0, 9);
            int len = shape < 2 ? 1 : shape < 8 ? rnd(3, 40) : rnd(70, 130);
            if (cut8 && recs.empty()) len = 8;
            len = std::min(len, left);
            const bool deep = rnd(0, 2) == 0;
            bool in_run = false;
            const int run_from = shape >= 8 ? rnd(0, 10) : -1;  // (a discordant run longer than 64 records)
            const bool end_run = rnd(0, 3) == 0;                // (the island ends inside a discordant run)
            int run_len = 0;
            for (int k = 0; k < len; ++k) {
                const bool rev = rnd(0, 1) != 0;
                int kind;
                if (run_from >= 0 && k >= run_from && k < run_from + 66 + (len % 7)) kind = 2;
                else if (end_run && k >= len - rnd(1, 4)) kind = 2;
                else if (in_run) kind = rnd(0, 9) < 7 ? 2 : rnd(0, 1);
                else { const int x = rnd(0, 99); kind = x < 60 ? 0 : x < 72 ? 1 : x < 90 ? 2 : x < 96 ? 3 : 4; }
                if (cut8 && recs.size() < 8 && kind > 2) kind = 0;
                in_run = kind == 2;
                run_len = in_run ? run_len + 1 : 0;
                if (run_len == 65) ++cs.long_runs;
                one(chr, p, kind, rev);
                if (cut8 && recs.size() <= 5) recs.back().totlen = read - 20 + 4 * (int)recs.size();  // (ReadLen still rises over the first five records)
                if (k + 1 == len && in_run) ++cs.run_at_end;
                p += in_run ? rnd(0, 2) : deep ? rnd(0, 3) : rnd(4, 30);
            }
            if (stale && chr == 0 && (int)recs.size() >= target - 3) p += 0;
            const int gap = rnd(0, 9);
            if (cut8 && recs.size() == 8) { p += 2 * read + 200; ++cs.cut_at_8; }
            else p += gap < 5 ? read + 64 + read + rnd(40, 2000) : gap < 8 ? read + rnd(5, 60) : rnd(0, 20);
        }
        if (stale && chr == 0) {  // a discordant run far to the right closes chromosome 0: its end outlives the chromosome
            const int far = p + 40000;
            const int k = std::min<int>(6, (int)recs.size());
            for (int i = 0; i < k; ++i) { Rec& r = recs[recs.size() - (size_t)k + (size_t)i]; const int d = far + i - r.pos; r.pos += d; for (size_t q = 0; q < r.b.size(); q += 4) r.b[q] += d; r.flag &= ~PROPER; }
            ++cs.stale;
        }
    }
    if (unsorted && recs.size() >= 16) {  // two passing records out of order
        for (int tries = 0; tries < 200 && !cs.planted_unsorted; ++tries) {
            const size_t i = (size_t)rnd(8, (int)recs.size() - 2);
            Rec &x = recs[i], &y = recs[i + 1];
            auto passes = [](const Rec& r) { return r.mapq && !(r.flag & (DUP | UNMAPPED)) && !(r.aux & SQ_AUX_MULTI); };
            if (!passes(x) || !passes(y) || x.refid != y.refid || x.pos == y.pos) continue;
            std::swap(x, y);
            ++cs.planted_unsorted;
        }
    }
    HostBatch& hb = cs.hb;
    hb.blk_off.assign(1, 0); hb.name_off.assign(1, 0);
    for (const Rec& r : recs) {
        hb.refid.push_back(r.refid); hb.pos.push_back(r.pos); hb.mrefid.push_back(r.mrefid); hb.mpos.push_back(r.mpos); hb.endpos.push_back(r.pos);
        hb.flag.push_back((uint16_t)r.flag); hb.totlen.push_back((uint16_t)r.totlen); hb.mapq.push_back((uint8_t)r.mapq); hb.aux.push_back((uint8_t)r.aux);
        for (size_t q = 0; q < r.b.size(); q += 4) { hb.b_refpos.push_back(r.b[q]); hb.b_matchref.push_back(r.b[q + 1]); hb.b_readpos.push_back((uint16_t)r.b[q + 2]); hb.b_matchread.push_back((uint16_t)r.b[q + 3]); }
        hb.blk_off.push_back((uint32_t)hb.b_refpos.size());
        hb.name_off.push_back(0);
    }
    return cs;
}
void write_case(std::FILE* f, const Case& cs, bool fallback) {
    const HostBatch& hb = cs.hb;
    std::fprintf(f, "case %zu %zu %d\n", hb.size(), hb.b_refpos.size(), (int)fallback);
    for (size_t r = 0; r < hb.size(); ++r)
        std::fprintf(f, "%d %d %d %d %d %d %d %d %u\n", hb.refid[r], hb.pos[r], hb.mrefid[r], hb.mpos[r], (int)hb.flag[r], (int)hb.totlen[r], (int)hb.mapq[r], (int)hb.aux[r], hb.blk_off[r + 1] - hb.blk_off[r]);
    for (size_t b = 0; b < hb.b_refpos.size(); ++b) std::fprintf(f, "%d %d %d %d\n", hb.b_refpos[b], hb.b_matchref[b], (int)hb.b_readpos[b], (int)hb.b_matchread[b]);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: bwa_nodes_emu <bwa.bam> [read_len] | --fuzz <cases> <seed> [--write <file>]\n"); return 2; }
    sq_ctx c;
    sq_default_params(&c.P);
    c.pool.reset(new HostPool(3));
    if (!std::strcmp(argv[1], "--fuzz")) {
        if (argc < 4) return 2;
        const int cases = std::atoi(argv[2]);
        std::mt19937_64 rng((uint64_t)std::strtoull(argv[3], nullptr, 10));
        std::FILE* out = argc > 5 && !std::strcmp(argv[4], "--write") ? std::fopen(argv[5], "w") : nullptr;
        long bad = 0, records = 0, seeds = 0, reads = 0, stretches = 0, again = 0, single = 0, longest = 0, flush_nodes = 0, marks = 0, cover_fails = 0, fallbacks = 0, planted = 0, named_sizes = 0, run_at_end = 0,
             long_runs = 0, cut_at_8 = 0, zero_blocks = 0, clipped_fwd = 0, clipped_rev = 0, stale = 0;
        for (int k = 0; k < cases; ++k) {
            Case cs = make_case(rng, k);
            c.read_len = k % 5 == 4 ? 60 : 0;  // (now and then the chimeric file's value is there first)
            Both b;
            const long d = compare(c, cs.hb, b, true);
            if (d) std::printf("case %d (%zu records): %ld differences\n", k, cs.hb.size(), d);
            bad += d;
            if (out) write_case(out, cs, b.fallback);
            planted += cs.planted_unsorted;
            if ((cs.planted_unsorted != 0) != b.fallback) { ++bad; std::printf("case %d: planted %ld, fallback %d (flags %u)\n", k, cs.planted_unsorted, (int)b.fallback, b.flag_word); }
            if (b.fallback) { ++fallbacks; continue; }
            const size_t n = cs.hb.size();
            named_sizes += n == 0 || n == 1 || n == 63 || n == 64 || n == 65 || n == 129;
            records += (long)n; seeds += (long)b.seeds.size(); reads += (long)b.reads; stretches += (long)b.W.stretches; again += (long)b.W.again; single += (long)b.W.single; longest = std::max(longest, (long)b.W.longest);
            flush_nodes += (long)b.W.flush_nodes; marks += (long)b.W.marks_closed; cover_fails += b.cover_fails;
            run_at_end += cs.run_at_end; long_runs += cs.long_runs; cut_at_8 += cs.cut_at_8; zero_blocks += cs.zero_blocks_at_change; clipped_fwd += cs.clipped_fwd; clipped_rev += cs.clipped_rev; stale += cs.stale;
        }
        if (out) std::fclose(out);
        std::printf("%d cases, %ld records, seeds %ld, Reads records %ld, stretches %ld, run again %ld, single-record stretches %ld, longest stretch %ld, flushes that emitted a node %ld, "
                    "marks closed by the zero-coverage rule %ld, cover tests failed %ld, fallback cases %ld (planted unsorted %ld), tables of 0 1 63 64 65 129 records %ld, islands that end in a discordant run %ld, "
                    "discordant runs longer than 64 records %ld, cuts at record 8 %ld, records without a block at a chromosome change %ld, clipped reads forward %ld reverse %ld, stale rightmost tables %ld, %ld differences\n",
                    cases, records, seeds, reads, stretches, again, single, longest, flush_nodes, marks, cover_fails, fallbacks, planted, named_sizes, run_at_end, long_runs, cut_at_8, zero_blocks, clipped_fwd, clipped_rev,
                    stale, bad);
        std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
        return bad ? 1 : 0;
    }
    c.read_len = argc > 2 ? std::atoi(argv[2]) : 0;
    std::vector<std::string> names;
    std::string err;
    if (read_bam_header(argv[1], names, c.ref_len, err)) { std::printf("header: %s\n", err.c_str()); return 1; }
    auto all = std::make_shared<HostBatch>();
    all->blk_off.assign(1, 0); all->name_off.assign(1, 0);
    ParseOpts o{c.P.phred_type, c.P.min_phred, c.P.max_lowphred_len, true, nullptr};
    if (parse_bam_file(argv[1], o, (size_t)1 << 21, 4, err, [&](const HostBatch& hb) { all->append(hb); return 0; })) { std::printf("parse: %s\n", err.c_str()); return 1; }
    c.bwa = all;
    Both b;
    long bad = compare(c, *all, b, true);
    if (b.fallback) { std::printf("   the emulated kernels handed the table back (flags %u)\n", b.flag_word); ++bad; }
    std::printf("%zu records, seeds %zu, Reads records %lld, stretches %lld, run again %lld, single-record stretches %lld, longest stretch %lld, flushes that emitted a node %lld, "
                "marks closed by the zero-coverage rule %lld, cover tests failed %ld, read length %d, %ld differences\n",
                all->size(), b.seeds.size(), (long long)b.reads, (long long)b.W.stretches, (long long)b.W.again, (long long)b.W.single, (long long)b.W.longest, (long long)b.W.flush_nodes, (long long)b.W.marks_closed,
                b.cover_fails, b.read_len, bad);
    std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
    return bad ? 1 : 0;
}
