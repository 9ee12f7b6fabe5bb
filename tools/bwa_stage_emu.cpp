// The --bwa stages of the device route (squid_amd/csrc/sq_bwa_stage.inc: the class byte of every record, the node depth loop as a prefix
// maximum) on the CPU: the kernel source itself -- the class kernel lane by lane, the three depth kernels as waves of 64 coroutines
// (sq_wave.h with SQ_WAVE_EMU) -- against the host loops of the library (sq_bwa.cpp: seed_record_passes, decide() of the breakpoint
// support, the depth loop; linked against libsquid_hip.so, no device needed).  Compared: both class bits of every record, Support and
// the integer sum of every node, the fallback flag; the held blocks (m != g, ledger W6) against a plain count made here.
//   bwa_stage_emu <bwa.bam> [min_mapqual]                       BuildNode_BWA / RawEdges by the library's host code, then both routes
//   bwa_stage_emu --fuzz <cases> <seed> [--write <file>]        random tables (see make_case); --write keeps the cases as numbers for
//                                                               the device test (sq_debug_bwa_depth)
//   bwa_stage_emu --fuzz-long <seed> [--write <file>]           the tables of LONG_SPECS: Reads lists around one and two rounds of depth_prefix
//                                                               (64 tiles = 65 536 blocks), which the tables of --fuzz (five tiles) never reach
#include "../squid_amd/csrc/sq_internal.h"
#include "../squid_amd/csrc/sq_bwa_stage.inc"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
using namespace sq;

namespace {
struct NodeTab {
    std::vector<int32_t> chr, pos, len, chr_start, fine, fine_off;
    bws::Nodes N;
    // with_fine: the position index dev_upload_nodes / k_node_buckets make (ref_len per chromosome), else plain bisection
    void make(const std::vector<int32_t>& nodes3, int n_ref, bool with_fine, const std::vector<int32_t>& ref_len) {
        const int n = (int)(nodes3.size() / 3);
        for (int i = 0; i < n; ++i) { chr.push_back(nodes3[3 * (size_t)i]); pos.push_back(nodes3[3 * (size_t)i + 1]); len.push_back(nodes3[3 * (size_t)i + 2]); }
        chr_start.assign((size_t)n_ref + 1, n);
        { int j = 0; for (int k = 0; k <= n_ref; ++k) { while (j < n && chr[(size_t)j] < k) ++j; chr_start[(size_t)k] = j; } }
        chr.push_back(0); pos.push_back(0); len.push_back(0);  // (never empty)
        N.n = n; N.n_ref = n_ref; N.chr = chr.data(); N.pos = pos.data(); N.len = len.data(); N.chr_start = chr_start.data(); N.fine = nullptr; N.fine_off = nullptr;
        if (!with_fine) return;
        fine_off.assign((size_t)n_ref + 1, 0);
        for (int k = 0; k < n_ref; ++k) fine_off[(size_t)k + 1] = fine_off[(size_t)k] + ((std::max(ref_len[(size_t)k], 1) + (1 << NODE_FINE_SHIFT) - 1) >> NODE_FINE_SHIFT) + 1;
        fine.assign((size_t)fine_off[(size_t)n_ref] + 1, 0);
        for (int k = 0; k < n_ref; ++k)
            for (int g = fine_off[(size_t)k]; g < fine_off[(size_t)k + 1]; ++g) {
                if (g == fine_off[(size_t)k + 1] - 1) { fine[(size_t)g] = chr_start[(size_t)k + 1] - 1; continue; }
                const int p = (g - fine_off[(size_t)k]) << NODE_FINE_SHIFT;
                int lo = chr_start[(size_t)k], hi = chr_start[(size_t)k + 1];
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pos[(size_t)mid] <= p) lo = mid; else hi = mid; }
                fine[(size_t)g] = lo;
            }
        N.fine = fine.data(); N.fine_off = fine_off.data();
    }
};
struct DepthOut { std::vector<int32_t> cnt, sum; long held = 0; bool fallback = false; };
struct WaveArg { const bws::Nodes* N; const bws::Blocks* B; int64_t tile, ntiles; int32_t *tmax, *front; uint32_t *support, *sum, *counters; };
void lane_max(void* p) { const WaveArg& a = *(const WaveArg*)p; bws::depth_tile_max(*a.N, *a.B, a.tile, a.tmax); }
void lane_prefix(void* p) { const WaveArg& a = *(const WaveArg*)p; bws::depth_prefix(a.ntiles, a.tmax, a.front); }
void lane_apply(void* p) { const WaveArg& a = *(const WaveArg*)p; bws::depth_tile_apply(*a.N, *a.B, a.tile, a.front, a.support, a.sum, a.counters); }
// the three launches of dev_bwa_node_depth; the tiles are visited from the last to the first (a tile that needed another tile's work would show)
DepthOut depth_emulated(const bws::Nodes& N, const std::vector<int32_t>& blk_chr, const std::vector<uint32_t>& pack) {
    DepthOut r;
    const size_t nn = (size_t)N.n;
    const int64_t nb = (int64_t)blk_chr.size() - 1, ntiles = (nb + bws::TILE_BLOCKS - 1) / bws::TILE_BLOCKS;  // (the arrays carry one spare element)
    std::vector<uint32_t> acc(2 * nn + 2, 0);
    std::vector<int32_t> tmax(2 * (size_t)ntiles + 2, 0), front(2 * (size_t)ntiles + 2, 0);
    const bws::Blocks B{nb, blk_chr.data(), pack.data()};
    WaveArg a{&N, &B, 0, ntiles, tmax.data(), front.data(), acc.data(), acc.data() + nn, acc.data() + 2 * nn};
    for (int64_t t = ntiles; t-- > 0;) { a.tile = t; wv::run_wave(lane_max, &a); }
    if (ntiles) wv::run_wave(lane_prefix, &a);
    for (int64_t t = ntiles; t-- > 0;) { a.tile = t; wv::run_wave(lane_apply, &a); }
    r.cnt.assign(nn, 0); r.sum.assign(nn, 0);
    for (size_t i = 0; i < nn; ++i) { r.cnt[i] = (int32_t)acc[i]; r.sum[i] = (int32_t)acc[nn + i]; }
    r.held = (long)acc[2 * nn + bws::CNT_HELD];
    r.fallback = acc[2 * nn + bws::CNT_DECREASING] != 0;
    return r;
}
// g, its prefix maximum and the held blocks by plain loops over the definition (g by a search of the standard library over the whole table)
struct Plain { long held = 0; bool decreasing = false; std::vector<int> g, m; };
Plain plain_held(const std::vector<int32_t>& nodes3, const std::vector<int32_t>& reads3) {
    Plain r;
    const int n = (int)(nodes3.size() / 3);
    int run = -1, cmax = -1;
    for (size_t j = 0; j < reads3.size() / 3; ++j) {
        const int c = reads3[3 * j], p = reads3[3 * j + 1];
        // (the first node that is not in front of (c, p): on an earlier chromosome, or on c and ending at or before p)
        int lo = 0, hi = n;
        while (lo < hi) { const int i = (lo + hi) / 2; if (nodes3[3 * (size_t)i] < c || (nodes3[3 * (size_t)i] == c && nodes3[3 * (size_t)i + 1] + nodes3[3 * (size_t)i + 2] <= p)) lo = i + 1; else hi = i; }
        const int g = lo < n && nodes3[3 * (size_t)lo] == c ? lo : n;
        if (c < cmax) r.decreasing = true;
        cmax = std::max(cmax, c);
        run = std::max(run, g);
        if (run != g) ++r.held;
        r.g.push_back(g); r.m.push_back(run);
    }
    return r;
}

// ---- fuzz
const int LENGTHS[] = {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500, 3300, 5000};
struct Case {
    std::vector<int32_t> nodes3, reads3, ref_len;
    int n_ref = 0;
    bool one_per_chr = false, tiny = false, single = false, empty_chr = false, far_tile = false, dead_tail = false, decreasing = false;
    long exact_end = 0, one_beyond = 0, one_before = 0;
};
// what make_table is asked for.  style: 0 random tiling, 1 one node per chromosome, 2 nodes of 1-4 bases, 3 short nodes under dense blocks, 4 one
// node takes every block.  far_tile: the last block of tile `far_at` stands near the chromosome's end and the two tiles behind it lie in front of it.
// dead_tail: block `plant_at` (-1: the middle one) lies beyond the last node of its chromosome.  decreasing: block `plant_at` (-1: one of the
// last 40) lies on the first chromosome, behind a block of a later one.  scale: the chromosomes' lengths times this.
// few_introns (the long tables): two records in a thousand are spliced, their introns a tenth as long, and no block behind an intron lies beyond the
// chromosome -- with the rates of the short tables a list of 65 536 blocks has a block that nothing consumes near its start and counts nothing behind it
struct Spec { int want, style; bool far_tile, dead_tail, decreasing; long far_at, plant_at; int scale; bool few_introns; };
Case make_table(std::mt19937_64& rng, const Spec& sp) {
    Case cs;
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int want = sp.want, style = sp.style;
    cs.far_tile = sp.far_tile; cs.dead_tail = sp.dead_tail; cs.decreasing = sp.decreasing;
    const int nchr = cs.far_tile || style == 4 ? 2 : rnd(3, 5);
    const int skip = nchr >= 3 ? rnd(1, nchr - 2) : -1;  // a chromosome between two used ones that no block lies on
    cs.empty_chr = skip >= 0 && want >= 2;
    cs.one_per_chr = style == 1; cs.tiny = style == 2; cs.single = style == 4;
    cs.n_ref = nchr;
    std::vector<std::vector<int>> first((size_t)nchr);  // node index range per chromosome
    for (int ch = 0; ch < nchr; ++ch) {
        const int L = sp.scale * (style == 2 ? rnd(300, 700) : style == 3 ? rnd(1500, 2500) : rnd(3000, 9000));
        int p = 0;
        while (p < L) {
            int len;
            if (style == 1 || style == 4) len = L;
            else if (style == 2) len = rnd(1, 4);
            else if (style == 3) len = rnd(2, 9);
            else len = rnd(0, 9) == 0 ? rnd(1, 4) : rnd(15, 260);
            first[(size_t)ch].push_back((int)(cs.nodes3.size() / 3));
            cs.nodes3.push_back(ch); cs.nodes3.push_back(p); cs.nodes3.push_back(len);
            p += len;
        }
        cs.ref_len.push_back(p);
    }
    // records in coordinate order per chromosome; a record has one to three blocks, the later ones behind an intron (what holds the cursor)
    std::vector<int> used;
    for (int ch = 0; ch < nchr; ++ch) if (ch != skip && !(cs.single && ch != 0) && !(cs.far_tile && ch != 0)) used.push_back(ch);
    struct Rec { int pos; std::vector<std::pair<int, int>> blk; };
    int made = 0;
    for (size_t u = 0; u < used.size() && made < want; ++u) {
        const int ch = used[u], L = cs.ref_len[(size_t)ch];
        const int share = u + 1 == used.size() ? want - made : std::max(1, (want - made) / (int)(used.size() - u));
        std::vector<Rec> recs;
        int blocks = 0;
        while (blocks < share) {
            Rec r;
            const std::vector<int>& nd = first[(size_t)ch];
            const int i = nd[(size_t)rnd(0, (int)nd.size() - 1)], np = cs.nodes3[3 * (size_t)i + 1], nl = cs.nodes3[3 * (size_t)i + 2];
            const int kind = rnd(0, 99);
            int p, len;
            if (kind < 15) { len = rnd(1, std::min(nl, 40)); p = np + nl - len; ++cs.exact_end; }             // ends exactly at the node's end
            else if (kind < 27) { len = rnd(1, std::min(nl, 40)) + 1; p = np + nl + 1 - len; ++cs.one_beyond; }  // ends one base beyond
            else if (kind < 39) { p = np - 1; len = rnd(1, std::max(1, std::min(nl, 40))); if (p < 0) p = 0; else ++cs.one_before; }  // starts one base before
            else if (kind < 75) { len = rnd(1, std::min(nl, 60)); p = np + rnd(0, nl - len); }                  // inside
            else { p = rnd(0, L - 1); len = rnd(1, 80); }                                                       // anywhere, over the end included
            r.pos = p;
            r.blk.push_back(std::make_pair(p, len));
            const int extra = (sp.few_introns ? rnd(0, 999) < 2 : rnd(0, 99) < (style == 3 ? 1 : 2)) ? rnd(1, 2) : 0;
            int at = p + len;
            for (int k = 0; k < extra && blocks + (int)r.blk.size() < share; ++k) {
                at += sp.few_introns ? rnd(L / 400, L / 100) : rnd(L / 40, L / 10);
                const int l2 = rnd(5, 60);
                if (sp.few_introns && at + l2 > L) break;
                r.blk.push_back(std::make_pair(at, l2)); at += l2;  // (may lie behind the last node)
            }
            blocks += (int)r.blk.size();
            recs.push_back(r);
        }
        std::stable_sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.pos < y.pos; });
        for (const Rec& r : recs) for (const auto& b : r.blk) { cs.reads3.push_back(ch); cs.reads3.push_back(b.first); cs.reads3.push_back(b.second); }
        made += blocks;
    }
    const size_t nr = cs.reads3.size() / 3;
    if (cs.far_tile) {  // the last block of tile far_at stands near the chromosome's end; the blocks of the next tiles (and those in front) lie in front of it
        const size_t upto = ((size_t)sp.far_at + 3) * (size_t)bws::TILE_BLOCKS;
        if (nr < upto) cs.far_tile = false;
        else {
            // (the later blocks of spliced records are pulled in so that nothing up to there reaches the far block's node)
            const int L = cs.ref_len[0], far = L - 2;
            for (size_t j = 0; j < upto; ++j) if (cs.reads3[3 * j + 1] >= L * 3 / 5) cs.reads3[3 * j + 1] = rnd(L / 5, L * 3 / 5 - 1);
            const size_t j = ((size_t)sp.far_at + 1) * (size_t)bws::TILE_BLOCKS - 1;
            cs.reads3[3 * j] = 0; cs.reads3[3 * j + 1] = far; cs.reads3[3 * j + 2] = 1;
        }
    }
    if (cs.dead_tail && nr >= 8) {  // a block beyond the last node of its chromosome, in the middle of the list
        const size_t j = sp.plant_at < 0 ? nr / 2 : (size_t)sp.plant_at;
        cs.reads3[3 * j + 1] = cs.ref_len[(size_t)cs.reads3[3 * j]] + rnd(0, 50);
    } else cs.dead_tail = false;
    if (cs.decreasing && nr >= 2 && cs.reads3[0] != cs.reads3[3 * (nr - 1)]) {  // a block of the first chromosome behind a block of a later one
        const size_t j = sp.plant_at >= 0 ? (size_t)sp.plant_at : nr - 1 - (size_t)rnd(0, (int)std::min<size_t>(nr / 3, 40));
        if (j >= 1 && cs.reads3[3 * (j - 1)] != cs.reads3[0]) { cs.reads3[3 * j] = cs.reads3[0]; cs.reads3[3 * j + 1] = rnd(0, cs.ref_len[(size_t)cs.reads3[0]] - 1); } else cs.decreasing = false;
    } else cs.decreasing = false;
    return cs;
}
Case make_case(std::mt19937_64& rng, int index) {
    Spec sp;
    sp.want = LENGTHS[index % (int)(sizeof LENGTHS / sizeof *LENGTHS)];
    sp.far_tile = sp.want >= 3300 && index % 3 == 0;
    sp.style = sp.far_tile ? (index % 2 ? 3 : 0) : (index / 2) % 5;
    sp.dead_tail = !sp.far_tile && sp.want >= 63 && index % 4 == 1;
    sp.decreasing = !sp.far_tile && !sp.dead_tail && sp.want >= 2 && index % 7 == 2;
    sp.far_at = 0; sp.plant_at = -1; sp.scale = 1; sp.few_introns = false;
    return make_table(rng, sp);
}
// ---- the long tables.  depth_prefix walks the tiles in rounds of 64 (ROUND blocks) and carries the two running maxima from round to round:
// lists one block short of a round, exactly one and two rounds, and one block into the second and the third round; random tiling and short
// nodes under dense blocks.  The specials put the value that must cross a round where only the carry brings it: a far block as the last block of
// the first round that holds the first two tiles of the second, a block beyond the last node (g = n_nodes: nothing behind it is counted) in the
// last tile of the first round, and one inside the second round of a list that reaches into the third; and for the other maximum a block of the
// first chromosome as the only block of the second round, behind a round of later chromosomes (the flag that sends the case to the host loop)
constexpr long ROUND = 64l * bws::TILE_BLOCKS;
const Spec LONG_SPECS[] = {
    {(int)ROUND - 1, 0, false, false, false, 0, -1, 20, true},
    {(int)ROUND, 3, false, false, false, 0, -1, 20, true},
    {(int)ROUND + 1, 0, false, false, false, 0, -1, 20, true},
    {2 * (int)ROUND, 3, true, false, false, 63, -1, 20, true},
    {2 * (int)ROUND + 1, 0, false, true, false, 0, ROUND + 10 * bws::TILE_BLOCKS + 5, 20, true},
    {2 * (int)ROUND, 0, false, true, false, 0, ROUND - 500, 20, true},
    {(int)ROUND + 1, 3, false, false, false, 0, -1, 20, true},
    {(int)ROUND + 1, 0, false, false, true, 0, ROUND, 20, true},
};
void write_case(std::FILE* f, const Case& cs) {
    std::fprintf(f, "case %zu %zu\n", cs.nodes3.size() / 3, cs.reads3.size() / 3);
    for (size_t i = 0; i < cs.nodes3.size(); i += 3) std::fprintf(f, "%d %d %d\n", cs.nodes3[i], cs.nodes3[i + 1], cs.nodes3[i + 2]);
    for (size_t i = 0; i < cs.reads3.size(); i += 3) std::fprintf(f, "%d %d %d\n", cs.reads3[i], cs.reads3[i + 1], cs.reads3[i + 2]);
}
// both routes on one pair of tables; returns the differences.  The emulated route that raises the flag hands the case to the host loop,
// as the library does (its result is then route 0's by construction: what is compared is the flag)
long compare_depth(const std::vector<int32_t>& nodes3, int n_ref, const std::vector<int32_t>& ref_len, bool with_fine, const std::vector<int32_t>& reads3, bool expect_fallback, long& held, long& counted, bool say) {
    NodeTab nt;
    nt.make(nodes3, n_ref, with_fine, ref_len);
    const size_t nr = reads3.size() / 3;
    std::vector<int32_t> blk_chr(nr + 1, -1);
    std::vector<uint32_t> pack(4 * (nr + 1), 0);
    for (size_t j = 0; j < nr; ++j) { blk_chr[j] = reads3[3 * j]; pack[4 * j] = (uint32_t)reads3[3 * j + 1]; pack[4 * j + 1] = (uint32_t)reads3[3 * j + 2]; }
    const DepthOut d = depth_emulated(nt.N, blk_chr, pack);
    std::vector<int32_t> cnt, sum;
    bwa_node_depth_flat(nt.N.n, nodes3.data(), (int64_t)nr, reads3.data(), cnt, sum);
    long bad = 0;
    if (d.fallback != expect_fallback) { ++bad; if (say) std::printf("   fallback flag %d, expected %d\n", (int)d.fallback, (int)expect_fallback); }
    held = 0; counted = 0;
    if (d.fallback) return bad;
    for (int32_t v : cnt) counted += v;
    for (size_t i = 0; i < cnt.size(); ++i)
        if (cnt[i] != d.cnt[i] || sum[i] != d.sum[i]) { if (say && bad < 10) std::printf("   node %zu (%d %d %d): host %d / %d, emulated %d / %d\n", i, nodes3[3 * i], nodes3[3 * i + 1], nodes3[3 * i + 2], cnt[i], sum[i], d.cnt[i], d.sum[i]); ++bad; }
    const Plain pl = plain_held(nodes3, reads3);
    if (pl.held != d.held) { ++bad; if (say) std::printf("   held blocks: %ld by the definition, %ld emulated\n", pl.held, d.held); }
    held = d.held;
    return bad;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: bwa_stage_emu <bwa.bam> [min_mapqual] | --fuzz <cases> <seed> [--write <file>] | --fuzz-long <seed> [--write <file>]\n"); return 2; }
    if (!std::strcmp(argv[1], "--fuzz-long")) {
        if (argc < 3) return 2;
        std::mt19937_64 rng((uint64_t)std::strtoull(argv[2], nullptr, 10));
        std::FILE* out = argc > 4 && !std::strcmp(argv[3], "--write") ? std::fopen(argv[4], "w") : nullptr;
        const int cases = (int)(sizeof LONG_SPECS / sizeof *LONG_SPECS);
        long bad = 0, blocks = 0, held = 0, counted = 0;
        int far_round = 0, dead_round = 0, dead_second = 0, random_tiling = 0, dense = 0, down_round = 0;
        for (int k = 0; k < cases; ++k) {
            const Spec& sp = LONG_SPECS[k];
            Case cs = make_table(rng, sp);
            if (out) write_case(out, cs);
            const size_t nr = cs.reads3.size() / 3, T = (size_t)bws::TILE_BLOCKS;
            const int nn = (int)(cs.nodes3.size() / 3);
            const Plain pl = plain_held(cs.nodes3, cs.reads3);
            long b = 0, h = 0, cn = 0;
            if ((long)nr != sp.want) { ++b; std::printf("   case %d: %zu blocks, asked for %d\n", k, nr, sp.want); }
            if (pl.decreasing != sp.decreasing || cs.decreasing != sp.decreasing) { ++b; std::printf("   case %d: the chromosome order along Reads is not what was asked for\n", k); }
            b += compare_depth(cs.nodes3, cs.n_ref, cs.ref_len, k % 2 == 1, cs.reads3, sp.decreasing, h, cn, true);
            // what the specials promise, checked on the tables themselves
            if (sp.decreasing) {  // the first block whose chromosome is smaller than one in front of it is the first block of a round, and its tile holds nothing else
                size_t first = 1;
                for (int cmax = cs.reads3[0]; first < nr && cs.reads3[3 * first] >= cmax; ++first) cmax = cs.reads3[3 * first];
                if (first == (size_t)sp.plant_at && first % (size_t)ROUND == 0 && first + 1 == nr) ++down_round; else { ++b; std::printf("   case %d: no chromosome going down at the first block of a round (first %zu)\n", k, first); }
            }
            if (sp.far_tile) {  // the last block of the first round holds every block of the first two tiles of the second
                const size_t far = ((size_t)sp.far_at + 1) * T - 1;
                bool ok = cs.far_tile && (long)far == ROUND - 1;
                for (size_t j = far + 1; ok && j <= far + 2 * T; ++j) ok = pl.m[j] != pl.g[j] && pl.m[j] == pl.g[far] && pl.m[j] < nn;
                if (ok) ++far_round; else { ++b; std::printf("   case %d: the far block does not hold two tiles of the second round\n", k); }
            }
            if (sp.dead_tail) {  // the first block nothing consumes is the planted one, with counted blocks in front of it and blocks of a later round behind it
                size_t first = 0;
                while (first < nr && pl.m[first] != nn) ++first;
                const bool ok = cs.dead_tail && first == (size_t)sp.plant_at && cn > 0 && first / (size_t)ROUND < (nr - 1) / (size_t)ROUND;
                if (ok) { ++dead_round; dead_second += first / (size_t)ROUND == 1; } else { ++b; std::printf("   case %d: no block beyond the last node in front of a later round (first %zu)\n", k, first); }
            }
            random_tiling += sp.style == 0; dense += sp.style == 3;
            if (b) std::printf("case %d: %ld differences\n", k, b);
            bad += b; blocks += (long)nr; held += h; counted += cn;  // (a fallback case adds its blocks and nothing else)
            std::printf("long case %d: %zu nodes, %zu blocks, held %ld, counted %ld, fallback %d\n", k, (size_t)nn, nr, h, cn, (int)sp.decreasing);
        }
        if (out) std::fclose(out);
        std::printf("%d long cases, %ld blocks, held %ld, counted %ld, random tiling %d, short nodes under dense blocks %d, far block holds two tiles of the next round %d, "
                    "block beyond the last node in front of a later round %d (inside the second round %d), chromosome going down at the first block of a round %d\n",
                    cases, blocks, held, counted, random_tiling, dense, far_round, dead_round, dead_second, down_round);
        std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
        return bad ? 1 : 0;
    }
    if (!std::strcmp(argv[1], "--fuzz")) {
        if (argc < 4) return 2;
        const int cases = std::atoi(argv[2]);
        std::mt19937_64 rng((uint64_t)std::strtoull(argv[3], nullptr, 10));
        std::FILE* out = argc > 5 && !std::strcmp(argv[4], "--write") ? std::fopen(argv[5], "w") : nullptr;
        long bad = 0, blocks = 0, held = 0, counted = 0, exact_end = 0, one_beyond = 0, one_before = 0;
        int one_per_chr = 0, tiny = 0, single = 0, empty_chr = 0, far_tile = 0, dead_tail = 0, fallbacks = 0, dense = 0, lengths = 0;
        unsigned long seen_len = 0;
        for (int k = 0; k < cases; ++k) {
            Case cs = make_case(rng, k);
            if (out) write_case(out, cs);
            const size_t nr = cs.reads3.size() / 3;
            const Plain pl = plain_held(cs.nodes3, cs.reads3);
            long b = 0, h = 0, cn = 0;
            if (pl.decreasing != cs.decreasing) { ++b; std::printf("   case %d: the generator's chromosome order is not what it says\n", k); }
            b += compare_depth(cs.nodes3, cs.n_ref, cs.ref_len, k % 2 == 1, cs.reads3, cs.decreasing, h, cn, true);
            if (b) std::printf("case %d: %ld differences\n", k, b);
            bad += b;
            // what the generator promises, checked on the tables themselves
            if (cs.far_tile) {  // every block of the two tiles behind the far block is held by it
                bool ok = nr >= 3 * (size_t)bws::TILE_BLOCKS;
                for (size_t j = (size_t)bws::TILE_BLOCKS; ok && j < 3 * (size_t)bws::TILE_BLOCKS; ++j) ok = pl.m[j] != pl.g[j] && pl.m[j] == pl.g[(size_t)bws::TILE_BLOCKS - 1];
                if (ok) ++far_tile; else { ++bad; std::printf("case %d: the far block does not hold two tiles\n", k); }
            }
            if (cs.dead_tail) { if (pl.m[nr / 2] == (int)(cs.nodes3.size() / 3) && nr / 2 + 1 < nr) ++dead_tail; else { ++bad; std::printf("case %d: no block beyond the last node\n", k); } }
            for (size_t j = 0; j + 64 <= nr; j += 64) { int lo = INT32_MAX, hi = -1; for (size_t q = j; q < j + 64; ++q) if (pl.g[q] < (int)(cs.nodes3.size() / 3)) { lo = std::min(lo, pl.g[q]); hi = std::max(hi, pl.g[q]); } if (hi >= 0) dense = std::max(dense, hi - lo + 1); }
            if (cs.decreasing) ++fallbacks; else { blocks += (long)nr; held += h; counted += cn; }
            one_per_chr += cs.one_per_chr; tiny += cs.tiny; single += cs.single; empty_chr += cs.empty_chr;
            exact_end += cs.exact_end; one_beyond += cs.one_beyond; one_before += cs.one_before;
            for (size_t q = 0; q < sizeof LENGTHS / sizeof *LENGTHS; ++q) if ((int)nr == LENGTHS[q] && !((seen_len >> q) & 1)) { seen_len |= 1ul << q; ++lengths; }
        }
        if (out) std::fclose(out);
        std::printf("%d cases, %ld blocks, held %ld (share %.3f), counted %ld, %d of %zu list lengths, one node per chromosome %d, nodes of 1-4 bases %d, one node takes every block %d, "
                    "empty chromosome between used ones %d, most nodes under one wave %d, exact end %ld, one beyond %ld, one before %ld, far block holds two tiles %d, "
                    "block beyond the last node %d, fallback cases %d\n",
                    cases, blocks, held, blocks ? (double)held / blocks : 0.0, counted, lengths, sizeof LENGTHS / sizeof *LENGTHS, one_per_chr, tiny, single, empty_chr, dense, exact_end, one_beyond, one_before,
                    far_tile, dead_tail, fallbacks);
        std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
        return bad ? 1 : 0;
    }
    sq_ctx c;
    sq_default_params(&c.P);
    c.P.min_mapqual = argc > 2 ? std::atoi(argv[2]) : 1;
    c.pool.reset(new HostPool(3));
    std::vector<std::string> names;
    std::string err;
    if (read_bam_header(argv[1], names, c.ref_len, err)) { std::printf("header: %s\n", err.c_str()); return 1; }
    auto all = std::make_shared<HostBatch>();
    all->blk_off.assign(1, 0); all->name_off.assign(1, 0);
    ParseOpts o{c.P.phred_type, c.P.min_phred, c.P.max_lowphred_len, true, nullptr};
    if (parse_bam_file(argv[1], o, (size_t)1 << 21, 4, err, [&](const HostBatch& hb) { all->append(hb); return 0; })) { std::printf("parse: %s\n", err.c_str()); return 1; }
    c.bwa = all;
    const HostBatch& hb = *all;
    std::vector<Edge> raw;
    if (bwa_nodes_and_edges(&c, raw)) { std::printf("host stages: %s\n", c.err.c_str()); return 1; }  // (nodes with the host loop's Support / AvgDepth, the rebuilt fragments' names)
    const size_t nrec = hb.size(), nblk = hb.b_refpos.size();
    // the host's bytes
    std::vector<uint8_t> h_reads, h_look, h_names;
    bwa_reads_bytes(hb, h_reads); bwa_look_bytes(&c, h_look); bwa_name_bytes(&c, h_names);
    // the class kernel, lane by lane from the last record to the first: READS first (with the chromosome per block), then both bits behind the name test
    const RecCols R = hb.cols();
    std::vector<uint8_t> cls(nrec + 1, 0xff);
    std::vector<int32_t> blk_chr(nblk + 1, -2);
    long bad = 0, n_reads = 0, n_p3 = 0, n_named = 0, n_left = 0, n_below = 0;
    for (int64_t r = (int64_t)nrec; r-- > 0;) bws::classify(R, c.P.min_mapqual, nullptr, cls.data(), blk_chr.data(), r);
    for (size_t r = 0; r < nrec; ++r) {
        if (((cls[r] & C_READS) != 0) != (h_reads[r] != 0)) { if (bad < 10) std::printf("   record %zu: READS bit %d, host %d\n", r, (cls[r] & C_READS) != 0, (int)h_reads[r]); ++bad; }
        for (uint32_t b = hb.blk_off[r]; b < hb.blk_off[r + 1]; ++b) if (blk_chr[b] != (h_reads[r] ? hb.refid[r] : -1)) { if (bad < 10) std::printf("   block %u: chromosome %d\n", b, blk_chr[b]); ++bad; }
    }
    for (int64_t r = (int64_t)nrec; r-- > 0;) bws::classify(R, c.P.min_mapqual, h_names.data(), cls.data(), nullptr, r);
    for (size_t r = 0; r < nrec; ++r) {
        const bool reads = (cls[r] & C_READS) != 0, p3 = (cls[r] & C_P3) != 0;
        if (reads != (h_reads[r] != 0) || p3 != (h_look[r] != 0) || (cls[r] & ~(C_READS | C_P3))) { if (bad < 10) std::printf("   record %zu: class %d, host READS %d / look %d\n", r, (int)cls[r], (int)h_reads[r], (int)h_look[r]); ++bad; }
        n_reads += reads; n_p3 += p3; n_named += h_names[r];
        // of the host's READS records: the middle class (MAPQ below -mq: feeds Reads, not looked at by the breakpoint support), and the left-hand
        // records of a pair among the others
        if (h_reads[r] && hb.mapq[r] < c.P.min_mapqual) ++n_below;
        else if (h_reads[r] && !(hb.flag[r] & 0x8) && hb.mrefid[r] == hb.refid[r] && (hb.mpos[r] > hb.pos[r] || (hb.mpos[r] == hb.pos[r] && (hb.flag[r] & 0x80)))) ++n_left;
    }
    // the depth kernels over the block arrays against the nodes of the host loop, and against the loop on the flat Reads list
    std::vector<int32_t> nodes3, reads3;
    for (const Node& n : c.nodes) { nodes3.push_back(n.chr); nodes3.push_back(n.pos); nodes3.push_back(n.len); }
    for (size_t r = 0; r < nrec; ++r) if (h_reads[r]) for (uint32_t b = hb.blk_off[r]; b < hb.blk_off[r + 1]; ++b) { reads3.push_back(hb.refid[r]); reads3.push_back(hb.b_refpos[b]); reads3.push_back(hb.b_matchref[b]); }
    NodeTab nt;
    nt.make(nodes3, (int)c.ref_len.size(), true, c.ref_len);
    std::vector<uint32_t> pack(4 * (nblk + 1), 0);
    for (size_t b = 0; b < nblk; ++b) { pack[4 * b] = (uint32_t)hb.b_refpos[b]; pack[4 * b + 1] = (uint32_t)hb.b_matchref[b]; pack[4 * b + 2] = (uint32_t)hb.b_readpos[b] | ((uint32_t)hb.b_matchread[b] << 16); }
    const DepthOut d = depth_emulated(nt.N, blk_chr, pack);
    std::vector<int32_t> cnt, sum;
    bwa_node_depth_flat(nt.N.n, nodes3.data(), (int64_t)(reads3.size() / 3), reads3.data(), cnt, sum);
    if (d.fallback) { std::printf("   the emulated route raised the fallback flag on a sorted file\n"); ++bad; }
    for (size_t i = 0; i < c.nodes.size() && !d.fallback; ++i) {
        const Node& n = c.nodes[i];
        if (d.cnt[i] != n.support || 1.0 * d.sum[i] / n.len != n.depth || d.cnt[i] != cnt[i] || d.sum[i] != sum[i]) {
            if (bad < 10) std::printf("   node %zu (%d %d %d): host Support %d AvgDepth %g (loop on the flat list %d / %d), emulated %d / %d\n", i, n.chr, n.pos, n.len, n.support, n.depth, cnt[i], sum[i], d.cnt[i], d.sum[i]);
            ++bad;
        }
    }
    const Plain pl = plain_held(nodes3, reads3);
    if (pl.held != d.held) { std::printf("   held blocks: %ld by the definition, %ld emulated\n", pl.held, d.held); ++bad; }
    std::printf("%zu records, %zu blocks, READS records %ld (%zu blocks in Reads), breakpoint-support records %ld, records named like a rebuilt fragment %ld of %zu names, %zu nodes, held blocks %ld, "
                "left-hand READS records %ld, READS records below -mq %d: %ld\n",
                nrec, nblk, n_reads, reads3.size() / 3, n_p3, n_named, c.chim_names.size(), c.nodes.size(), d.held, n_left, c.P.min_mapqual, n_below);
    std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
    return bad ? 1 : 0;
}
