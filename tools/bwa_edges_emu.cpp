// RawEdges' BAM loop of the --bwa device route (squid_amd/csrc/sq_bwa_edges.inc: the fragment table made from the records, the position chain
// of sq_chim_stage.inc over it, the per-record edge kernel, the three lists compacted in record order) on the CPU: the kernel source itself
// (sq_wave.h with SQ_WAVE_EMU; every body is lane-local, so a body is called once per lane index, from the last index to the first -- a
// result that depended on another lane's work would show -- and the scans of dev_bwa_raw_edges are plain loops) against the host loop of the
// library in one go (bwa_raw_edges_debug route 0; linked against libsquid_hip.so, no device needed).  Compared: the summed (key, weight) list,
// the three lists in order, the would-be edges of the listed second mates, the position behind the last record, the number of emitted edges.
//   bwa_edges_emu <bwa.bam> [min_mapqual]                       nodes by the library's host code (BuildNode_BWA), then both routes
//   bwa_edges_emu --fuzz <cases> <seed> [--write <file>]        random node tilings and record tables (see make_case); --write keeps the cases as
//                                                               numbers for the device test (sq_debug_bwa_raw_edges_tables)
#include "../squid_amd/csrc/sq_internal.h"
#include "../squid_amd/csrc/sq_bwa_edges.inc"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
using namespace sq;

namespace {
struct Emulated {
    bool tie = false, assert_ = false;
    std::vector<unsigned long long> keys, second_keys;
    std::vector<int32_t> weights;
    std::vector<uint32_t> part, first_dis, second;
    int32_t final_pos = 0;
    long n_emitted = 0, n_soft = 0, soft_runs = 0, longest_run = 0, kind1 = 0, kind2 = 0, blocks = 0;
};
// dev_bwa_raw_edges, step by step
Emulated emulate(const HostBatch& hb, const std::vector<Node>& nodes, const chs::Params& P) {
    Emulated r;
    const int64_t nf = (int64_t)hb.size();
    if (nf == 0 || nodes.empty()) return r;
    std::vector<int32_t> nchr, npos, nlen;
    for (const Node& n : nodes) { nchr.push_back(n.chr); npos.push_back(n.pos); nlen.push_back(n.len); }
    const chs::Nodes N{(int32_t)nodes.size(), nchr.data(), npos.data(), nlen.data()};
    const RecCols R = hb.cols();
    std::vector<uint8_t> meta((size_t)nf, 0xff), bits((size_t)nf, 0xff), low((size_t)nf, 0), cls((size_t)nf + 1, 0);
    std::vector<int32_t> cnt((size_t)nf, -1), atot((size_t)nf, 0), btot((size_t)nf, 0);
    std::vector<uint32_t> off((size_t)nf + 1, 0), na((size_t)nf, 0);
    uint32_t flags[16] = {0};
    for (int64_t q = nf; q-- > 0;) bwe::count_record(R, meta.data(), cnt.data(), flags + 11, q);
    if (flags[11] & bwe::FLAG_TIE) { r.tie = true; return r; }
    for (int64_t q = 0; q < nf; ++q) off[(size_t)q + 1] = off[(size_t)q] + (uint32_t)cnt[(size_t)q];
    const size_t nblk = off[(size_t)nf];
    r.blocks = (long)nblk;
    std::vector<int32_t> refid(nblk + 1, INT32_MIN), refpos(nblk + 1, INT32_MIN), readpos(nblk + 1, INT32_MIN), matchref(nblk + 1, INT32_MIN), matchread(nblk + 1, INT32_MIN), rn(nblk + 1, -7), t[4];
    std::vector<uint8_t> rev(nblk + 1, 0xff);
    for (auto& v : t) v.assign(nblk + 1, 0);
    const bwe::FragsW W{off.data(), na.data(), atot.data(), btot.data(), low.data(), refid.data(), rev.data(), refpos.data(), readpos.data(), matchref.data(), matchread.data()};
    for (int64_t q = nf; q-- > 0;) bwe::fill_record(R, meta.data(), W, q);
    chs::Frags F;
    F.nf = nf; F.nblk = (int64_t)nblk; F.off = off.data(); F.na = na.data(); F.atot = atot.data(); F.btot = btot.data(); F.low = low.data(); F.refid = refid.data(); F.rev = rev.data();
    F.refpos = refpos.data(); F.readpos = readpos.data(); F.matchref = matchref.data(); F.matchread = matchread.data();
    const chs::Trim T{t[0].data(), t[1].data(), t[2].data(), t[3].data()};
    // the position chain (chim_chain): the soft list holds every fragment
    std::vector<int32_t> pin((size_t)nf + 1, 0), lastdeep((size_t)nf + 1, 0), spos((size_t)nf + 1, 0), sout((size_t)nf + 1, 0);
    std::vector<uint32_t> soft((size_t)nf + 1, 0);
    const chs::Chain C{pin.data(), lastdeep.data(), spos.data(), soft.data(), sout.data(), cls.data(), (uint32_t)nf};
    for (int64_t q = nf; q-- > 0;) chs::classify(N, F, F.refpos, F.matchref, 1, C, q);
    int last = INT32_MIN, ns = 0;
    for (int64_t q = 0; q < nf; ++q) { lastdeep[(size_t)q] = last; spos[(size_t)q] = ns; if (pin[(size_t)q] >= 0) last = (int)q; if (cls[(size_t)q] == chs::CLS_SOFT) ++ns; }
    r.n_soft = ns;
    for (int64_t q = nf; q-- > 0;) chs::soft_list(F, C, q);
    for (uint32_t k = (uint32_t)ns; k-- > 0;) chs::soft_resolve(N, F, F.refpos, F.readpos, F.matchref, F.matchread, C, (uint32_t)ns, k);
    for (uint32_t k = 0, run = 0; k < (uint32_t)ns; ++k) {
        run = chs::soft_follows(C, k) ? run + 1 : 1;
        if (run == 2) ++r.soft_runs;
        r.longest_run = std::max<long>(r.longest_run, run);
    }
    // the edge kernel; the table starts small and grows, as on the device
    std::vector<unsigned long long> hk;
    std::vector<uint32_t> hv;
    for (uint32_t slots = 64;; slots <<= 2) {
        hk.assign(slots, ~0ull); hv.assign(slots, 0);
        flags[0] = 0;
        int32_t fin = 0;
        for (int64_t q = nf; q-- > 0;) bwe::edge_fragment(N, F, T, rn.data(), C, P, meta.data(), hk.data(), hv.data(), slots - 1, flags, bits.data(), &fin, q);
        r.final_pos = fin;
        if (!(flags[0] & chs::FLAG_FULL)) break;
    }
    if (flags[0] & chs::FLAG_ASSERT) { r.assert_ = true; return r; }
    std::vector<std::pair<unsigned long long, int32_t>> kw;
    for (size_t s = 0; s < hk.size(); ++s) if (hk[s] != ~0ull) { kw.push_back(std::make_pair(hk[s], (int32_t)hv[s])); r.n_emitted += hv[s]; }
    std::sort(kw.begin(), kw.end());
    for (const auto& x : kw) { r.keys.push_back(x.first); r.weights.push_back(x.second); }
    // the lists: three exclusive scans, one scatter
    std::vector<int32_t> at[3];
    size_t tot[3] = {0, 0, 0};
    const uint8_t which[3] = {bwe::B_PART, bwe::B_FIRST_DIS, bwe::B_SECOND};
    for (int l = 0; l < 3; ++l) { at[l].assign((size_t)nf, 0); for (int64_t q = 0; q < nf; ++q) { at[l][(size_t)q] = (int32_t)tot[l]; if (bits[(size_t)q] & which[l]) ++tot[l]; } }
    r.part.assign(tot[0] + 1, ~0u); r.first_dis.assign(tot[1] + 1, ~0u); r.second.assign(tot[2] + 1, ~0u); r.second_keys.assign(tot[2] + 1, ~0ull);
    for (int64_t q = nf; q-- > 0;) bwe::scatter_lists(F, rn.data(), bits.data(), at[0].data(), at[1].data(), at[2].data(), r.part.data(), r.first_dis.data(), r.second.data(), r.second_keys.data(), q);
    r.part.resize(tot[0]); r.first_dis.resize(tot[1]); r.second.resize(tot[2]); r.second_keys.resize(tot[2]);
    for (int64_t q = 0; q < nf; ++q) { r.kind1 += (meta[(size_t)q] & bwe::M_KIND) == 1; r.kind2 += (meta[(size_t)q] & bwe::M_KIND) == 2; }
    return r;
}

// both routes on one batch and one node table.  host_rc: what the host loop returned (SQ_E_ASSERT: the emulated route must raise its flag)
long compare(sq_ctx& c, const HostBatch& hb, const std::vector<Node>& nodes, Emulated& e, BwaEdgesDebug& h, int& host_rc, bool say) {
    long bad = 0;
    host_rc = SQ_OK;
    if (!nodes.empty() || hb.size() == 0) host_rc = hb.size() ? bwa_raw_edges_debug(&c, &hb, nodes, 0, h) : SQ_OK;
    e = emulate(hb, nodes, chs::Params{c.P.concord_dist_pos, c.P.concord_dist_idx});
    if (e.tie) { if (say) std::printf("   the emulated route found equal read offsets inside a record\n"); return 1; }
    if (host_rc == SQ_E_ASSERT || e.assert_) {
        if ((host_rc == SQ_E_ASSERT) != e.assert_) { ++bad; if (say) std::printf("   assert: host loop %d, emulated flag %d\n", host_rc, (int)e.assert_); }
        return bad;
    }
    if (host_rc) { if (say) std::printf("   host loop: %s\n", c.err.c_str()); return 1; }
    auto diff = [&](const char* what, bool d) { if (d) { ++bad; if (say) std::printf("   %s differ\n", what); } };
    diff("edge keys", e.keys != h.keys);
    diff("edge weights", e.weights != h.weights);
    diff("partial lists", e.part != h.part);
    diff("first_dis lists", e.first_dis != h.first_dis);
    diff("second lists", e.second != h.second);
    diff("second keys", e.second_keys != h.second_keys);
    diff("final positions", e.final_pos != h.final_pos);
    diff("emitted edges", e.n_emitted != h.n_emitted);
    if (bad && say) {
        std::printf("   host: %zu keys, %zu / %zu / %zu listed, final %d, emitted %lld; emulated: %zu keys, %zu / %zu / %zu listed, final %d, emitted %ld\n", h.keys.size(), h.part.size(), h.first_dis.size(),
                    h.second.size(), h.final_pos, (long long)h.n_emitted, e.keys.size(), e.part.size(), e.first_dis.size(), e.second.size(), e.final_pos, e.n_emitted);
        for (size_t i = 0, shown = 0; i < std::max(e.keys.size(), h.keys.size()) && shown < 6; ++i) {
            const unsigned long long a = i < h.keys.size() ? h.keys[i] : 0, b = i < e.keys.size() ? e.keys[i] : 0;
            const int wa = i < h.keys.size() ? h.weights[i] : 0, wb = i < e.keys.size() ? e.weights[i] : 0;
            if (a != b || wa != wb) { std::printf("   edge %zu: host (%d, %d, %d%d) x %d, emulated (%d, %d, %d%d) x %d\n", i, (int)(a >> 32), (int)((a & 0xffffffffull) >> 2), (int)((a >> 1) & 1), (int)(a & 1), wa, (int)(b >> 32), (int)((b & 0xffffffffull) >> 2), (int)((b >> 1) & 1), (int)(b & 1), wb); ++shown; }
        }
    }
    return bad;
}

// ---- fuzz
struct Case { std::vector<Node> nodes; HostBatch hb; int n_ref = 0; bool tiny = false; long edge_near = 0, big = 0, other_chr = 0, mate_unmapped = 0, mate_none = 0, planted = 0; };
// table sizes: one below, exactly at and one above one and two blocks of 256 lanes and one and two tiles of the scans (256 x 16 elements)
const int SIZES[] = {0, 1, 7, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 100, 1000, 2500};
// style 0: random tiling (15-260 bases, now and then 1-4); 1: nodes of 1-4 bases (most first blocks are soft, soft runs are long); 2: 2-9 bases
// plant: 0 none, 1 a block behind the last node, 2 a block that hangs over the end of the last node (its home edge would leave the table),
// 3 a block in front of the first node
Case make_case(std::mt19937_64& rng, int index) {
    Case cs;
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int want = SIZES[index % (int)(sizeof SIZES / sizeof *SIZES)];
    const int style = (index / 3) % 3;
    const int plant = index % 5 == 3 && want >= 7 ? 1 + (index / 5) % 3 : 0;
    cs.tiny = style == 1;
    cs.hb.blk_off.assign(1, 0); cs.hb.name_off.assign(1, 0);
    if (want == 0 && index % 2 == 0) return cs;  // zero fragments and zero nodes
    const int nchr = rnd(1, 4);
    cs.n_ref = nchr;
    std::vector<std::pair<int, int>> range((size_t)nchr);  // node index range per chromosome
    std::vector<int> L((size_t)nchr);
    for (int ch = 0; ch < nchr; ++ch) {
        const int len = style == 1 ? rnd(200, 500) : style == 2 ? rnd(600, 1500) : rnd(3000, 9000);
        int p = 0;
        range[(size_t)ch].first = (int)cs.nodes.size();
        while (p < len) {
            const int l = style == 1 ? rnd(1, 4) : style == 2 ? rnd(2, 9) : (rnd(0, 9) == 0 ? rnd(1, 4) : rnd(15, 260));
            cs.nodes.push_back(Node{ch, p, l, 0, 0.0});
            p += l;
        }
        range[(size_t)ch].second = (int)cs.nodes.size();
        L[(size_t)ch] = p;
    }
    struct Rec { int refid, pos, mrefid, mpos, flag, totlen, mapq, aux; std::vector<int> b; /* refpos, matchref, readpos, matchread */ };
    std::vector<Rec> recs;
    for (int k = 0; k < want; ++k) {
        Rec r;
        const int ch = rnd(0, nchr - 1);
        const bool first = rnd(0, 99) < 70, rev = rnd(0, 1) != 0;
        const int pick = rnd(0, 99);
        int nb = pick < 55 ? 1 : pick < 85 ? 2 : pick < 93 ? 3 : pick < 98 ? 17 : 256;
        if (nb > 2) ++cs.big;
        // the first block (in reference order): around a node edge, inside a node, or anywhere
        const int ni = rnd(range[(size_t)ch].first, range[(size_t)ch].second - 1);
        const Node& nd = cs.nodes[(size_t)ni];
        const int where = rnd(0, 99);
        int p, len = nb >= 17 ? rnd(1, 3) : rnd(1, 60);
        if (where < 25) { p = nd.pos + rnd(-5, 5); ++cs.edge_near; }
        else if (where < 50) { p = nd.pos + nd.len + rnd(-5, 5) - len; ++cs.edge_near; }
        else if (where < 80) { len = std::min(len, nd.len); p = nd.pos + rnd(0, nd.len - len); }
        else p = rnd(0, std::max(0, L[(size_t)ch] - 1));
        if (p < 0) p = 0;
        // the blocks in reference order; read offsets run with them on the forward strand and against them on the reverse strand
        std::vector<std::pair<int, int>> ref;  // refpos, matchref
        int at = p;
        for (int q = 0; q < nb; ++q) {
            const int l = q == 0 ? len : (nb >= 17 ? rnd(1, 3) : rnd(5, 60));
            if (q) at += nb >= 17 ? rnd(1, 12) : rnd(1, std::max(2, L[(size_t)ch] / 10));
            if (at + l > L[(size_t)ch]) { if (q == 0) { at = std::max(0, L[(size_t)ch] - l); } else break; }
            ref.push_back(std::make_pair(at, std::min(l, L[(size_t)ch] - at)));
            at += l;
        }
        const int lead = std::min(rnd(0, 99) < 60 ? rnd(0, 3) : rnd(13, 19), 19);  // read offset of the block that comes first in the read: around 15 / 16
        const int trail = rnd(0, 99) < 70 ? rnd(0, 10) : rnd(14, 30);
        int rp = lead;
        std::vector<int> rps(ref.size());
        for (size_t q = 0; q < ref.size(); ++q) { const size_t j = rev ? ref.size() - 1 - q : q; rps[j] = rp; rp += ref[j].second + (rnd(0, 9) == 0 ? rnd(1, 5) : 0); }
        r.totlen = std::min(rp + trail, 65000);
        for (size_t q = 0; q < ref.size(); ++q) { r.b.push_back(ref[q].first); r.b.push_back(ref[q].second); r.b.push_back(rps[q]); r.b.push_back(ref[q].second); }
        r.refid = ch; r.pos = ref[0].first;
        r.flag = 0x1 | (first ? 0x40 : 0x80) | (rev ? 0x10 : 0) | (rnd(0, 1) ? 0x20 : 0);
        const int mate = rnd(0, 99);
        // (a mate stub is 15 bases long: kept inside its chromosome, so that only the planted blocks make the loop assert)
        if (mate < 55) { r.mrefid = ch; r.mpos = rnd(0, L[(size_t)ch] - 21); }
        else if (mate < 75) { r.mrefid = rnd(0, nchr - 1); r.mpos = rnd(0, L[(size_t)r.mrefid] - 21); cs.other_chr += r.mrefid != ch; }
        else if (mate < 90) { r.mrefid = ch; r.mpos = r.pos; r.flag |= 0x8; ++cs.mate_unmapped; }
        else { r.mrefid = -1; r.mpos = -1; ++cs.mate_none; }
        if (rnd(0, 99) < 3) r.flag |= 0x400;
        if (rnd(0, 99) < 3) r.flag |= 0x4;
        if (rnd(0, 99) < 30) r.flag |= 0x2;
        r.aux = (first ? rnd(0, 99) < 8 : rnd(0, 99) < 75) ? SQ_AUX_MULTI : 0;
        if (rnd(0, 99) < 10) r.aux |= SQ_AUX_LOWPHRED;
        r.mapq = rnd(0, 99) < 8 ? 0 : rnd(1, 60);
        recs.push_back(r);
    }
    std::stable_sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.refid != y.refid ? x.refid < y.refid : x.pos < y.pos; });
    if (plant && !recs.empty()) {
        // a first mate that passes every filter, with one block that no node takes and whose home edge has no place in the table
        Rec r;
        const Node& lastn = cs.nodes.back();
        const int end = lastn.pos + lastn.len;
        r.refid = plant == 3 ? 0 : lastn.chr;
        const int p = plant == 1 ? end + rnd(6, 40) : plant == 2 ? end - 1 : -20, l = plant == 2 ? 30 : 10;
        r.pos = p; r.mrefid = -1; r.mpos = -1; r.flag = 0x1 | 0x40; r.totlen = l; r.mapq = 60; r.aux = 0;
        r.b = {p, l, 0, l};
        recs[plant == 3 ? 0 : recs.size() - 1 - (size_t)rnd(0, (int)std::min<size_t>(recs.size() - 1, 3))] = r;  // (the table keeps its size)
        ++cs.planted;
    }
    HostBatch& hb = cs.hb;
    for (const Rec& r : recs) {
        hb.refid.push_back(r.refid); hb.pos.push_back(r.pos); hb.mrefid.push_back(r.mrefid); hb.mpos.push_back(r.mpos); hb.endpos.push_back(r.pos);
        hb.flag.push_back((uint16_t)r.flag); hb.totlen.push_back((uint16_t)r.totlen); hb.mapq.push_back((uint8_t)r.mapq); hb.aux.push_back((uint8_t)r.aux);
        for (size_t q = 0; q < r.b.size(); q += 4) { hb.b_refpos.push_back(r.b[q]); hb.b_matchref.push_back(r.b[q + 1]); hb.b_readpos.push_back((uint16_t)r.b[q + 2]); hb.b_matchread.push_back((uint16_t)r.b[q + 3]); }
        hb.blk_off.push_back((uint32_t)hb.b_refpos.size());
        hb.name_off.push_back(0);
    }
    return cs;
}
void write_case(std::FILE* f, const Case& cs, bool asserts, long soft) {
    const HostBatch& hb = cs.hb;
    std::fprintf(f, "case %zu %zu %zu %d %ld\n", cs.nodes.size(), hb.size(), hb.b_refpos.size(), (int)asserts, soft);
    for (const Node& n : cs.nodes) std::fprintf(f, "%d %d %d\n", n.chr, n.pos, n.len);
    for (size_t r = 0; r < hb.size(); ++r)
        std::fprintf(f, "%d %d %d %d %d %d %d %d %u\n", hb.refid[r], hb.pos[r], hb.mrefid[r], hb.mpos[r], (int)hb.flag[r], (int)hb.totlen[r], (int)hb.mapq[r], (int)hb.aux[r], hb.blk_off[r + 1] - hb.blk_off[r]);
    for (size_t b = 0; b < hb.b_refpos.size(); ++b) std::fprintf(f, "%d %d %d %d\n", hb.b_refpos[b], hb.b_matchref[b], (int)hb.b_readpos[b], (int)hb.b_matchread[b]);
}
std::string qname_of(const HostBatch& hb, size_t r) {
    std::string q(hb.names.data() + hb.name_off[r], hb.names.data() + hb.name_off[r + 1]);
    if (q.size() >= 2 && (q.compare(q.size() - 2, 2, "/1") == 0 || q.compare(q.size() - 2, 2, "/2") == 0)) q.resize(q.size() - 2);
    return q;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: bwa_edges_emu <bwa.bam> [min_mapqual] | --fuzz <cases> <seed> [--write <file>]\n"); return 2; }
    sq_ctx c;
    sq_default_params(&c.P);
    c.pool.reset(new HostPool(3));
    if (!std::strcmp(argv[1], "--fuzz")) {
        if (argc < 4) return 2;
        const int cases = std::atoi(argv[2]);
        std::mt19937_64 rng((uint64_t)std::strtoull(argv[3], nullptr, 10));
        std::FILE* out = argc > 5 && !std::strcmp(argv[4], "--write") ? std::fopen(argv[5], "w") : nullptr;
        long bad = 0, records = 0, blocks = 0, soft = 0, runs = 0, longest = 0, kind1 = 0, kind2 = 0, part = 0, first_dis = 0, second = 0, asserts = 0, planted = 0, tiny = 0, near = 0, big = 0, other_chr = 0,
             mate_unmapped = 0, mate_none = 0, empty = 0, edges = 0;
        for (int k = 0; k < cases; ++k) {
            Case cs = make_case(rng, k);
            Emulated e;
            BwaEdgesDebug h;
            int host_rc = 0;
            const long b = compare(c, cs.hb, cs.nodes, e, h, host_rc, true);
            if (b) std::printf("case %d: %ld differences\n", k, b);
            bad += b;
            if (out) write_case(out, cs, e.assert_, e.n_soft);
            empty += cs.hb.size() == 0;
            planted += cs.planted;
            if (cs.planted && !e.assert_) { ++bad; std::printf("case %d: the planted block did not raise the assert flag\n", k); }
            if (e.assert_) { ++asserts; continue; }
            records += (long)cs.hb.size(); blocks += e.blocks; soft += e.n_soft; runs += e.soft_runs; longest = std::max(longest, e.longest_run); kind1 += e.kind1; kind2 += e.kind2;
            part += (long)e.part.size(); first_dis += (long)e.first_dis.size(); second += (long)e.second.size(); edges += e.n_emitted;
            tiny += cs.tiny; near += cs.edge_near; big += cs.big; other_chr += cs.other_chr; mate_unmapped += cs.mate_unmapped; mate_none += cs.mate_none;
        }
        if (out) std::fclose(out);
        std::printf("%d cases, %ld records, %ld block slots, kind-1 %ld, kind-2 %ld, soft fragments %ld, soft runs longer than one %ld (longest %ld), partial %ld, first_dis %ld, second %ld, emitted edges %ld, "
                    "assert cases %ld (planted %ld), empty tables %ld, tables on nodes of 1-4 bases %ld, first blocks at a node edge %ld, records of 3 and more blocks %ld, mates on another chromosome %ld, "
                    "unmapped mates %ld, mates without a reference %ld, %ld differences\n",
                    cases, records, blocks, kind1, kind2, soft, runs, longest, part, first_dis, second, edges, asserts, planted, empty, tiny, near, big, other_chr, mate_unmapped, mate_none, bad);
        std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
        return bad ? 1 : 0;
    }
    c.P.min_mapqual = argc > 2 ? std::atoi(argv[2]) : 1;
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
    if (bwa_nodes_and_edges(&c, raw)) { std::printf("host stages: %s\n", c.err.c_str()); return 1; }  // (the nodes of BuildNode_BWA)
    Emulated e;
    BwaEdgesDebug h;
    int host_rc = 0;
    long bad = compare(c, hb, c.nodes, e, h, host_rc, true);
    if (host_rc == SQ_E_ASSERT || e.assert_) { std::printf("   the loop asserts on this file\n"); ++bad; }
    // the -1 edges that are really added: the listed second mates whose name is among the first mates that added a discordant pair edge
    std::set<std::string> fd;
    for (const uint32_t r : e.first_dis) fd.insert(qname_of(hb, r));
    long added = 0, big = 0;
    for (const uint32_t r : e.second) added += fd.count(qname_of(hb, r)) != 0;
    for (size_t r = 0; r < hb.size(); ++r) big += hb.blk_off[r + 1] - hb.blk_off[r] >= 3;
    std::printf("%zu records, %zu nodes, kind-1 %ld, kind-2 %ld, soft fragments %ld, soft runs longer than one %ld (longest %ld), partial %zu, first_dis %zu, second %zu, -1 edges added %ld, "
                "records of 3 and more blocks %ld, emitted edges %ld, final position %d, %ld differences\n",
                hb.size(), c.nodes.size(), e.kind1, e.kind2, e.n_soft, e.soft_runs, e.longest_run, e.part.size(), e.first_dis.size(), e.second.size(), added, big, e.n_emitted, e.final_pos, bad);
    std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
    return bad ? 1 : 0;
}
