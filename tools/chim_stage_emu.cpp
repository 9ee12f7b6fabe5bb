// The chimeric graph stages of the device route (squid_amd/csrc/sq_chim_stage.inc: RawEdgesChim, ExactBreakpoint + CountTop) on the CPU: the
// kernel source itself -- lane-local bodies called once per lane index, the wave-level CountTop as 64 coroutines (sq_wave.h with
// SQ_WAVE_EMU) -- against the host functions of the library (chimeric_edges, exact_breakpoints; linked against libsquid_hip.so, no device
// needed).  Compared: the reduced raw-edge list, the trimmed blocks of every fragment behind each stage, the per-edge breakpoint lists in
// order.  The lane indices are visited from the last to the first, so a result that depended on another lane's work would show.
//   chim_stage_emu <chimeric.bam> <oracle dump dir> [threads]      fragments by the library's host code, node / edge tables of the oracle
//   chim_stage_emu --fuzz <cases> <seed> [--write <file>]          random tables (see make_case); --write keeps the cases as numbers for
//                                                                  the device test (sq_debug_chim_stages)
#include "../squid_amd/csrc/sq_internal.h"
#include "../squid_amd/csrc/sq_chim_stage.inc"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
using namespace sq;

namespace {
struct Flat {  // the device's fragment table, on the host
    std::vector<uint32_t> off, na;
    std::vector<int32_t> atot, btot, refid, refpos, readpos, matchref, matchread;
    std::vector<uint8_t> low, rev;
    std::vector<int32_t> t[4];  // the trimmed blocks
    chs::Frags F;
    chs::Trim T;
    void make(const std::vector<Frag>& src) {
        const size_t nf = src.size();
        off.assign(nf + 1, 0); na.resize(nf); atot.resize(nf); btot.resize(nf); low.resize(nf);
        for (size_t q = 0; q < nf; ++q) {
            const Frag& f = src[q];
            off[q + 1] = off[q] + (uint32_t)(f.a.size() + f.b.size()); na[q] = (uint32_t)f.a.size(); atot[q] = f.atot; btot[q] = f.btot; low[q] = (uint8_t)((f.alow ? 1 : 0) | (f.blow ? 2 : 0));
            for (int mate = 0; mate < 2; ++mate)
                for (const Blk& b : (mate ? f.b : f.a)) { refid.push_back(b.refid); refpos.push_back(b.refpos); readpos.push_back(b.readpos); matchref.push_back(b.matchref); matchread.push_back(b.matchread); rev.push_back(b.rev ? 1 : 0); }
        }
        const size_t nb = refid.size();
        for (auto& v : t) v.assign(nb + 1, 0);
        refid.push_back(0); refpos.push_back(0); readpos.push_back(0); matchref.push_back(0); matchread.push_back(0); rev.push_back(0);  // (never empty)
        F.nf = (int64_t)nf; F.nblk = (int64_t)nb; F.off = off.data(); F.na = na.data(); F.atot = atot.data(); F.btot = btot.data(); F.low = low.data(); F.refid = refid.data(); F.rev = rev.data();
        F.refpos = refpos.data(); F.readpos = readpos.data(); F.matchref = matchref.data(); F.matchread = matchread.data();
        T.refpos = t[0].data(); T.readpos = t[1].data(); T.matchref = t[2].data(); T.matchread = t[3].data();
    }
};
struct NodeTab {
    std::vector<int32_t> chr, pos, len;
    chs::Nodes N;
    void make(const std::vector<Node>& v) {
        for (const Node& n : v) { chr.push_back(n.chr); pos.push_back(n.pos); len.push_back(n.len); }
        N.n = (int32_t)v.size(); N.chr = chr.data(); N.pos = pos.data(); N.len = len.data();
    }
};
struct ChainMem {
    std::vector<int32_t> pin, lastdeep, spos, sout;
    std::vector<uint32_t> soft;
    std::vector<uint8_t> cls;
    chs::Chain C;
    uint32_t nsoft = 0;
};
// the position chain of a stage: the kernels' bodies, and the two scans of dev_* as plain loops
void chain(const chs::Nodes& N, const Flat& fl, int stage, ChainMem& m) {
    const int64_t nf = fl.F.nf;
    m.pin.assign(nf + 1, 0); m.lastdeep.assign(nf + 1, 0); m.spos.assign(nf + 1, 0); m.cls.assign(nf + 1, 0); m.soft.assign(nf + 1, 0); m.sout.assign(nf + 1, 0);
    m.C.pin = m.pin.data(); m.C.lastdeep = m.lastdeep.data(); m.C.spos = m.spos.data(); m.C.soft = m.soft.data(); m.C.sout = m.sout.data(); m.C.cls = m.cls.data(); m.C.soft_cap = (uint32_t)nf;
    const int32_t *refpos = stage == 1 ? fl.F.refpos : fl.T.refpos, *readpos = stage == 1 ? fl.F.readpos : fl.T.readpos, *matchref = stage == 1 ? fl.F.matchref : fl.T.matchref,
                  *matchread = stage == 1 ? fl.F.matchread : fl.T.matchread;
    for (int64_t q = nf; q-- > 0;) chs::classify(N, fl.F, refpos, matchref, stage, m.C, q);
    int last = INT32_MIN, ns = 0;
    for (int64_t q = 0; q < nf; ++q) { m.lastdeep[q] = last; m.spos[q] = ns; if (m.pin[q] >= 0) last = (int)q; if (m.cls[q] == chs::CLS_SOFT) ++ns; }
    m.nsoft = (uint32_t)ns;
    for (int64_t q = nf; q-- > 0;) chs::soft_list(fl.F, m.C, q);
    for (uint32_t k = m.nsoft; k-- > 0;) chs::soft_resolve(N, fl.F, refpos, readpos, matchref, matchread, m.C, m.nsoft, k);
}
struct TopArg { int32_t e; const int32_t *goff, *p1, *p2; int32_t* score; bool ha, hb; int32_t *out_n, *out_xy; };
void top_lane(void* p) { const TopArg& a = *(const TopArg*)p; chs::count_top_wave(a.e, a.goff, a.p1, a.p2, a.score, a.ha, a.hb, a.out_n, a.out_xy); }

struct Result {
    int rc = 0;
    std::vector<Edge> red;
    std::vector<Frag> f1, f2;  // the fragments behind stage 1 / stage 2
    BPMap bp;
    long soft1 = 0, soft2 = 0;
    int biggest = 0;
};
void unflatten(const Flat& fl, std::vector<Frag>& f) {
    size_t k = 0;
    for (Frag& x : f) for (int mate = 0; mate < 2; ++mate) for (Blk& b : (mate ? x.b : x.a)) { b.refpos = fl.t[0][k]; b.readpos = fl.t[1][k]; b.matchref = fl.t[2][k]; b.matchread = fl.t[3][k]; ++k; }
}
Result run_emulated(const std::vector<Frag>& frags, const std::vector<Node>& N1, const std::vector<Node>& N2, const std::vector<Edge>& E, const chs::Params& P) {
    Result r;
    Flat fl;
    fl.make(frags);
    NodeTab n1, n2;
    n1.make(N1); n2.make(N2);
    const int64_t nf = fl.F.nf, nblk = fl.F.nblk;
    std::vector<int32_t> rn((size_t)nblk + 1, 0);
    ChainMem m;
    chain(n1.N, fl, 1, m);
    r.soft1 = m.nsoft;
    uint32_t slots = 64;
    while (slots < 8 * (uint32_t)(nblk + 1)) slots <<= 1;
    std::vector<unsigned long long> hk(slots, ~0ull);
    std::vector<uint32_t> hv(slots, 0);
    uint32_t flags = 0;
    for (int64_t q = nf; q-- > 0;) chs::stage1_fragment(n1.N, fl.F, fl.T, rn.data(), m.C, P, hk.data(), hv.data(), slots - 1, &flags, q);
    if (flags & chs::FLAG_FULL) { std::printf("emulated hash table full\n"); r.rc = SQ_E_CAPACITY; return r; }
    if (flags & chs::FLAG_ASSERT) { r.rc = SQ_E_ASSERT; return r; }
    std::vector<Edge> raw;
    for (uint32_t s = 0; s < slots; ++s)
        if (hk[s] != ~0ull) { Edge e; e.a = (int32_t)(hk[s] >> 32); e.b = (int32_t)((hk[s] & 0xffffffffull) >> 2); e.ha = (hk[s] >> 1) & 1; e.hb = hk[s] & 1; e.w = (int32_t)hv[s]; e.gw = 0; raw.push_back(e); }
    reduce_edges(raw, r.red);
    r.f1 = frags; unflatten(fl, r.f1);
    // stage 2
    const int32_t me = (int32_t)E.size();
    std::vector<unsigned long long> ekey;
    for (const Edge& e : E) ekey.push_back(edge_pack(e));
    ekey.push_back(0);
    chain(n2.N, fl, 2, m);
    r.soft2 = m.nsoft;
    std::vector<int32_t> hit_e((size_t)nblk + 1, -1), hit_b1((size_t)nblk + 1, 0), hit_b2((size_t)nblk + 1, 0), goff((size_t)me + 1, 0), p1((size_t)nblk + 1, 0), p2((size_t)nblk + 1, 0),
        score((size_t)nblk + 1, 0), out_n((size_t)me + 1, 0), out_xy(10 * (size_t)me + 10, 0);
    std::vector<uint32_t> hist((size_t)me + 1, 0), cursor((size_t)me + 1, 0);
    for (int64_t q = nf; q-- > 0;) chs::stage2_fragment(n2.N, fl.F, fl.T, rn.data(), m.C, P, ekey.data(), me, hit_e.data(), hit_b1.data(), hit_b2.data(), hist.data(), q);
    for (int32_t e = 0; e < me; ++e) { goff[(size_t)e + 1] = goff[(size_t)e] + (int32_t)hist[(size_t)e]; r.biggest = std::max(r.biggest, (int)hist[(size_t)e]); }
    for (int64_t k = nblk; k-- > 0;) chs::scatter_hit(nblk, hit_e.data(), hit_b1.data(), hit_b2.data(), goff.data(), cursor.data(), p1.data(), p2.data(), k);
    for (int32_t e = 0; e < me; ++e) {
        TopArg a{e, goff.data(), p1.data(), p2.data(), score.data(), E[(size_t)e].ha != 0, E[(size_t)e].hb != 0, out_n.data(), out_xy.data()};
        wv::run_wave(top_lane, &a);
        if (out_n[(size_t)e] > 0) {
            std::vector<std::pair<int, int>> x;
            for (int k = 0; k < out_n[(size_t)e]; ++k) x.push_back(std::make_pair(out_xy[10 * (size_t)e + 2 * (size_t)k], out_xy[10 * (size_t)e + 2 * (size_t)k + 1]));
            r.bp[ekey[(size_t)e]] = x;
        }
    }
    r.f2 = frags; unflatten(fl, r.f2);
    return r;
}
Result run_host(sq_ctx& c, const std::vector<Frag>& frags, const std::vector<Node>& N1, const std::vector<Node>& N2) {
    Result r;
    c.frags = frags; c.nodes = N1; c.err.clear();
    r.soft1 = chim_stage_soft_count(&c, N1, 1);
    std::vector<Edge> raw;
    r.rc = chimeric_edges(&c, raw);
    if (r.rc) return r;
    reduce_edges(raw, r.red);
    r.f1 = c.frags;
    c.nodes = N2;
    r.soft2 = chim_stage_soft_count(&c, N2, 2);
    r.rc = exact_breakpoints(&c, r.bp);
    r.f2 = c.frags;
    return r;
}
long blocks_differ(const std::vector<Frag>& x, const std::vector<Frag>& y) {
    long bad = 0;
    for (size_t q = 0; q < x.size(); ++q)
        for (int mate = 0; mate < 2; ++mate) {
            const BlkList &p = mate ? x[q].b : x[q].a, &r = mate ? y[q].b : y[q].a;
            for (size_t k = 0; k < p.size(); ++k) if (p[k].refpos != r[k].refpos || p[k].readpos != r[k].readpos || p[k].matchref != r[k].matchref || p[k].matchread != r[k].matchread) ++bad;
        }
    return bad;
}
// differences between the two routes; the breakpoint lists are compared for the keys of E (call_sv looks up nothing else)
long compare(const Result& h, const Result& d, const std::vector<Edge>& E, bool say) {
    long bad = 0;
    if (h.rc != d.rc) { if (say) std::printf("   return codes differ: host %d, emulated %d\n", h.rc, d.rc); return 1; }
    if (h.rc) return 0;
    if (h.red.size() != d.red.size()) { ++bad; if (say) std::printf("   raw edges: %zu vs %zu\n", h.red.size(), d.red.size()); }
    for (size_t i = 0; i < std::min(h.red.size(), d.red.size()); ++i)
        if (!edge_key_eq(h.red[i], d.red[i]) || h.red[i].w != d.red[i].w) { if (say && bad < 10) std::printf("   raw edge %zu: (%d %d %d %d w%d) vs (%d %d %d %d w%d)\n", i, h.red[i].a, h.red[i].b, h.red[i].ha, h.red[i].hb, h.red[i].w, d.red[i].a, d.red[i].b, d.red[i].ha, d.red[i].hb, d.red[i].w); ++bad; }
    const long b1 = blocks_differ(h.f1, d.f1), b2 = blocks_differ(h.f2, d.f2);
    if (say && (b1 || b2)) std::printf("   trimmed blocks differ: %ld behind stage 1, %ld behind stage 2\n", b1, b2);
    bad += b1 + b2;
    for (const Edge& e : E) {
        const BPMap::const_iterator a = h.bp.find(edge_pack(e)), b = d.bp.find(edge_pack(e));
        const bool ha = a != h.bp.end(), hb = b != d.bp.end();
        if (ha != hb || (ha && a->second != b->second)) { if (say && bad < 10) std::printf("   breakpoint list of edge (%d %d %d %d) differs\n", e.a, e.b, e.ha, e.hb); ++bad; }
    }
    if (h.soft1 != d.soft1 || h.soft2 != d.soft2) { ++bad; if (say) std::printf("   soft fragments: host %ld + %ld, emulated %ld + %ld\n", h.soft1, h.soft2, d.soft1, d.soft2); }
    return bad;
}

std::vector<std::vector<long long>> read_table(const std::string& path) {
    std::vector<std::vector<long long>> rows;
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::vector<long long> row;
        std::string f;
        while (std::getline(ss, f, '\t')) row.push_back(std::strtoll(f.c_str(), nullptr, 10));  // (the hex double of a node line reads as 0: not used)
        rows.push_back(row);
    }
    return rows;
}

// ---- fuzz: node tables that tile a few chromosomes without gaps (nodes shorter than 5 bases included), one for each stage;
// fragments whose blocks are placed deep inside, on, within 5 bases of,
// across and outside node boundaries, on the same and on other chromosomes than their neighbours'; clusters of split reads between two
// spots (hit groups, one of more than 64 pairs in case 0)
struct Case { std::vector<Node> N1, N2; std::vector<Frag> frags; std::vector<Edge> E; };
Case make_case(std::mt19937_64& rng, int index) {
    Case cs;
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int nchr = rnd(2, 4);  // (and one more behind them that only the blocks of an `outside` case use: a block that no node takes has a node behind it)
    std::vector<int> chrlen((size_t)nchr + 1);
    std::vector<std::vector<int>> bounds((size_t)nchr + 1), bounds2((size_t)nchr + 1);  // node starts of N1 / N2
    for (int ch = 0; ch <= nchr; ++ch) {
        int p = 0;
        const int L = rnd(1500, 5000);
        while (p < L) {
            const int len = rnd(0, 9) == 0 ? rnd(1, 4) : rnd(15, 260);
            cs.N1.push_back(Node{ch, p, len, 0, 0.0});
            bounds[(size_t)ch].push_back(p);
            p += len;
        }
        chrlen[(size_t)ch] = p;
        for (int q = 0; q < p;) {  // (a tiling of its own: a block deep inside a node of N1 may lie on a boundary of N2)
            const int len = std::min(p - q, rnd(0, 9) == 0 ? rnd(1, 4) : rnd(30, 500));
            cs.N2.push_back(Node{ch, q, len, 0, 0.0});
            bounds2[(size_t)ch].push_back(q);
            q += len;
        }
    }
    const bool with_outside = index % 7 == 3;  // a case in which the reference would assert
    auto block = [&](int chr, bool first, bool lead) {
        Blk b{};
        b.refid = chr; b.rev = rnd(0, 1) != 0; b.first = first; b.readpos = rnd(0, 90);
        const std::vector<int>& bd = rnd(0, 1) ? bounds[(size_t)chr] : bounds2[(size_t)chr];
        const int at = bd[(size_t)rnd(0, (int)bd.size() - 1)];
        if (lead && rnd(0, 9) != 0) {  // a fragment's first block, mostly: up to 5 bases over a boundary, the case LocateRead's start position decides
            b.matchref = rnd(12, 40);
            b.refpos = rnd(0, 1) ? std::max(0, at - rnd(1, 5)) : std::max(0, at + rnd(1, 5) - b.matchref);
            b.matchread = b.matchref;
            return b;
        }
        const int kind = rnd(0, 99);
        if (kind < 25) { b.refpos = rnd(0, std::max(0, chrlen[(size_t)chr] - 60)); b.matchref = rnd(8, 50); }            // anywhere
        else if (kind < 60) { b.refpos = std::max(0, at + rnd(-5, 5)); b.matchref = rnd(6, 40); }                              // starts at / near a boundary
        else if (kind < 85) { b.matchref = rnd(6, 40); b.refpos = std::max(0, at + rnd(-5, 5) - b.matchref); }                 // ends at / near a boundary
        else if (kind < 97) { b.refpos = std::max(0, at - rnd(1, 60)); b.matchref = rnd(20, 400); }                            // across boundaries
        else if (with_outside) { b.refid = nchr; b.refpos = chrlen[(size_t)nchr] + rnd(0, 300); b.matchref = rnd(10, 40); }    // behind the last node of the table
        else { b.refpos = std::max(0, chrlen[(size_t)chr] - rnd(1, 30)); b.matchref = rnd(10, 40); }                           // over the chromosome's end
        b.matchread = b.matchref;
        return b;
    };
    const int nfrag = rnd(60, 220);
    int chr = 0;
    for (int q = 0; q < nfrag; ++q) {
        Frag f;
        f.atot = 150; f.btot = 150;
        const int na = rnd(0, 11) == 0 ? 0 : rnd(1, 3) + (rnd(0, 3) ? 1 : 0), nb = rnd(0, 5) == 0 ? 0 : rnd(1, 3);
        for (int k = 0; k < na; ++k) { if (rnd(0, 9) < 4) chr = rnd(0, nchr - 1); f.a.push_back(block(chr, true, k == 0)); }
        for (int k = 0; k < nb; ++k) { if (rnd(0, 9) < 3) chr = rnd(0, nchr - 1); f.b.push_back(block(chr, false, na == 0 && k == 0)); }
        cs.frags.push_back(f);
    }
    const int clusters = index == 0 ? 3 : rnd(0, 3);
    for (int cl = 0; cl < clusters; ++cl) {
        const int c1 = rnd(0, nchr - 1), c2 = rnd(0, nchr - 1), x = rnd(100, chrlen[(size_t)c1] - 100), y = rnd(100, chrlen[(size_t)c2] - 100), count = (index == 0 && cl == 0) ? 150 : rnd(3, 40);
        const bool r1 = rnd(0, 1) != 0, r2 = rnd(0, 1) != 0;
        const int spread = rnd(0, 2) == 0 ? 60 : 4;
        for (int k = 0; k < count; ++k) {
            Frag f;
            f.atot = 150; f.btot = 150;
            Blk p{}, s{};
            p.refid = c1; p.rev = r1; p.first = true; p.matchref = p.matchread = rnd(20, 40); p.refpos = x + rnd(-spread, spread) - p.matchref; p.readpos = 0;
            s.refid = c2; s.rev = r2; s.first = true; s.matchref = s.matchread = rnd(20, 40); s.refpos = y + rnd(-spread, spread); s.readpos = p.matchread;
            f.a.push_back(p); f.a.push_back(s);
            if (rnd(0, 1)) f.b.push_back(block(c2, false, false));
            cs.frags.insert(cs.frags.begin() + rnd(0, (int)cs.frags.size()), f);
        }
    }
    return cs;
}
// the final edges of a case: most of the keys the host's ExactBreakpoint finds, and random others; sorted by key, unique
void make_edges(std::mt19937_64& rng, Case& cs, const BPMap& found) {
    std::vector<uint64_t> keys;
    for (const auto& kv : found) if (rng() % 10 < 8) keys.push_back(kv.first);
    const int n2 = (int)cs.N2.size();
    for (int k = 0; k < 20 && n2 > 1; ++k) { const int a = (int)(rng() % (uint64_t)(n2 - 1)), b = a + 1 + (int)(rng() % (uint64_t)(n2 - 1 - a)); keys.push_back(edge_pack(make_edge(a, rng() & 1, b, rng() & 1))); }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    cs.E.clear();
    for (uint64_t k : keys) { Edge e; e.a = (int32_t)(k >> 32); e.b = (int32_t)((k & 0xffffffffull) >> 2); e.ha = (k >> 1) & 1; e.hb = k & 1; e.w = 1; e.gw = 0; cs.E.push_back(e); }
}
void write_case(std::FILE* f, const Case& cs) {
    size_t nblk = 0;
    for (const Frag& x : cs.frags) nblk += x.a.size() + x.b.size();
    std::fprintf(f, "case %zu %zu %zu %zu %zu\n", cs.N1.size(), cs.N2.size(), cs.frags.size(), nblk, cs.E.size());
    for (const Node& n : cs.N1) std::fprintf(f, "%d %d %d\n", n.chr, n.pos, n.len);
    for (const Node& n : cs.N2) std::fprintf(f, "%d %d %d\n", n.chr, n.pos, n.len);
    for (const Frag& x : cs.frags) {
        std::fprintf(f, "%zu %zu %d %d\n", x.a.size(), x.b.size(), x.atot, x.btot);
        for (int mate = 0; mate < 2; ++mate) for (const Blk& b : (mate ? x.b : x.a)) std::fprintf(f, "%d %d %d %d %d %d\n", b.refid, b.refpos, b.readpos, b.matchref, b.matchread, b.rev ? 1 : 0);
    }
    for (const Edge& e : cs.E) std::fprintf(f, "%d %d %d %d\n", e.a, e.b, e.ha, e.hb);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: chim_stage_emu <chimeric.bam> <dump dir> [threads] | --fuzz <cases> <seed> [--write <file>]\n"); return 2; }
    sq_ctx c;
    sq_default_params(&c.P);
    const chs::Params P{c.P.concord_dist_pos, c.P.concord_dist_idx};
    if (!std::strcmp(argv[1], "--fuzz")) {
        if (argc < 4) return 2;
        c.pool.reset(new HostPool(3));
        const int cases = std::atoi(argv[2]);
        std::mt19937_64 rng((uint64_t)std::strtoull(argv[3], nullptr, 10));
        std::FILE* out = argc > 5 && !std::strcmp(argv[4], "--write") ? std::fopen(argv[5], "w") : nullptr;
        long frags = 0, soft1 = 0, soft2 = 0, bad = 0, asserts = 0;
        int biggest = 0;
        for (int k = 0; k < cases; ++k) {
            Case cs = make_case(rng, k);
            Result h = run_host(c, cs.frags, cs.N1, cs.N2);
            make_edges(rng, cs, h.bp);
            if (out) write_case(out, cs);
            const Result d = run_emulated(cs.frags, cs.N1, cs.N2, cs.E, P);
            const long b = compare(h, d, cs.E, true);
            if (b) std::printf("case %d: %ld differences\n", k, b);
            bad += b;
            if (h.rc == SQ_E_ASSERT) ++asserts;
            else { frags += (long)cs.frags.size(); soft1 += d.soft1; soft2 += d.soft2; biggest = std::max(biggest, d.biggest); }
        }
        if (out) std::fclose(out);
        std::printf("%d cases, %ld fragments, chim_soft_fragments stage 1: %ld (share %.3f), stage 2: %ld (share %.3f), %ld cases trip the reference's assert on both routes, largest hit group %d pairs\n",
                    cases, frags, soft1, frags ? (double)soft1 / frags : 0.0, soft2, frags ? (double)soft2 / frags : 0.0, asserts, biggest);
        std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
        return bad ? 1 : 0;
    }
    c.pool.reset(new HostPool(argc > 3 ? std::atoi(argv[3]) : 3));
    std::vector<std::string> names;
    std::string err;
    if (read_bam_header(argv[1], names, c.ref_len, err)) { std::printf("header: %s\n", err.c_str()); return 1; }
    if (chimeric_fragments_host(&c, argv[1], 2)) { std::printf("fragments: %s\n", c.err.c_str()); return 1; }
    const std::vector<Frag> frags = c.frags0.size() == c.frags.size() ? c.frags0 : c.frags;
    const std::string dump = argv[2];
    std::vector<Node> N1, N2;
    std::vector<Edge> E;
    for (const auto& r : read_table(dump + "/nodes_build.txt")) N1.push_back(Node{(int32_t)r[0], (int32_t)r[1], (int32_t)r[2], 0, 0.0});
    for (const auto& r : read_table(dump + "/nodes_final.txt")) N2.push_back(Node{(int32_t)r[0], (int32_t)r[1], (int32_t)r[2], 0, 0.0});
    for (const auto& r : read_table(dump + "/edges_final.txt")) E.push_back(make_edge((int)r[0], r[1] != 0, (int)r[2], r[3] != 0));  // ind1, head1, ind2, head2
    if (N1.empty() || N2.empty() || E.empty()) { std::printf("empty oracle tables in %s\n", dump.c_str()); return 1; }
    for (size_t i = 0; i + 1 < E.size(); ++i) if (!edge_key_less(E[i], E[i + 1])) { std::printf("final edges are not sorted by key\n"); return 1; }
    const Result h = run_host(c, frags, N1, N2);
    const Result d = run_emulated(frags, N1, N2, E, P);
    long in1 = 0, in2 = 0;
    for (const Frag& f : frags) { if (!(f.a.empty() && f.b.empty())) ++in1; if (!(f.a.size() <= 1 && f.b.size() <= 1)) ++in2; }
    std::printf("%zu fragments (stage 1: %ld, stage 2: %ld), %zu + %zu nodes, %zu final edges, %zu raw edges after the reduction, %zu edges with breakpoint lists, largest hit group %d pairs\n",
                frags.size(), in1, in2, N1.size(), N2.size(), E.size(), d.red.size(), d.bp.size(), d.biggest);
    std::printf("soft fragments by first_block_fit: stage 1 %ld, stage 2 %ld; chim_soft_fragments of the emulated run: stage 1 %ld, stage 2 %ld\n", h.soft1, h.soft2, d.soft1, d.soft2);
    const long bad = compare(h, d, E, true);
    std::printf(bad ? "%ld DIFFERENT\n" : "%ld differences: same\n", bad);
    return bad ? 1 : 0;
}
