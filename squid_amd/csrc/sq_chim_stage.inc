// The two chimeric graph stages on the device: RawEdgesChim (SegmentGraph.cpp:1394-1555) and ExactBreakpoint + CountTop (:3019-3081,
// :51-102), restated from the host versions in sq_graph.cpp (chimeric_edges, exact_breakpoints, count_top) -- same multiset of raw edge
// keys, same trimmed blocks, same per-edge breakpoint lists in the same order.  Everything here is either lane-local (one lane = one
// fragment, one soft fragment, one block slot) or one wave per edge group, written in the operations of sq_wave.h, so that
// tools/chim_stage_emu.cpp runs this source on the CPU (SQ_WAVE_EMU) against the host functions; the __global__ wrappers, the two scans
// (device_scan) and the host entry points dev_chimeric_edges / dev_exact_breakpoints are in sq_kernels.hip.
//
// The one thing carried from fragment to fragment is LocateRead's start position: the node of the first block of the last earlier
// fragment whose first block was located.  A first block is *deep* (located in one node from any start: pin[q] = that node), *none*
// (no node can take it: leaves the position alone) or *soft* (its node depends on the incoming position) -- first_block_fit of
// sq_graph.cpp is the definition.  lastdeep[q] = index of the last deep fragment in front of q (exclusive max-scan), spos[q] = number
// of soft fragments in front of q (exclusive sum-scan), soft[] = the soft fragments in fragment order.  A soft fragment whose nearest
// earlier deep fragment lies behind the soft fragment in front of it starts from that deep node and needs nothing else; only runs of soft
// fragments with no deep fragment in between are a chain, and one lane walks such a run in order (soft_resolve).  sout[k] = the
// position behind soft fragment k.  hint_of() then gives every fragment its exact incoming position.
#pragma once
#include "sq_wave.h"
#include "sq_stage_layout.h"
namespace chs {
struct Nodes { int32_t n; const int32_t *chr, *pos, *len; };
// fragment table (SoA, never written by a kernel): blocks of fragment q = [off[q], off[q + 1]), mate a first (na[q] blocks), then mate b
struct Frags {
    int64_t nf, nblk;
    const uint32_t *off, *na;
    const int32_t *atot, *btot;
    const uint8_t* low;  // alow | blow << 1
    const int32_t* refid;
    const uint8_t* rev;
    const int32_t *refpos, *readpos, *matchref, *matchread;  // untrimmed
};
struct Trim { int32_t *refpos, *readpos, *matchref, *matchread; };  // the blocks as the stages trimmed them (stage 1 writes, stage 2 reads and trims further)
struct Blk { int32_t refid, refpos, readpos, matchref, matchread; bool rev; };
struct Params { int32_t dp, di; };
// position chain of one stage
struct Chain { int32_t *pin, *lastdeep, *spos; uint32_t* soft; int32_t* sout; uint8_t* cls; uint32_t soft_cap; };

WV_FN int imin(int a, int b) { return a < b ? a : b; }
WV_FN int imax(int a, int b) { return a > b ? a : b; }
WV_FN int iabs(int a) { return a < 0 ? -a : a; }

// ---- node searches (the nodes tile every chromosome: all predicates are monotone)
struct Fit { int a, bb, lo, hi; bool any; };  // nodes [lo, hi) of the chromosome, fitting range [a, bb]
WV_FN Fit fit_range(const Nodes& N, int refid, int refpos, int end) {
    Fit f;
    int l = 0, h = N.n;
    while (l < h) { const int m = (l + h) >> 1; if (N.chr[m] < refid) l = m + 1; else h = m; }
    f.lo = l;
    h = N.n;
    while (l < h) { const int m = (l + h) >> 1; if (!(refid < N.chr[m])) l = m + 1; else h = m; }
    f.hi = l;
    l = f.lo; h = f.hi;
    while (l < h) { const int m = (l + h) >> 1; if (N.pos[m] + N.len[m] < end - 5) l = m + 1; else h = m; }
    f.a = l;
    l = f.lo; h = f.hi;
    while (l < h) { const int m = (l + h) >> 1; if (!(refpos + 5 < N.pos[m])) l = m + 1; else h = m; }
    f.bb = l - 1;
    f.any = f.a <= f.bb && f.a < f.hi && f.bb >= f.lo;
    return f;
}
// one block of locate_fragment (sq_graph.cpp): i = position of the walk (in/out), hint = where the fragment's search started; trims b
WV_FN int locate_one(const Nodes& N, int& i, int hint, Blk& b) {
    const int n = N.n;
    if (i < 0 || i >= n) i = hint;
    const bool fits = N.chr[i] == b.refid && b.refpos >= N.pos[i] - 5 && b.refpos + b.matchref <= N.pos[i] + N.len[i] + 5;
    if (!fits) {
        const Fit f = fit_range(N, b.refid, b.refpos, b.refpos + b.matchref);
        if (N.chr[i] < b.refid || (N.chr[i] == b.refid && N.pos[i] <= b.refpos)) {
            if (f.any && f.bb >= i) i = imax(i, f.a); else i = imax(i, f.hi);
        } else {
            if (f.any && f.a <= i) i = imin(i, f.bb); else i = imin(i, f.lo - 1);
        }
    }
    if (i < 0 || i >= n || N.chr[i] != b.refid) return -1;
    const int np = N.pos[i], ne = np + N.len[i];
    if (b.refpos < np) { const int d = np - b.refpos; if (!b.rev) b.readpos += d; b.matchref -= d; b.matchread -= d; b.refpos = np; }
    if (b.refpos + b.matchref > ne) { const int d = b.refpos + b.matchref - ne; if (b.rev) b.readpos += d; b.matchref -= d; b.matchread -= d; }
    return i;
}
// first_block_fit of sq_graph.cpp
WV_FN uint8_t first_fit(const Nodes& N, int refid, int refpos, int matchref, int& node) {
    const int end = refpos + matchref;
    const Fit f = fit_range(N, refid, refpos, end);
    node = -1;
    if (!f.any) return CLS_NONE;
    if (f.a == f.bb) {
        const int up = N.pos[f.a], ue = up + N.len[f.a];
        if (refpos >= up && end <= ue && end > up + 5 && refpos < ue - 5) { node = f.a; return CLS_DEEP; }
    }
    return CLS_SOFT;
}
WV_FN int home_node(const Nodes& N, int start, int refid, int refpos) {  // :1408-1409
    const int n = N.n;
    int l = 0, h = n;
    while (l < h) { const int m = (l + h) >> 1; if (N.chr[m] < refid || (N.chr[m] == refid && N.pos[m] + N.len[m] < refpos)) l = m + 1; else h = m; }
    const int i = imax(start, l);
    if (i >= n) return -2;
    l = 0; h = n;
    while (l < h) { const int m = (l + h) >> 1; if (N.chr[m] < refid || (N.chr[m] == refid && N.pos[m] <= refpos)) l = m + 1; else h = m; }
    return imin(i, l - 1);
}
WV_FN unsigned long long edge_key(int i, bool hi, int j, bool hj) {  // edge_pack(make_edge(...))
    int a = i, b = j; bool ha = hi, hb = hj;
    if (i > j) { a = j; ha = hj; b = i; hb = hi; }
    return ((unsigned long long)(uint32_t)a << 32) | ((unsigned long long)(uint32_t)b << 2) | ((unsigned long long)ha << 1) | (unsigned long long)hb;
}
WV_FN bool edge_discordant(const Nodes& N, const Params& P, unsigned long long key) {  // :159-190
    const int a = (int)(key >> 32), b = (int)((key & 0xffffffffull) >> 2);
    if (N.chr[a] != N.chr[b]) return true;
    if (N.pos[b] - N.pos[a] - N.len[a] > P.dp && b - a > P.di) return true;
    return ((key >> 1) & 1) != 0 || (key & 1) != 1;
}
WV_FN Blk load_blk(const Frags& F, const int32_t* refpos, const int32_t* readpos, const int32_t* matchref, const int32_t* matchread, uint32_t k) {
    Blk b;
    b.refid = F.refid[k]; b.rev = F.rev[k] != 0; b.refpos = refpos[k]; b.readpos = readpos[k]; b.matchref = matchref[k]; b.matchread = matchread[k];
    return b;
}
WV_FN Blk load_trimmed(const Frags& F, const Trim& T, uint32_t k) { return load_blk(F, T.refpos, T.readpos, T.matchref, T.matchread, k); }
WV_FN void store_trimmed(const Trim& T, uint32_t k, const Blk& b) { T.refpos[k] = b.refpos; T.readpos[k] = b.readpos; T.matchref[k] = b.matchref; T.matchread[k] = b.matchread; }
// ReadRec_t::IsEndDiscordant (ReadRec.cpp:178-209) over the blocks [o, o + cnt) of one mate
WV_FN bool end_discordant(const Frags& F, const Trim& T, uint32_t o, uint32_t cnt) {
    if (cnt <= 1) return false;
    for (uint32_t k = o; k + 1 < o + cnt; ++k) {
        if (F.refid[k] != F.refid[k + 1] || F.rev[k] != F.rev[k + 1]) return true;
        const bool refup = T.refpos[k] < T.refpos[k + 1], readup = T.readpos[k] < T.readpos[k + 1];
        if (!F.rev[k] && refup != readup) return true;
        if (F.rev[k] && refup == readup) return true;
    }
    return false;
}
// ReadRec_t::IsPairDiscordant(false) (ReadRec.cpp:211-228)
WV_FN bool pair_discordant(const Frags& F, const Trim& T, int64_t q, uint32_t o, uint32_t na, uint32_t nb) {
    if (na == 0 || nb == 0) return false;
    const Blk af = load_trimmed(F, T, o), ab = load_trimmed(F, T, o + na - 1), bf = load_trimmed(F, T, o + na), bb = load_trimmed(F, T, o + na + nb - 1);
    if (af.refid != bb.refid || af.rev == bb.rev) return true;
    if (!af.rev && af.refpos - af.readpos > bb.refpos - (F.btot[q] - bb.readpos - bb.matchread)) return true;
    if (!bf.rev && bf.refpos - bf.readpos > ab.refpos - (F.atot[q] - ab.readpos - ab.matchread)) return true;
    return false;
}
// the pair-edge suppression test of :1484-1502; rn = nodes of the fragment's blocks
WV_FN bool pair_overlap(const int32_t* rn, int na, int nb, bool enda, bool endb, int i, int j) {
    bool ov = false;
    for (int k = 0; k < na; ++k) if (j == rn[k]) ov = true;
    for (int k = 0; k < nb; ++k) if (i == rn[na + k]) ov = true;
    if (na > 1) {
        if (enda) { if ((rn[0] <= j && rn[na - 1] >= j) || (rn[0] >= j && rn[na - 1] <= j)) ov = true; }
        else if (iabs(i - j) < 3) ov = true;
    }
    if (nb > 1) {
        if (endb) { if ((rn[na] <= i && rn[na + nb - 1] >= i) || (rn[na] >= i && rn[na + nb - 1] <= i)) ov = true; }
        else if (iabs(i - j) < 3) ov = true;
    }
    return ov;
}
WV_FN void split_breakpoints(const Blk& x, const Blk& y, int& b1, int& b2) {  // :1435-1440
    b1 = x.rev ? x.refpos : x.refpos + x.matchref;
    b2 = y.rev ? y.refpos + y.matchref : y.refpos;
    const bool xgt = x.refid != y.refid ? x.refid > y.refid : x.refpos > y.refpos;
    if (xgt) { const int t = b1; b1 = b2; b2 = t; }
}
// (key, +1) into the open-addressing table of the concordant edge stage (hash_add of sq_kernels.hip without the wave aggregation)
WV_FN void hash_add(unsigned long long* hk, uint32_t* hv, uint32_t mask, unsigned long long key, uint32_t* flags) {
    uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40) & mask;
    for (uint32_t probe = 0; probe <= mask && probe < 256u; ++probe) {
        const unsigned long long cur = hk[h];
        if (cur == key) { wv::glb_atomic_add(&hv[h], 1u); return; }
        if (cur == ~0ull) {
            const unsigned long long old = wv::glb_atomic_cas64(&hk[h], ~0ull, key);
            if (old == ~0ull || old == key) { wv::glb_atomic_add(&hv[h], 1u); return; }
        }
        h = (h + 1) & mask;
    }
    wv::glb_atomic_or(flags, FLAG_FULL);
}

// ---- the position chain
WV_FN bool frag_skipped(int stage, uint32_t na, uint32_t nb) { return stage == 1 ? na + nb == 0 : (na <= 1 && nb <= 1); }
// one lane per fragment; refpos / matchref: the blocks the stage starts from (stage 1: untrimmed, stage 2: as stage 1 left them)
WV_FN void classify(const Nodes& N, const Frags& F, const int32_t* refpos, const int32_t* matchref, int stage, const Chain& C, int64_t q) {
    if (q >= F.nf) return;
    const uint32_t o = F.off[q], na = F.na[q], nb = F.off[q + 1] - o - na;
    int node = -1;
    uint8_t cls = CLS_NONE;
    if (!frag_skipped(stage, na, nb)) cls = first_fit(N, F.refid[o], refpos[o], matchref[o], node);
    C.cls[q] = cls;
    C.pin[q] = cls == CLS_DEEP ? node : -1;
}
WV_FN void soft_list(const Frags& F, const Chain& C, int64_t q) {
    if (q >= F.nf) return;
    if (C.cls[q] == CLS_SOFT && (uint32_t)C.spos[q] < C.soft_cap) C.soft[C.spos[q]] = (uint32_t)q;
}
WV_FN bool soft_follows(const Chain& C, uint32_t k) { return k > 0 && (int32_t)C.soft[k - 1] > C.lastdeep[C.soft[k]]; }  // no deep fragment between soft k - 1 and soft k
// one lane per soft fragment; the lane of the first one of a run walks the run
WV_FN void soft_resolve(const Nodes& N, const Frags& F, const int32_t* refpos, const int32_t* readpos, const int32_t* matchref, const int32_t* matchread, const Chain& C,
                        uint32_t nsoft, uint32_t k) {
    if (k >= nsoft || soft_follows(C, k)) return;
    const int d = C.lastdeep[C.soft[k]];
    int h = d >= 0 ? C.pin[d] : 0;
    for (uint32_t j = k;;) {
        Blk b = load_blk(F, refpos, readpos, matchref, matchread, F.off[C.soft[j]]);
        int i = h;
        const int r = locate_one(N, i, h, b);
        if (r != -1) h = r;
        C.sout[j] = h;
        if (++j >= nsoft || !soft_follows(C, j)) break;
    }
}
WV_FN int hint_of(const Chain& C, int64_t q) {
    const int d = C.lastdeep[q];
    const uint32_t ks = (uint32_t)C.spos[q];
    if (ks > 0 && ks - 1 < C.soft_cap && (int32_t)C.soft[ks - 1] > d) return C.sout[ks - 1];
    return d >= 0 ? C.pin[d] : 0;
}

// ---- stage 1: locate, trim, emit the raw edge keys (one lane per fragment)
WV_FN void stage1_fragment(const Nodes& N, const Frags& F, const Trim& T, int32_t* rn, const Chain& C, const Params& P, unsigned long long* hk, uint32_t* hv, uint32_t mask,
                           uint32_t* flags, int64_t q) {
    if (q >= F.nf) return;
    const uint32_t o = F.off[q], nblk = F.off[q + 1] - o, na = F.na[q], nb = nblk - na;
    if (nblk == 0) return;
    int hint = hint_of(C, q);
    int i = hint;
    for (uint32_t k = 0; k < nblk; ++k) {
        Blk b = load_blk(F, F.refpos, F.readpos, F.matchref, F.matchread, o + k);
        rn[o + k] = locate_one(N, i, hint, b);
        store_trimmed(T, o + k, b);
    }
    if (rn[o] != -1) hint = rn[o];
    const int n = N.n;
    for (uint32_t k = 0; k < nblk; ++k)
        if (rn[o + k] == -1) {
            const int h = home_node(N, hint, F.refid[o + k], T.refpos[o + k]);
            if (h < 0 || h + 1 >= n) { wv::glb_atomic_or(flags, FLAG_ASSERT); return; }
            hash_add(hk, hv, mask, edge_key(h, false, h + 1, true), flags);
        }
    for (int mate = 0; mate < 2; ++mate) {
        const uint32_t base = mate ? o + na : o, cnt = mate ? nb : na;
        for (uint32_t k = base; k + 1 < base + cnt; ++k) {
            const int a = rn[k], b = rn[k + 1];
            if (a == b || a == -1 || b == -1) continue;
            hash_add(hk, hv, mask, edge_key(a, F.rev[k] != 0, b, F.rev[k + 1] == 0), flags);
        }
    }
    if (na > 0 && nb > 0) {
        const bool enda = end_discordant(F, T, o, na), endb = end_discordant(F, T, o + na, nb);
        if (!enda && !endb) {
            const int a = rn[o + na - 1], b = rn[o + nblk - 1];
            if (a != b && a != -1 && b != -1 && !pair_overlap(rn + o, (int)na, (int)nb, enda, endb, a, b)) {
                const unsigned long long key = edge_key(a, F.rev[o + na - 1] != 0, b, F.rev[o + nblk - 1] != 0);
                if (!edge_discordant(N, P, key) || pair_discordant(F, T, q, o, na, nb)) hash_add(hk, hv, mask, key, flags);
            }
        }
    }
}

// ---- stage 2: locate on the final nodes, trim further, one hit slot per block (slot k = the split between blocks k and k + 1)
WV_FN void stage2_fragment(const Nodes& N, const Frags& F, const Trim& T, int32_t* rn, const Chain& C, const Params& P, const unsigned long long* ekey, int32_t m,
                           int32_t* hit_e, int32_t* hit_b1, int32_t* hit_b2, uint32_t* hist, int64_t q) {
    if (q >= F.nf) return;
    const uint32_t o = F.off[q], nblk = F.off[q + 1] - o, na = F.na[q], nb = nblk - na;
    if (frag_skipped(2, na, nb)) return;
    const int hint = hint_of(C, q);
    int i = hint;
    for (uint32_t k = 0; k < nblk; ++k) {
        Blk b = load_trimmed(F, T, o + k);
        rn[o + k] = locate_one(N, i, hint, b);
        store_trimmed(T, o + k, b);
    }
    for (int mate = 0; mate < 2; ++mate) {
        const uint32_t base = mate ? o + na : o, cnt = mate ? nb : na;
        for (uint32_t k = base; k + 1 < base + cnt; ++k) {
            const int a = rn[k], b = rn[k + 1];
            if (a == b || a == -1 || b == -1) continue;
            const unsigned long long key = edge_key(a, F.rev[k] != 0, b, F.rev[k + 1] == 0);
            if (!edge_discordant(N, P, key)) continue;
            int l = 0, h = m;  // call_sv only ever looks up the keys of final edges
            while (l < h) { const int mid = (l + h) >> 1; if (ekey[mid] < key) l = mid + 1; else h = mid; }
            if (l >= m || ekey[l] != key) continue;
            int b1, b2;
            split_breakpoints(load_trimmed(F, T, k), load_trimmed(F, T, k + 1), b1, b2);
            hit_e[k] = l; hit_b1[k] = b1; hit_b2[k] = b2;
            wv::glb_atomic_add(&hist[l], 1u);
        }
    }
}
// one lane per block slot: the hits grouped by edge (goff = exclusive scan of hist; the order inside a group is not defined and not needed)
WV_FN void scatter_hit(int64_t nblk, const int32_t* hit_e, const int32_t* hit_b1, const int32_t* hit_b2, const int32_t* goff, uint32_t* cursor, int32_t* p1, int32_t* p2, int64_t k) {
    if (k >= nblk) return;
    const int e = hit_e[k];
    if (e < 0) return;
    const uint32_t at = (uint32_t)goff[e] + wv::glb_atomic_add(&cursor[e], 1u);
    p1[at] = hit_b1[k]; p2[at] = hit_b2[k];
}

// ---- CountTop (:51-102), one wave per edge.  Scores are 2 x the reference's (equal pair +2, other pair at Manhattan distance < 10 +1;
// `score > 3` is `> 6`).  The reference works on the sorted unique pairs; here every hit carries the score of its pair (equal pairs get
// equal scores), the best is the highest score with ties to the lexicographically smallest pair -- what max_element over the sorted
// unique list returns --, and zeroing a pair zeroes all its copies.  Any group size: the pairs stay in global memory (L2), a tile of 64
// crosses the wave through readlane.  out_n[e] = 0 (no hit) .. 5, out_xy[10 e ..] = the accepted pairs in the order of acceptance.
WV_FN bool better(int s, int x, int y, int s0, int x0, int y0) { return s > s0 || (s == s0 && (x < x0 || (x == x0 && y < y0))); }
WV_FN void count_top_wave(int32_t e, const int32_t* goff, const int32_t* p1, const int32_t* p2, int32_t* score, bool ha, bool hb, int32_t* out_n, int32_t* out_xy) {
    const int lane = wv::lane();
    const int base = goff[e], n = goff[e + 1] - base;
    if (n <= 0) { if (lane == 0) out_n[e] = 0; return; }  // (uniform)
    const int32_t *X = p1 + base, *Y = p2 + base;
    int32_t* S = score + base;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int x = i < n ? X[i] : 0, y = i < n ? Y[i] : 0;
        int s = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const uint32_t tx = (uint32_t)(j < n ? X[j] : 0), ty = (uint32_t)(j < n ? Y[j] : 0);
            const int cnt = imin(64, n - j0);
            for (int t = 0; t < cnt; ++t) {
                const int px = (int)wv::bcast(tx, t), py = (int)wv::bcast(ty, t);
                if (px == x && py == y) s += 2;
                else if (iabs(x - px) + iabs(y - py) < 10) s += 1;
            }
        }
        if (i < n) S[i] = s;
    }
    int acc = 0, ax[5], ay[5];
    while (acc < 5) {
        int bs = -1, bx = 0, by = 0;
        for (int i = lane; i < n; i += 64) { const int s = S[i]; if (bs < 0 || better(s, X[i], Y[i], bs, bx, by)) { bs = s; bx = X[i]; by = Y[i]; } }
        for (int d = 32; d >= 1; d >>= 1) {
            const int os = (int)wv::shfl((uint32_t)bs, lane ^ d), ox = (int)wv::shfl((uint32_t)bx, lane ^ d), oy = (int)wv::shfl((uint32_t)by, lane ^ d);
            if (os >= 0 && (bs < 0 || better(os, ox, oy, bs, bx, by))) { bs = os; bx = ox; by = oy; }
        }
        if (!(bs > 6)) break;  // (uniform: every lane holds the same best)
        bool far = true;
        for (int k = 0; k < acc; ++k) if (iabs(ax[k] - bx) + iabs(ay[k] - by) < 50) far = false;
        if (far) { ax[acc] = bx; ay[acc] = by; ++acc; }
        for (int i = lane; i < n; i += 64) if (X[i] == bx && Y[i] == by) S[i] = 0;  // (a lane only ever reads the scores it writes)
    }
    if (acc == 0) {  // bounding box (:95-100)
        int lo1 = 0x7fffffff, lo2 = 0x7fffffff, hi1 = 0, hi2 = 0;
        for (int i = lane; i < n; i += 64) { lo1 = imin(lo1, X[i]); hi1 = imax(hi1, X[i]); lo2 = imin(lo2, Y[i]); hi2 = imax(hi2, Y[i]); }
        for (int d = 32; d >= 1; d >>= 1) {
            lo1 = imin(lo1, (int)wv::shfl((uint32_t)lo1, lane ^ d)); hi1 = imax(hi1, (int)wv::shfl((uint32_t)hi1, lane ^ d));
            lo2 = imin(lo2, (int)wv::shfl((uint32_t)lo2, lane ^ d)); hi2 = imax(hi2, (int)wv::shfl((uint32_t)hi2, lane ^ d));
        }
        ax[0] = ha ? lo1 : hi1; ay[0] = hb ? lo2 : hi2; acc = 1;
    }
    if (lane == 0) {
        out_n[e] = acc;
        for (int k = 0; k < acc; ++k) { out_xy[10 * e + 2 * k] = ax[k]; out_xy[10 * e + 2 * k + 1] = ay[k]; }
    }
}
}  // namespace chs
