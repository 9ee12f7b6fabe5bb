// BuildNode_STAR's segmentation automaton on the device (sq_segment_on_device): the control automaton of SegmentGraph.cpp:354-646 that turns
// every passed discordant cluster into seed nodes (Seg::process_cluster / replay_range of sq_segment.cpp).  Written in the operations of
// sq_wave.h, so that tools/segment_emu.cpp runs this source on the CPU (SQ_WAVE_EMU) against the host automaton in one go; the __global__
// wrapper and the host entry dev_segment_run are in sq_kernels.hip.
//
// What the automaton reads is all made by segment_clusters / segment_scan / segment_prepare: the sorted discordant blocks plus the zero
// sentinel, PartAlignPos, the cluster table, the ConcordRest candidates per cluster (CSR, sorted by refpos), the trigger of every cluster, the
// active stretches with their first cluster, and the 24-byte summaries of the records inside them.  Only the last node emitted so far
// crosses a stretch boundary (the other carried values are functions of the cluster at hand), so ONE WAVE RUNS EACH ACTIVE STRETCH from a
// fresh state on the guess "a node exists in front and is too far away to matter" (replay_range's virtual_back).  The wave does not trust
// the guess, it reports what the guess rested on: every comparison with the node in front before the wave's own first node is a threshold
// on that node's end on one chromosome -- the row keeps the lowest chromosome touched and the tightest bound there: the guess held iff the
// real node lies on an earlier chromosome, or on that one and ends at or before the bound --; the one comparison without a chromosome test
// (:623) is kept as values (R_SENS, a short list); F_EXIST says that the mere existence of a node was used (step 1 of :531-561), so a row
// without it is valid with and without a node in front.  The host walks the rows in stretch order with the real last node and runs a
// stretch whose conditions do not hold, or that hit a capacity (margin list, nodes, sens list, guard), again with replay_range.
//
// Inside a wave control flow is uniform.  Windows are not storage: a window is the range [offset, window end) of the stretch's summaries
// filtered by class (SR_CONC without / with SR_PART); offsets are record indices.  The margin list of a sub-cluster is assembled and sorted
// (bitonic) in LDS; the counts sr / pl / pr and the spanning cover of a break candidate do not depend on the node state and are computed
// for 64 candidates at a time, one per lane, by uniform loops over the blocks, the windows and the ConcordRest candidates; the chain
// skip / lastC / lastSup / markStart runs as a uniform serial pass over the ballot of the candidates that passed.  The first window advance
// (step 1) finds its first failing element by ballot; the second one depends on concord0pos through its break and walks element by element.
#pragma once
#include "sq_wave.h"
#include "sq_stage_layout.h"
#ifndef SGS_TRACE
#define SGS_TRACE(kind, value) ((void)0)  // (the CPU harness counts what its cases contained through these; nothing on the device)
#define SGS_TRACE_WINDOWS(S) ((void)0)
#endif
namespace sgs {
struct Tab {
    const Rec* recs;
    int32_t RL, nd, ncl, npart, na, K_eff;
    const int32_t* d4;      // nd + 1 blocks: refid, refpos, matchref, rev
    const int32_t* part2;   // first, second
    const int32_t* cl4;     // ds, de, chr, right
    const int32_t *rest_off, *rest_pos, *rest_len, *trigger;
    const int32_t* stretch; // na rows of STRETCH
};
WV_FN int imax(int a, int b) { return a > b ? a : b; }
WV_FN int imin(int a, int b) { return a < b ? a : b; }
WV_FN int wave_max(int v) { for (int d = 1; d < 64; d <<= 1) v = imax(v, (int)wv::shfl((uint32_t)v, wv::lane() ^ d)); return v; }

struct St {
    const Tab* X;
    const Rec* R;   // R[kept index]
    wv::lds_u32* M;
    int wend, co, po;
    int kc, ds, de, dcur, ps, pe;
    int disChr, nextdisChr, disright, nextdisright, markStart, markChr;
    int nown, bchr, bpos, blen;  // the wave's own nodes so far and the last of them (nown == 0: the node in front, which is a guess)
    int flags, minchr, bound, nsens, ext0, ext1, ext2, nclusters, nsubs, mmax;
    int32_t *nodes, *row;
    int node_cap;
};
WV_FN int dref(const St& S, int d) { return S.X->d4[4 * d]; }
WV_FN int dpos(const St& S, int d) { return S.X->d4[4 * d + 1]; }
WV_FN int dend(const St& S, int d) { return S.X->d4[4 * d + 1] + S.X->d4[4 * d + 2]; }
WV_FN bool drev(const St& S, int d) { return S.X->d4[4 * d + 3] != 0; }
WV_FN int back_end(const St& S) { return S.bpos + S.blen; }
WV_FN int rend(const Rec& r) { return r.fb_refpos + r.fb_matchref; }

// the first record of window class `want` in [from, end) for which pred holds (end: none)
template <class F> WV_FN int first_of(const St& S, uint8_t want, int from, int end, F pred) {
    for (int base = from; base < end; base += 64) {
        const int q = base + wv::lane();
        bool ok = false;
        if (q < end) { const Rec r = S.R[q]; ok = (r.flags & W_MASK) == want && pred(r); }
        const unsigned long long m = wv::ballot(ok);
        if (m) return base + wv::ctz64(m);
    }
    return end;
}
WV_FN int next_of(const St& S, uint8_t want, int from, int end) { return first_of(S, want, from, end, [](const Rec&) { return true; }); }
WV_FN int last_of(const St& S, uint8_t want, int from, int end) {  // (-1: none)
    for (int top = end; top > from; top -= 64) {
        const int q = top - 1 - wv::lane();
        const unsigned long long m = wv::ballot(q >= from && (S.R[q >= from ? q : from].flags & W_MASK) == want);
        if (m) return top - 1 - wv::ctz64(m);
    }
    return -1;
}
// the largest end of the class elements in [from, to) (INT32_MIN: none)
WV_FN int max_end(const St& S, uint8_t want, int from, int to) {
    int m = INT32_MIN;
    for (int base = from; base < to; base += 64) { const int q = base + wv::lane(); if (q < to) { const Rec r = S.R[q]; if ((r.flags & W_MASK) == want) m = imax(m, rend(r)); } }
    return wave_max(m);
}
// a comparison with the node in front that came out the way the guess says: it holds for a real node on an earlier chromosome than chr, or
// on chr with an end <= b
WV_FN void consult(St& S, int chr, int b) {
    if (S.nown != 0) return;
    S.flags |= F_CONSULTED;
    if (chr < S.minchr) { S.minchr = chr; S.bound = b; }
    else if (chr == S.minchr) S.bound = imin(S.bound, b);
}
WV_FN void emit(St& S, int chr, int pos, int len) {
    if (S.nown < S.node_cap) { if (wv::lane() == 0) { S.nodes[3 * S.nown] = chr; S.nodes[3 * S.nown + 1] = pos; S.nodes[3 * S.nown + 2] = len; } }
    else S.flags |= F_NODES_FULL;
    ++S.nown; S.bchr = chr; S.bpos = pos; S.blen = len;
}
WV_FN void extend(St& S, int by) {  // out.back().len += by, on a node of the wave's own
    S.blen += by;
    if (S.nown <= S.node_cap && wv::lane() == 0) S.nodes[3 * (S.nown - 1) + 2] = S.blen;
}
WV_FN void new_cluster(St& S) {
    const Tab& X = *S.X;
    ++S.kc;
    S.disright = S.nextdisright; S.disChr = S.nextdisChr;
    if (S.kc < X.ncl) { const int32_t* k = X.cl4 + 4 * S.kc; S.ds = k[0]; S.de = k[1]; S.nextdisChr = k[2]; S.nextdisright = k[3]; }
    else { S.ds = S.de = X.nd; S.nextdisright = 0; }  // past the last cluster: the zero sentinel (ledger B21); nextdisChr keeps its value
}
WV_FN void close_node(St& S, int chr, int& curStart, int& curEnd, int lastC, bool& split) {  // :483-493 / :506-515
    split = true;
    const int p = dpos(S, S.ds);
    if (p - curStart > NEAR && lastC - p > NEAR) { emit(S, chr, curStart, p - curStart); curStart = p; }
    emit(S, chr, curStart, lastC - curStart);
    curStart = lastC; curEnd = lastC;
    S.markStart = lastC; S.markChr = chr;
}
WV_FN void m_put(St& S, int at, int v) { if (at < M_CAP) S.M[at] = (uint32_t)v; }
WV_FN int m_get(const St& S, int at) { return (int)S.M[at]; }
WV_FN int m_lower(const St& S, int n, int x) { int a = 0, b = n; while (a < b) { const int m = (a + b) >> 1; if (m_get(S, m) < x) a = m + 1; else b = m; } return a; }  // lane-local
// FP64 with one rounding per operation, in the reference's order (-ffp-contract=off; the division is the IEEE one)
WV_FN bool dense(int disStart, int disEnd, int disCount, int RL) {
    if (disStart == -1) return false;
    const double v = 4.0 * (double)(disEnd - disStart) / (double)RL;
    const double m = v < 5.0 ? v : 5.0;  // std::min(5.0, v)
    return (double)disCount > m;
}

// one discordant cluster has been passed by record (recChr, recPos): SegmentGraph.cpp:354-611 (Seg::process_cluster)
WV_FN void process_cluster(St& S, int recChr, int recPos) {
    const Tab& X = *S.X;
    const int L = wv::lane(), RL = X.RL, nd = X.nd, wend = S.wend;
    int curEnd = 0, curStart = 0, disStart = -1, disEnd = -1, disCount = -1;
    bool split = false;
    ++S.nclusters;
    const int chr0 = dref(S, S.ds), pos0 = dpos(S, S.ds);
    if (S.markStart != -1 && chr0 != S.markChr) { S.markChr = -1; S.markStart = -1; SGS_TRACE(T_CHR_CHANGE, 0); }
    S.co = first_of(S, W_C, S.co, wend, [&](const Rec& r) { return !(r.refid < chr0); });
    S.po = first_of(S, W_P, S.po, wend, [&](const Rec& r) { return !(r.refid < chr0); });
    if (S.co < wend) { const Rec b = S.R[last_of(S, W_C, S.co, wend)]; if (pos0 > rend(b) + RL) S.co = wend; }
    if (S.po < wend) { const Rec b = S.R[last_of(S, W_P, S.po, wend)]; if (pos0 > rend(b) + RL) S.po = wend; }
    SGS_TRACE_WINDOWS(S);
    SGS_TRACE(T_BLOCKS, S.de - S.ds);
    curStart = pos0;
    {
        const bool hc = S.co < wend, hp = S.po < wend;
        int tr = 0, tp = 0;
        if (hc && hp) {
            const Rec x = S.R[S.co], y = S.R[S.po];
            const bool less = x.refid != y.refid ? x.refid < y.refid : x.fb_refpos < y.fb_refpos;
            tr = less ? x.refid : y.refid; tp = less ? x.fb_refpos : y.fb_refpos;
        } else if (hc) { tr = S.R[S.co].refid; tp = S.R[S.co].fb_refpos; }
        else if (hp) { tr = S.R[S.po].refid; tp = S.R[S.po].fb_refpos; }
        if ((hc || hp) && (tr < chr0 || (tr == chr0 && tp < pos0))) curStart = tp;
    }
    curStart = imax(curStart, S.markStart);
    {   // ps / pe: lower bounds in the sorted PartAlignPos (the host's running pointers reach the same places)
        int a = 0, b = X.npart;
        while (a < b) { const int m = (a + b) >> 1; const int f = X.part2[2 * m], s = X.part2[2 * m + 1]; if (f < chr0 || (f == chr0 && s + RL < pos0)) a = m + 1; else b = m; }
        S.ps = a; b = X.npart;
        while (a < b) { const int m = (a + b) >> 1; if (X.part2[2 * m] == chr0 && X.part2[2 * m + 1] < S.nextdisright + RL) a = m + 1; else b = m; }
        S.pe = a;
    }
    const int guard_max = 4 * (S.de - S.ds) + 64;
    int guard = 0;
    while (S.ds != S.de) {
        if (++guard > guard_max) { S.flags |= F_GUARD; S.ds = S.de; break; }
        const int ds = S.ds, de = S.de;
        const int chr = dref(S, ds);
        if (ds != 0 && chr != dref(S, ds - 1)) { SGS_TRACE(T_CHR_CHANGE, 1); if (S.co >= wend && S.po >= wend) curStart = dpos(S, ds); }
        split = false;
        ++S.nsubs;
        SGS_TRACE(T_SUB, guard - 1);
        // ---- the margin list: the leading run of blocks that touch, the blocks that start within `thresh` behind it, clip positions
        int nm = 0, dcur = de;
        for (int base = ds; base < de; base += 64) {
            const int d = base + L;
            const bool v = d < de;
            const int p = v ? dpos(S, d) : 0, e = v ? dend(S, d) : 0;
            const unsigned long long bm = wv::ballot(v && d + 1 != de && dpos(S, d + 1) > e);
            const int nin = bm ? wv::ctz64(bm) + 1 : imin(64, de - base);
            if (L < nin) { m_put(S, nm + 2 * L, p); m_put(S, nm + 2 * L + 1, e); }
            curEnd = imax(curEnd, wave_max(L < nin ? e : INT32_MIN));
            nm += 2 * nin;
            if (bm) { dcur = base + wv::ctz64(bm); break; }
        }
        disStart = imax(curStart, dpos(S, ds));
        disEnd = curEnd;
        disCount = dcur - ds;
        if (dcur != de)
            for (int base = dcur + 1; base < de; base += 64) {
                const int d = base + L;
                const bool v = d < de;
                const int p = v ? dpos(S, d) : 0, e = v ? dend(S, d) : 0;
                const unsigned long long stop = wv::ballot(v && !(p < curEnd + THRESH));
                const int nin = stop ? wv::ctz64(stop) : imin(64, de - base);
                if (L < nin) { m_put(S, nm + 2 * L, p); m_put(S, nm + 2 * L + 1, e); }
                nm += 2 * nin;
                if (stop) break;
            }
        for (int base = S.ps; base < S.pe; base += 64) {
            const int q = base + L;
            const bool v = q < S.pe;
            const int s = v ? X.part2[2 * q + 1] : 0;
            const unsigned long long stop = wv::ballot(v && !(s < curEnd + THRESH));
            const int nin = stop ? wv::ctz64(stop) : imin(64, S.pe - base);
            if (L < nin) m_put(S, nm + L, s);
            nm += nin;
            if (stop) break;
        }
        {
            const int front = dpos(S, ds);
            for (int base = S.po; base < wend; base += 64) {  // clipped reads of the partial window next to the run
                const int q = base + L;
                bool take = false;
                int val = 0;
                if (q < wend) {
                    const Rec r = S.R[q];
                    if ((r.flags & W_MASK) == W_P && r.refid == chr) {
                        const int p = r.fb_refpos, e = rend(r);
                        const bool rev = (r.flags & W_REV) != 0;
                        const bool inp = p > front - THRESH && p < curEnd + THRESH, ine = e > front - THRESH && e < curEnd + THRESH;
                        if (r.fb_readpos > 15 && inp) { if (rev && ine) { take = true; val = e; } else if (!rev) { take = true; val = p; } }
                        else { if (rev && inp) { take = true; val = p; } else if (!rev && ine) { take = true; val = e; } }
                        if (take) SGS_TRACE(T_CLIP, rev ? 1 : 0);
                    }
                }
                const unsigned long long wm = wv::ballot(take);
                if (take) m_put(S, nm + wv::popc64(wm & wv::lanemask_lt()), val);
                nm += wv::popc64(wm);
            }
        }
        S.mmax = imax(S.mmax, nm);
        SGS_TRACE(T_MARGIN, nm);
        if (nm > M_CAP) { S.flags |= F_M_FULL; S.ds = S.de; break; }
        {   // sort (bitonic, padded to a power of two)
            int n2 = 64;
            while (n2 < nm) n2 <<= 1;
            for (int i = nm + L; i < n2; i += 64) S.M[i] = (uint32_t)INT32_MAX;
            wv::sync();
            for (int k = 2; k <= n2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = L; t < n2 / 2; t += 64) {
                        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                        const int a = m_get(S, i), b = m_get(S, p);
                        if ((a > b) == ((i & k) == 0)) { S.M[i] = (uint32_t)b; S.M[p] = (uint32_t)a; }
                    }
                    wv::sync();
                }
        }
        const int rest_n = S.kc < X.ncl ? X.rest_off[S.kc + 1] - X.rest_off[S.kc] : 0;
        const int32_t *rest_p = X.rest_pos + (S.kc < X.ncl ? X.rest_off[S.kc] : 0), *rest_l = X.rest_len + (S.kc < X.ncl ? X.rest_off[S.kc] : 0);
        const int wfrom = imin(S.co, S.po);
        // ---- the break candidates, 64 at a time
        int lastC = -1, lastSup = 0;
        for (int base = 0; base < nm; base += 64) {
            const int i = base + L;
            const bool v = i < nm;
            const int brk = v ? m_get(S, i) : 0;
            const bool first = v && (i == 0 || m_get(S, i - 1) != brk);
            const int maxbrk = m_get(S, imin(base + 63, nm - 1));
            int sr = 0, pl = 0, pr = 0;
            if (first) sr = m_lower(S, nm, brk + THRESH) - m_lower(S, nm, brk - THRESH + 1);  // |brk - M[k]| < thresh
            for (int d = ds; d < de; ++d) {  // forward blocks ending in (brk - RL, brk), reverse blocks starting in (brk, brk + RL)
                const int p = dpos(S, d), e = dend(S, d);
                if (p >= maxbrk + RL) break;
                if (drev(S, d)) pr += (p > brk && p < brk + RL) ? 1 : 0; else pl += (e < brk && e > brk - RL) ? 1 : 0;
            }
            const bool need = first && (sr > 3 || sr + pl > 4 || sr + pr > 4);
            bool pass = false;
            if (wv::any(need)) {
                int cov = 0;  // blocks that span the candidate: p < brk - thresh and p + m >= brk + thresh
                for (int q = wfrom; q < wend; ++q) {
                    const Rec r = S.R[q];
                    const uint8_t cl = r.flags & W_MASK;
                    if (((cl == W_C && q >= S.co) || (cl == W_P && q >= S.po)) && r.refid == chr) cov += (rend(r) >= brk + THRESH && r.fb_refpos < brk - THRESH) ? 1 : 0;
                }
                for (int d = ds; d < de; ++d) {
                    const int p = dpos(S, d);
                    if (p >= maxbrk - THRESH) break;
                    if (dref(S, d) == chr) cov += (dend(S, d) >= brk + THRESH && p < brk - THRESH) ? 1 : 0;
                }
                const bool pass1 = need && sr > imax(cov - sr, 0) + 2;
                if (rest_n && wv::any(pass1))
                    for (int q = 0; q < rest_n; ++q) {  // (same chromosome by construction, see k_rest_candidates)
                        const int p = rest_p[q];
                        if (p >= maxbrk - THRESH) break;
                        if (pass1) cov += (p + rest_l[q] >= brk + THRESH && p < brk - THRESH) ? 1 : 0;
                    }
                pass = pass1 && sr > imax(cov - sr, 0) + 2;
                if (pass1 && !pass) SGS_TRACE(T_REST_FAIL, 0);
            }
            const int sup = imax(sr + pl, sr + pr);
            unsigned long long m = wv::ballot(pass);
            while (m) {  // the chain that depends on the nodes: in candidate order, uniform
                const int l = wv::ctz64(m);
                m &= m - 1;
                const int b = (int)wv::bcast((uint32_t)brk, l), s = (int)wv::bcast((uint32_t)sup, l);
                bool skip = false;
                if (S.nown > 0) skip = S.bchr == chr && b - back_end(S) < NEAR; else consult(S, chr, b - NEAR);
                if (skip) continue;
                if (lastC == -1 && b - curStart < NEAR) { S.markStart = curStart; S.markChr = chr; }
                else if ((lastC == -1 || b - lastC < NEAR) && s > lastSup) { lastC = b; lastSup = s; }
                else if (b - lastC >= NEAR) { close_node(S, chr, curStart, curEnd, lastC, split); lastC = b; }
            }
        }
        if (lastC != -1 && (!split || back_end(S) != lastC)) close_node(S, chr, curStart, curEnd, lastC, split);
        const bool many = dense(disStart, disEnd, disCount, RL);
        if (many) SGS_TRACE(T_DENSE, split ? 1 : 0);
        if (many && !split) {  // :518-527
            const int lchr = dref(S, de - 1);
            bool ext = false;
            if (S.nown > 0) ext = S.bchr == lchr && disEnd - back_end(S) < NEAR; else consult(S, lchr, disEnd - NEAR);
            if (ext) { extend(S, disEnd - back_end(S)); ++S.ext0; } else emit(S, lchr, disStart, disEnd - disStart);
            curStart = disEnd; curEnd = disEnd;
            S.markStart = disEnd; S.markChr = chr;
        }
        wv::sync();  // (the margin list is read by all lanes before the next round writes it)
        S.co = first_of(S, W_C, S.co, wend, [&](const Rec& r) { return !(r.refid < chr); });
        S.po = first_of(S, W_P, S.po, wend, [&](const Rec& r) { return !(r.refid < chr); });
        dcur = de;
        for (int base = ds; base < de; base += 64) {  // the blocks that end inside what is decided
            const int d = base + L;
            const unsigned long long stop = wv::ballot(d < de && !(dend(S, d < de ? d : ds) <= curEnd));
            if (stop) { dcur = base + wv::ctz64(stop); break; }
        }
        S.dcur = dcur;
        int zero = curStart;  // concord0pos
        const int dn_ref = dref(S, dcur), dn_pos = dpos(S, dcur);
        // step 1 (:531-561): nothing it tests depends on concord0pos -- the first failing element by ballot
        for (int w = 0; w < 2; ++w) {
            const uint8_t want = w ? W_P : W_C;
            const int off = w ? S.po : S.co;
            if (off >= wend) continue;
            auto two = [&](const Rec& r) { return !(r.refid > chr) && !(dcur != nd && r.refid == dn_ref && rend(r) + RL >= dn_pos); };
            int stop = off;
            if (S.nown == 0) {  // the guess: the node in front lies before every element, so the first one already fails
                const Rec r = S.R[off];
                if (two(r)) { S.flags |= F_EXIST; consult(S, r.refid, r.fb_refpos); }
            } else {
                const int bc = S.bchr, be = back_end(S);
                stop = first_of(S, want, off, wend, [&](const Rec& r) { return !(two(r) && !(r.refid > bc || (r.refid == bc && r.fb_refpos >= be))); });
                if (stop > off) zero = imax(zero, max_end(S, want, off, stop));
            }
            if (w) S.po = stop; else S.co = stop;
        }
        // step 2 (:563-603): its break depends on concord0pos
        for (;;) {
            const bool ce = S.co >= wend, pe = S.po >= wend;
            bool cfree = ce, pfree = pe;
            if (!ce) { const Rec r = S.R[S.co]; cfree = r.refid != S.markChr || r.fb_refpos > zero + RL; }
            if (!pe) { const Rec r = S.R[S.po]; pfree = r.refid != S.markChr || r.fb_refpos > zero; }
            if (S.markStart != -1 && (recChr > S.markChr || recPos > zero + RL) && cfree && pfree) {
                if (zero > S.markStart && zero < S.markStart + NEAR) {
                    if (S.nown > 0 && S.bchr == S.markChr) { extend(S, zero - back_end(S)); ++S.ext1; }
                    else { if (S.nown == 0) consult(S, S.markChr, INT32_MIN); emit(S, S.markChr, S.markStart, zero - S.markStart); }
                } else if (zero > S.markStart) emit(S, S.markChr, S.markStart, zero - S.markStart);
                curStart = zero;
                S.markChr = -1; S.markStart = -1;
                break;
            }
            bool f1 = false, f2 = false;
            if (!ce) { const Rec r = S.R[S.co]; f1 = dcur == nd || r.refid < dn_ref || (r.refid == dn_ref && rend(r) + RL < dn_pos); if (f1) { zero = imax(zero, rend(r)); S.co = next_of(S, W_C, S.co + 1, wend); } }
            if (!pe) { const Rec r = S.R[S.po]; f2 = dcur == nd || r.refid < dn_ref || (r.refid == dn_ref && rend(r) + RL < dn_pos); if (f2) { zero = imax(zero, rend(r)); S.po = next_of(S, W_P, S.po + 1, wend); } }
            if (!f1 && !f2) break;
            if (S.co >= wend && S.po >= wend) break;
        }
        S.ds = dcur;
    }
    new_cluster(S);
}
// window pruning as of a record on chromosome refid (:637-646)
WV_FN void prune_all(St& S, int refid) {
    const int wend = S.wend, dn_ref = dref(S, S.ds);
    for (int w = 0; w < 2; ++w) {
        const uint8_t want = w ? W_P : W_C;
        int off = first_of(S, want, w ? S.po : S.co, wend, [&](const Rec& r) { return r.refid == refid; });
        if (S.nown > 0) {
            const int bc = S.bchr, be = back_end(S);
            off = first_of(S, want, off, wend, [&](const Rec& r) { return !(r.refid < dn_ref || (r.refid == bc && r.fb_refpos < be)); });
        } else {
            off = first_of(S, want, off, wend, [&](const Rec& r) { return !(r.refid < dn_ref); });
            if (off < wend) consult(S, S.R[off].refid, S.R[off].fb_refpos);
        }
        if (w) S.po = off; else S.co = off;
    }
}
// events (+ the zero-coverage rule of the closing record, :616-636, or the pruning) of record i; false: the reference has left its loop
WV_FN bool head_step(St& S, int i, bool closing, int oChr, int oRight) {
    const Tab& X = *S.X;
    if (S.ds == X.nd) return false;
    const int rid = S.R[i].refid, rpos = S.R[i].pos;
    S.co = next_of(S, W_C, S.co, S.wend); S.po = next_of(S, W_P, S.po, S.wend);
    while (S.ds != X.nd && !(S.flags & F_CAPACITY) && (dref(S, S.ds) < rid || (dref(S, S.ds) == rid && S.nextdisright < rpos))) process_cluster(S, rid, rpos);
    if (S.flags & F_CAPACITY) return false;
    if (!closing) { prune_all(S, rid); return true; }
    const bool disLead = S.disChr > oChr || (S.disChr == oChr && S.disright > oRight);
    const int curRight = disLead ? S.disright : oRight, curChr = imax(S.disChr, oChr);
    // (the closing record of a stretch is a zero-coverage record by the scan that made the stretches; the test is repeated as the host does)
    const int dn_ref = dref(S, S.ds), dn_pos = dpos(S, S.ds);
    const bool zerocov = (rid != curChr || rpos > curRight + X.RL) && (curChr < dn_ref || (curChr == dn_ref && curRight + X.RL < dn_pos));
    if (!zerocov) { prune_all(S, rid); return true; }
    if (S.markStart != -1) {  // :621-630
        const bool on = curChr == S.markChr && curRight > S.markStart;
        if (on && curRight - S.markStart < NEAR) {
            if (S.nown > 0) { if (S.markStart == back_end(S)) { extend(S, curRight - S.markStart); ++S.ext2; } }
            else {  // compared with the end of the node in front WITHOUT a chromosome test: kept as a value
                if (S.nsens < SENS_CAP) { if (wv::lane() == 0) S.row[R_SENS + S.nsens] = S.markStart; } else S.flags |= F_SENS_FULL;
                ++S.nsens;
            }
        } else if (on && curRight - S.markStart >= NEAR) emit(S, S.markChr, S.markStart, curRight - S.markStart);
        S.markStart = -1; S.markChr = -1;
    }
    S.co = S.wend; S.po = S.wend;
    return true;
}
// one wave: active stretch a
WV_FN void run_stretch(const Tab& X, wv::lds_u32* M, int32_t* nodes, int32_t* report, int a) {
    const int32_t* sr = X.stretch + STRETCH * a;
    const int lo = sr[S_LO], hi = sr[S_HI];
    St S;
    S.X = &X; S.R = X.recs - sr[S_SHIFT]; S.M = M;
    S.nodes = nodes + 3 * (int64_t)sr[S_NODE_OFF]; S.node_cap = sr[S_NODE_CAP]; S.row = report + REPORT * (int64_t)a;
    S.kc = -1; S.ds = S.de = S.dcur = 0; S.ps = S.pe = 0;
    S.disChr = S.nextdisChr = S.disright = S.nextdisright = 0; S.markStart = -1; S.markChr = -1;
    S.nown = 0; S.bchr = -1; S.bpos = 0; S.blen = 0;
    S.flags = 0; S.minchr = INT32_MAX; S.bound = INT32_MAX; S.nsens = 0; S.ext0 = S.ext1 = S.ext2 = 0; S.nclusters = 0; S.nsubs = 0; S.mmax = 0;
    // the clusters consumed in front of the stretch leave nothing but the cluster at hand and the right end of the one before it
    const int fc = sr[S_KC];
    if (fc > 0) { S.nextdisChr = X.cl4[4 * (fc - 1) + 2]; S.nextdisright = X.cl4[4 * (fc - 1) + 3]; }
    S.kc = fc - 1;
    new_cluster(S);
    const int wbeg = lo >= 0 ? lo : 0;
    S.wend = lo >= 0 ? lo + 1 : 0;  // (the push step of the stretch's first record)
    S.co = S.po = wbeg;
    bool alive = true;
    int i = lo + 1;
    while (i < hi && alive) {
        if (S.ds == X.nd) { alive = false; break; }
        const int t = S.kc < X.ncl ? imin(X.trigger[S.kc], hi) : hi;
        if (i < t) {  // records in front of the next trigger only join a window; the pruning the trigger record finds is that of the last of them
            S.wend = t - 1;
            S.co = next_of(S, W_C, S.co, S.wend); S.po = next_of(S, W_P, S.po, S.wend);
            prune_all(S, S.R[t - 1].refid);
            S.wend = t;
            i = t;
        }
        if (i >= hi) break;
        alive = head_step(S, i, false, 0, 0);
        if (alive) { S.wend = i + 1; ++i; }
    }
    if (alive && hi < X.K_eff) head_step(S, hi, true, sr[S_OCHR], sr[S_ORIGHT]);
    if (wv::lane() == 0) {
        int32_t* o = S.row;
        o[R_FLAGS] = S.flags; o[R_NODES] = S.nown; o[R_MINCHR] = S.minchr; o[R_BOUND] = S.bound; o[R_NSENS] = S.nsens;
        o[R_EXT] = S.ext0; o[R_EXT + 1] = S.ext1; o[R_EXT + 2] = S.ext2; o[R_CLUSTERS] = S.nclusters; o[R_SUBS] = S.nsubs; o[R_MMAX] = S.mmax; o[R_SPARE] = 0;
    }
}
}  // namespace sgs
