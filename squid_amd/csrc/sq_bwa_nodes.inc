// `squid --bwa` on the device (sq_bwa_nodes_on_device): the stream loop of BuildNode_BWA (SegmentGraph.cpp:855-1114; seed_step /
// bwa_seed_nodes of sq_bwa.cpp) as kernels over the resident record table.  Written in the operations of sq_wave.h, so that
// tools/bwa_nodes_emu.cpp runs this source on the CPU (SQ_WAVE_EMU) against the host automaton in one go; the __global__ wrappers, the
// compacting scans (device_scan) and the host entry point dev_bwa_seed_nodes are in sq_kernels.hip.
//
// The loop is one automaton over all records, but what it carries dies at a gap in the coverage (the comment above SeedRun in
// sq_bwa.cpp): the stream is cut at EVERY gap record -- a passing record on another chromosome than the running maximum of
// (RefID, end of first block) over the passing records in front of it, or more than RL_final + 64 behind that maximum; never inside the
// first eight records, never before the first passing record -- and one wave runs each stretch from the state a fresh automaton has plus
// the host's guesses (zero coverage at the gap record, other_right 0, dis_right by the rule of its own), ends with the closing turn on the
// next stretch's gap record and reports what SeedRun reports.  The host walks the reports in order and runs a stretch whose guess was
// wrong where it counted again, with seed_step.
//
//   class_record    lane-local: class byte, start and end of the first block
//   tile_max / tile_prefix / tile_cut    tile-local exclusive prefix maxima (DESIGN.md section 3) of the two keys: cut bit, sortedness
//   scatter         lane-local behind three exclusive scans (cut bit, discordant, clipped concordant): cut list, discordant list
//   dis_summary / dis_carry    the dis_right every stretch is started with
//   run_stretch     one wave per stretch: the automaton
//   gather_seeds    lane-local behind an exclusive scan of the seed counts: the seeds in stretch order
//
// The three windows are not storage: a window is the range [head, current record) of the stream filtered by class (the discordant one:
// a range of the discordant list), plus the last four pushed indices for vote_chr.  The capacity-driven compaction (W1) is not modelled:
// unobservable, by the argument the host stretches already rely on.  Control flow is wave-uniform: every value that decides a branch is
// the same in all lanes (loads from uniform addresses, ballots, reductions); the lanes share the loops over windows inside a flush.
// Identities beyond seed_step are checked, not assumed: the passing records sorted by (RefID, pos) -- FLAG_UNSORTED, the caller takes the
// host route.
#pragma once
#include "sq_wave.h"
#include "sq_stage_layout.h"
namespace bwn {
using sq::RecCols;
WV_FN int imax(int a, int b) { return a > b ? a : b; }
WV_FN int imin(int a, int b) { return a < b ? a : b; }

// ---- lane-local: the class byte and the first block of record r
WV_FN void class_record(const RecCols& R, uint8_t* cls, int32_t* p0, int32_t* e0, int64_t r) {
    if (r >= R.n) return;
    cls[r] = 0; p0[r] = 0; e0[r] = 0;
    const int flag = R.flag[r], rid = R.refid[r];
    if ((R.aux[r] & SQ_AUX_MULTI) || R.mapq[r] == 0 || (flag & 0x400) || (flag & 0x4) || rid == -1) return;
    uint8_t cl = N_PASS1;
    const uint32_t b0 = R.blk_off[r], nb = R.blk_off[r + 1] - b0;
    if (nb != 0) {
        cl |= N_PASS;
        const int p = R.pos[r], mp = R.mpos[r], mrid = R.mrefid[r];
        const bool rev = (flag & 0x10) != 0, mrev = (flag & 0x20) != 0;
        bool conc = !(flag & 0x8) && mrid != -1 && rid == mrid && (flag & 0x2);  // pair_concordant (:1037-1040)
        if (conc) {
            if (rev && !mrev) conc = p >= mp && p - mp <= 750000;
            else if (!rev && mrev) conc = mp >= p && mp - p <= 750000;
            else conc = false;
        }
        const int rp0 = R.b_readpos[b0], bl = (int)(b0 + nb - 1);
        if (!conc) cl |= N_DISC;
        else if (!(R.aux[r] & SQ_AUX_LOWPHRED) && (rp0 > 15 || (int)R.totlen[r] - (int)R.b_readpos[bl] - (int)R.b_matchread[bl] > 15)) cl |= N_CLIP;
        if (rev) cl |= N_REV;
        if (rp0 > 15) cl |= N_RP15;
        p0[r] = R.b_refpos[b0]; e0[r] = R.b_refpos[b0] + R.b_matchref[b0];
    }
    cls[r] = cl;
}

// ---- the two keys and their exclusive prefix maxima: end key (RefID, end of first block) of the PASS records, start key (RefID, pos) of
// the PASS1 records; -1: none
struct Keys { int64_t n; const int32_t *refid, *pos, *e0; };
WV_FN long long end_key(const Keys& K, const uint8_t* cls, int64_t r) { return (r < K.n && (cls[r] & N_PASS)) ? (long long)(((unsigned long long)(uint32_t)K.refid[r] << 32) | (uint32_t)K.e0[r]) : -1ll; }
WV_FN long long start_key(const Keys& K, const uint8_t* cls, int64_t r) { return (r < K.n && (cls[r] & N_PASS1)) ? (long long)(((unsigned long long)(uint32_t)K.refid[r] << 32) | (uint32_t)K.pos[r]) : -1ll; }
WV_FN long long shfl64(long long v, int src) {
    const uint32_t lo = wv::shfl((uint32_t)(unsigned long long)v, src), hi = wv::shfl((uint32_t)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
WV_FN long long scan_incl_max64(long long v) {
    for (int d = 1; d < 64; d <<= 1) { const long long o = shfl64(v, wv::lane() - d); if (wv::lane() >= d && o > v) v = o; }
    return v;
}
WV_FN long long max64(long long a, long long b) { return a > b ? a : b; }
// pass 1, one wave per tile: tmax[2 t] = largest end key, tmax[2 t + 1] = largest start key
WV_FN void tile_max(const Keys& K, const uint8_t* cls, int64_t tile, long long* tmax) {
    long long e = -1, s = -1;
    for (int it = 0; it < TILE_ROUNDS; ++it) { const int64_t r = tile * TILE_RECS + it * 64 + wv::lane(); e = max64(e, end_key(K, cls, r)); s = max64(s, start_key(K, cls, r)); }
    e = shfl64(scan_incl_max64(e), 63); s = shfl64(scan_incl_max64(s), 63);
    if (wv::lane() == 0) { tmax[2 * tile] = e; tmax[2 * tile + 1] = s; }
}
// pass 2, one wave: front[2 t], front[2 t + 1] = the two maxima over the tiles in front of tile t
WV_FN void tile_prefix(int64_t ntiles, const long long* tmax, long long* front) {
    long long run_e = -1, run_s = -1;
    for (int64_t base = 0; base < ntiles; base += 64) {
        const int64_t t = base + wv::lane();
        const long long se = scan_incl_max64(t < ntiles ? tmax[2 * t] : -1ll), ss = scan_incl_max64(t < ntiles ? tmax[2 * t + 1] : -1ll);
        const long long pe = shfl64(se, wv::lane() - 1), ps = shfl64(ss, wv::lane() - 1);
        if (t < ntiles) { front[2 * t] = max64(run_e, wv::lane() ? pe : -1ll); front[2 * t + 1] = max64(run_s, wv::lane() ? ps : -1ll); }
        run_e = max64(run_e, shfl64(se, 63)); run_s = max64(run_s, shfl64(ss, 63));
    }
}
// pass 3, one wave per tile: the cut bit of every record, FLAG_UNSORTED
WV_FN void tile_cut(const Keys& K, uint8_t* cls, int64_t tile, const long long* front, int rl_final, uint32_t* flags) {
    long long run_e = front[2 * tile], run_s = front[2 * tile + 1];
    bool unsorted = false;
    for (int it = 0; it < TILE_ROUNDS; ++it) {
        const int64_t r = tile * TILE_RECS + it * 64 + wv::lane();
        const long long ek = end_key(K, cls, r), sk = start_key(K, cls, r);
        const long long se = scan_incl_max64(ek), ss = scan_incl_max64(sk);
        const long long pe = shfl64(se, wv::lane() - 1), ps = shfl64(ss, wv::lane() - 1);
        const long long xe = max64(run_e, wv::lane() ? pe : -1ll), xs = max64(run_s, wv::lane() ? ps : -1ll);
        if (r < K.n) {
            if (sk >= 0 && sk < xs) unsorted = true;
            if (ek >= 0 && r >= 8 && xe >= 0) {
                const int chr = (int)(xe >> 32), end = (int)(uint32_t)(unsigned long long)xe;
                if (K.refid[r] != chr || (long long)K.pos[r] > (long long)end + rl_final + 64) cls[r] = (uint8_t)(cls[r] | N_CUT);
            }
        }
        run_e = max64(run_e, shfl64(se, 63)); run_s = max64(run_s, shfl64(ss, 63));
    }
    if (wv::any(unsorted) && wv::lane() == 0) wv::glb_atomic_or(flags, FLAG_UNSORTED);
}
// lane-local behind the exclusive scans of the cut bit (at_cut), the discordant passing records (drank) and the clipped concordant ones:
// cut[0] = 0, cut[1 + at_cut[r]] = r, cut[np] = n; dlist[drank[r]] = r
WV_FN void scatter(int64_t n, const uint8_t* cls, const int32_t* at_cut, const int32_t* drank, int32_t n_cut, int32_t* cut, uint32_t* dlist, int64_t r) {
    if (r >= n) return;
    if (r == 0) { cut[0] = 0; cut[n_cut + 1] = (int32_t)n; }
    const uint8_t cl = cls[r];
    if (cl & N_CUT) cut[1 + at_cut[r]] = (int32_t)r;
    if ((cl & W_MASK) == W_DIS) dlist[drank[r]] = (uint32_t)r;
}

// ---- the tables the automaton reads
struct Tab {
    int64_t n;
    const int32_t *refid, *pos;
    const uint16_t* totlen;
    const uint8_t* cls;
    const int32_t *p0, *e0;
    const uint32_t* dlist;
    const int32_t *drank, *crank;  // n + 1 entries each
};
// read_len: the chimeric file's value; rl5[i]: ReadLen behind record i of the first five (:857-864); rl_final = rl5[4]
struct Par { int32_t read_len, rl_final, rl5[5]; };
WV_FN int rl_at(const Par& P, int k, int64_t ri) { return k == 0 ? (ri < 5 ? P.rl5[ri] : P.rl_final) : P.rl_final; }

// DiscordantRightmost as a fresh stretch leaves it (the rule of bwa_seed_nodes; the records are sorted -- checked --, so whether the window
// was emptied in front of a discordant record shows at that record itself): lane-local, one lane per stretch
WV_FN void dis_summary(const Tab& T, const Par& P, const int32_t* cut, int32_t np, int32_t* has, int32_t* dr_out, int64_t k) {
    if (k >= np) return;
    const int lo = cut[k], hi = cut[k + 1];
    bool nonempty = false;
    int dr = 0, last = -1;
    for (int i = T.drank[lo]; i < T.drank[hi]; ++i) {
        const int r = (int)T.dlist[i], rid = T.refid[r];
        if (nonempty && (last != rid || dr + rl_at(P, (int)k, r) < T.pos[r])) nonempty = false;
        dr = nonempty ? imax(dr, T.e0[r]) : T.e0[r];
        nonempty = true; last = rid;
    }
    has[k] = nonempty ? 1 : 0; dr_out[k] = dr;
}
// one wave: dis_in[k] = the value of the last stretch in front of k that has a discordant record (0: none)
WV_FN void dis_carry(int32_t np, const int32_t* has, const int32_t* dr, int32_t* dis_in) {
    int run = -1;  // index of that stretch
    for (int base = 0; base < np; base += 64) {
        const int k = base + wv::lane();
        const int mine = (k < np && has[k]) ? k : -1;
        const int s = wv::scan_incl_max(mine);
        const int x = imax(run, (int)wv::shfl_up1((uint32_t)s, (uint32_t)-1));
        if (k < np) dis_in[k] = x >= 0 ? dr[x] : 0;
        run = imax(run, (int)wv::bcast((uint32_t)s, 63));
    }
}

// ---- the automaton
struct Win { int head, cnt, l0, l1, l2, l3; };
WV_FN int wave_max(int v) { for (int d = 1; d < 64; d <<= 1) v = imax(v, (int)wv::shfl((uint32_t)v, wv::lane() ^ d)); return v; }
WV_FN int wave_min(int v) { for (int d = 1; d < 64; d <<= 1) v = imin(v, (int)wv::shfl((uint32_t)v, wv::lane() ^ d)); return v; }
// the first record of class `want` in [from, end) (end: none)
WV_FN int next_of(const Tab& T, uint8_t want, int from, int end) {
    int q = from;
    for (; q < end && q < from + 4; ++q) if ((T.cls[q] & W_MASK) == want) return q;
    for (int base = q; base < end; base += 64) {
        const int j = base + wv::lane();
        const unsigned long long m = wv::ballot(j < end && (T.cls[j] & W_MASK) == want);
        if (m) return base + wv::ctz64(m);
    }
    return end;
}
WV_FN void win_push(Win& w, int ri) { if (w.cnt == 0) w.head = ri; ++w.cnt; w.l3 = w.l2; w.l2 = w.l1; w.l1 = w.l0; w.l0 = ri; }
WV_FN void drop_left_of(const Tab& T, Win& w, uint8_t want, int rid, int p, int RL, int cur) {
    while (w.cnt > 0 && (T.refid[w.head] != rid || T.e0[w.head] + RL < p)) { --w.cnt; if (w.cnt > 0) w.head = next_of(T, want, w.head + 1, cur); }
}
WV_FN void vote_chr(const Tab& T, const Win& w, int& chr) {
    if (w.cnt <= 0) return;
    const int idx = w.cnt == 1 ? w.l0 : w.cnt == 2 ? w.l1 : w.cnt == 3 ? w.l2 : w.l3;
    chr = T.refid[idx];
}
struct State {
    int RL, prev0, mark_start, mark_chr, dis_right, other_right, bits, minpos_dis, minpos_oth, nreads;
    int nseeds, schr, spos, slen;  // the seeds of the stretch: how many, and the last one
    int flush_nodes, flushes, cover_fails, marks_closed;
    Win conc, part;
    int d0, doff, dend;  // the discordant window: [d0, dend) of the discordant list is its storage, [doff, dend) the window
    int32_t* seeds; int seed_cap;
    int32_t* margins; int margin_cap;
    uint32_t* flags;
    bool dead;  // a bound was hit: the flags say which, nothing of the stretch is valid
};
WV_FN void emit(State& S, int chr, int pos, int len) {
    if (S.nseeds < S.seed_cap) { if (wv::lane() == 0) { S.seeds[3 * S.nseeds] = chr; S.seeds[3 * S.nseeds + 1] = pos; S.seeds[3 * S.nseeds + 2] = len; } }
    else if (wv::lane() == 0) wv::glb_atomic_or(S.flags, FLAG_SEEDS_FULL);
    ++S.nseeds; S.schr = chr; S.spos = pos; S.slen = len;
}
WV_FN void push_node(State& S, int chr, int from, int to, int& cur_start, int& cur_end, int& emitted) {
    emit(S, chr, from, to - from);
    cur_start = to; cur_end = to; S.mark_start = to; S.mark_chr = chr; ++emitted;
}
// FP64 with one rounding per operation, as on the host (-ffp-contract=off; the division is the IEEE one: no fast-math flag on this file)
WV_FN bool dense(int d_start, int d_end, int d_count, bool split, int RL) {
    if (d_start == -1 || split) return false;
    const double v = 4.0 * (double)(d_end - d_start) / (double)RL;
    const double m = v < 5.0 ? v : 5.0;  // std::min(5.0, v)
    return (double)d_count > m;
}
// the discordant window is complete: the segment boundaries inside it (:888-998); (rid, p): the record in front of which it is flushed
WV_FN void flush(const Tab& T, State& S, int rid, int p, int ri) {
    const int L = wv::lane(), RL = S.RL;
    int cur_end = 0, cur_start = imax(S.prev0, S.mark_start);
    int d_start = -1, d_end = -1, d_count = -1, emitted = 0;
    bool split = false;
    const int chr0 = T.refid[T.dlist[S.d0]];  // (W2: element 0 of the storage)
    const long guard_max = 2l * S.margin_cap + (S.dend - S.d0) + 8;
    long guard = 0;
    while (S.doff < S.dend) {
        if (++guard > guard_max) { if (L == 0) wv::glb_atomic_or(S.flags, FLAG_GUARD); S.dead = true; return; }
        const int hchr = T.refid[T.dlist[S.doff]];
        if (dense(d_start, d_end, d_count, split, RL)) push_node(S, hchr, d_start, d_end, cur_start, cur_end, emitted);
        split = false;
        // the leading run of blocks that touch each other
        int ibreak = -1, nm = 0;
        for (int base = S.doff; base < S.dend; base += 64) {
            const int i = base + L;
            const bool valid = i < S.dend;
            const int r = valid ? (int)T.dlist[i] : 0, pp = T.p0[r], ee = T.e0[r];
            const bool brk = valid && i + 1 < S.dend && T.p0[T.dlist[i + 1]] > ee;
            const unsigned long long bm = wv::ballot(brk);
            const int nin = bm ? wv::ctz64(bm) + 1 : imin(64, S.dend - base);
            if (L < nin) { const int o = 2 * (i - S.doff); if (o + 1 < S.margin_cap) { S.margins[o] = pp; S.margins[o + 1] = ee; } }
            cur_end = imax(cur_end, wave_max(L < nin ? ee : INT32_MIN));
            nm += 2 * nin;
            if (bm) { ibreak = base + wv::ctz64(bm); break; }
        }
        const int i_after = ibreak >= 0 ? ibreak : S.dend;
        d_count = i_after - S.doff;
        const int m0 = T.p0[T.dlist[S.doff]];
        d_start = imax(cur_start, m0); d_end = cur_end;
        for (int base = i_after + 1; base < S.dend; base += 64) {  // the blocks that start within `thresh` behind the run
            const int i = base + L;
            const bool valid = i < S.dend;
            const int r = valid ? (int)T.dlist[i] : 0, pp = T.p0[r], ee = T.e0[r];
            const unsigned long long stop = wv::ballot(valid && !(pp < cur_end + THRESH));
            const int nin = stop ? wv::ctz64(stop) : imin(64, S.dend - base);
            if (L < nin) { const int o = nm + 2 * L; if (o + 1 < S.margin_cap) { S.margins[o] = pp; S.margins[o + 1] = ee; } }
            nm += 2 * nin;
            if (stop) break;
        }
        if (S.part.cnt > 0)  // clip positions of the partially aligned reads next to the run
            for (int base = S.part.head; base < ri; base += 64) {
                const int q = base + L;
                const uint8_t cl = q < ri ? T.cls[q] : 0;
                const bool is = q < ri && (cl & W_MASK) == W_PART && T.refid[q] == hchr;
                const int pr = is ? T.p0[q] : 0, pe = is ? T.e0[q] : 0;
                const bool rev = (cl & N_REV) != 0;
                const bool a = is && (cl & N_RP15) && pr > m0 - THRESH && pr < cur_end + THRESH;
                const bool b = is && !a && pe > m0 - THRESH && pe < cur_end + THRESH;
                const unsigned long long wm = wv::ballot(a || b);
                const int o = nm + wv::popc64(wm & wv::lanemask_lt());
                if ((a || b) && o < S.margin_cap) S.margins[o] = a ? (rev ? pe : pr) : (rev ? pr : pe);
                nm += wv::popc64(wm);
            }
        if (nm > S.margin_cap) { if (L == 0) wv::glb_atomic_or(S.flags, FLAG_MARGINS_FULL); S.dead = true; return; }
        wv::sync();
        // the distinct positions in ascending order (the host sorts the list and steps from value to value; the smallest value above the last
        // one is the same walk)
        int last_cursor = -1, last_support = 0;
        long long x_prev = -(1ll << 40);
        for (;;) {
            int mn = INT32_MAX;
            bool found = false;
            for (int base = 0; base < nm; base += 64) { const int i = base + L; if (i < nm) { const int v = S.margins[i]; if ((long long)v > x_prev) { found = true; mn = imin(mn, v); } } }
            if (!wv::any(found)) break;
            const int x = wave_min(mn);
            x_prev = x;
            if (S.nseeds > 0 && S.schr == chr0 && x - S.spos - S.slen < THRESH * 20) continue;
            int sr = 0, left_fwd = 0, right_rev = 0;
            for (int base = 0; base < nm; base += 64) { const int i = base + L; const int v = i < nm ? S.margins[i] : 0; sr += wv::popc64(wv::ballot(i < nm && v > x - THRESH && v < x + THRESH)); }
            for (int base = S.doff; base < S.dend; base += 64) {
                const int i = base + L;
                const bool valid = i < S.dend;
                const int r = valid ? (int)T.dlist[i] : 0, pp = T.p0[r], ee = T.e0[r];
                const bool rev = (T.cls[r] & N_REV) != 0;
                const bool a = valid && ee < x && ee > x - RL && !rev;
                const bool b = valid && !a && pp > x && pp < x + RL && rev;
                left_fwd += wv::popc64(wv::ballot(a)); right_rev += wv::popc64(wv::ballot(b));
            }
            bool cut_here = false;
            if (sr > 3 || sr + left_fwd > 4 || sr + right_rev > 4) {
                int cover = 0;
                if (S.conc.cnt > 0)
                    for (int base = S.conc.head; base < ri; base += 64) {
                        const int q = base + L;
                        const bool is = q < ri && (T.cls[q] & W_MASK) == W_CONC;
                        cover += wv::popc64(wv::ballot(is && T.e0[is ? q : 0] >= x + THRESH && T.p0[is ? q : 0] < x - THRESH));
                    }
                if (!(sr > imax(cover - sr, 0) + 2)) ++S.cover_fails;
                if (sr > imax(cover - sr, 0) + 2) {
                    const int strength = sr + imax(left_fwd, right_rev);
                    if (last_cursor == -1 && x - cur_start < THRESH * 20) { S.mark_start = cur_start; S.mark_chr = chr0; }
                    else if ((last_cursor == -1 || x - last_cursor < THRESH * 20) && strength > last_support) { last_cursor = x; last_support = strength; }
                    else if (x - last_cursor >= THRESH * 20) { split = true; push_node(S, chr0, cur_start, last_cursor, cur_start, cur_end, emitted); cut_here = true; }
                }
            }
            if (cut_here) break;
        }
        if (last_cursor != -1 && !split) { split = true; push_node(S, hchr, cur_start, last_cursor, cur_start, cur_end, emitted); }
        wv::sync();  // (the margins are read by all lanes before the next round writes them)
        while (S.doff < S.dend) {  // the blocks that end inside what is decided
            const int i = S.doff + L;
            const bool valid = i < S.dend;
            const unsigned long long stop = wv::ballot(valid && !(T.e0[T.dlist[valid ? i : S.doff]] <= cur_end));
            if (stop) { S.doff += wv::ctz64(stop); break; }
            S.doff = imin(S.doff + 64, S.dend);
        }
    }
    if (dense(d_start, d_end, d_count, split, RL)) push_node(S, chr0, d_start, d_end, cur_start, cur_end, emitted);  // (W2)
    S.d0 = S.doff = S.dend;
    ++S.flushes;
    if (emitted) ++S.flush_nodes;
    drop_left_of(T, S.conc, W_CONC, rid, p, RL, ri); drop_left_of(T, S.part, W_PART, rid, p, RL, ri);
}
// one turn of the loop for record ri (seed_step); closing: the record only closes the stretch in front of it; opening: it is the gap
// record of this stretch, whose turn up to the zero-coverage rule was the closing turn of the stretch in front (guess: zero coverage)
WV_FN void step(const Tab& T, const Par& P, State& S, int ri, bool closing, bool opening) {
    if (ri < 5 && !closing) S.RL = imax(S.RL, (int)T.totlen[ri]);  // (:857-864: in front of the filter; a stretch behind the first never sees ri < 8)
    const uint8_t cl = T.cls[ri];
    if (!(cl & N_PASS1)) return;
    const int rid = T.refid[ri], p = T.pos[ri];
    const bool dnone = S.doff == S.dend;
    if (!opening && ((!dnone && rid != T.refid[T.dlist[S.doff]]) || (S.conc.cnt > 0 && rid != T.refid[S.conc.head]) || (S.part.cnt > 0 && rid != T.refid[S.part.head]))) { S.other_right = 0; S.bits |= B_OTH_SET; }
    if (!(cl & N_PASS)) return;
    if (!closing) ++S.nreads;
    if (!opening && S.conc.cnt == 0 && S.part.cnt == 0 && dnone) S.prev0 = p;
    if (!opening && !dnone && (T.refid[T.dlist[S.dend - 1]] != rid || S.dis_right + S.RL < p)) { flush(T, S, rid, p, ri); if (S.dead) return; }
    // zero coverage in front of this record (:1000-1026)
    const int rightmost = imax(S.dis_right, S.other_right);
    int cur_chr = 0;
    vote_chr(T, S.conc, cur_chr); vote_chr(T, S.part, cur_chr);
    if (S.dend > S.doff) cur_chr = T.refid[T.dlist[S.dend - imin(4, S.dend - S.doff)]];
    const bool zero = opening ? true : (rid != cur_chr || p > rightmost + S.RL);
    if (!opening && zero && rid == cur_chr) {
        if (!(S.bits & B_DIS_SET)) S.minpos_dis = imin(S.minpos_dis, p);
        if (!(S.bits & B_OTH_SET)) S.minpos_oth = imin(S.minpos_oth, p);
    }
    if (closing) S.bits = zero ? (S.bits | B_CLOSING_ZERO) : (S.bits & ~B_CLOSING_ZERO);
    if (!opening && zero && S.mark_start != -1) {
        ++S.marks_closed;
        if (rightmost > S.mark_start && rightmost - S.mark_start < THRESH * 20 && S.nseeds > 0 && S.mark_start == S.spos + S.slen) {
            S.slen += rightmost - S.mark_start;
            if (S.nseeds <= S.seed_cap && wv::lane() == 0) S.seeds[3 * (S.nseeds - 1) + 2] = S.slen;
        } else if (rightmost > S.mark_start && rightmost - S.mark_start >= THRESH * 20) { emit(S, S.mark_chr, S.mark_start, rightmost - S.mark_start); }
        S.mark_start = -1; S.mark_chr = -1;
    }
    if (closing) return;
    if (zero) S.prev0 = p;
    if (S.doff == S.dend) { drop_left_of(T, S.conc, W_CONC, rid, p, S.RL, ri); drop_left_of(T, S.part, W_PART, rid, p, S.RL, ri); }
    // the record joins a window (:1035-1086)
    const int e0 = T.e0[ri];
    if (!(cl & N_DISC)) {
        S.bits |= B_OTH_SET;
        S.other_right = (S.conc.cnt > 0 || S.part.cnt > 0) ? imax(S.other_right, e0) : e0;
        win_push((cl & N_CLIP) ? S.part : S.conc, ri);
    } else {
        S.bits |= B_DIS_SET;
        S.dis_right = S.dend > S.d0 ? imax(S.dis_right, e0) : e0;
        ++S.dend;  // (the discordant list holds ri at this place)
    }
}
// one wave: stretch k = records [cut[k], cut[k + 1]), then the closing turn on record cut[k + 1].  margins / seeds: the scratch of all
// stretches; a stretch's slices start at 2 d + c and 3 (8 d + 2 c + 4 k) for d discordant and c clipped concordant records in front of it
// and hold 2 d' + c' values and 8 d' + 2 c' + 4 seeds for the d', c' of its own
WV_FN int64_t seed_slice(const Tab& T, int lo, int64_t k) { return 8ll * T.drank[lo] + 2ll * T.crank[lo] + 4ll * k; }
WV_FN void run_stretch(const Tab& T, const Par& P, const int32_t* cut, int32_t np, const int32_t* dis_in, int32_t* margins, int32_t* seeds, int32_t* report, uint32_t* flags, int64_t k) {
    const int lo = cut[k], hi = cut[k + 1];
    State S;
    S.RL = k == 0 ? P.read_len : P.rl_final;
    S.prev0 = 0; S.mark_start = -1; S.mark_chr = -1; S.dis_right = dis_in[k]; S.other_right = 0; S.bits = B_CLOSING_ZERO; S.minpos_dis = INT32_MAX; S.minpos_oth = INT32_MAX; S.nreads = 0;
    S.nseeds = 0; S.schr = 0; S.spos = 0; S.slen = 0; S.flush_nodes = 0; S.flushes = 0; S.cover_fails = 0; S.marks_closed = 0;
    S.conc = Win{0, 0, 0, 0, 0, 0}; S.part = S.conc;
    S.d0 = S.doff = S.dend = T.drank[lo];
    const int nd = T.drank[hi] - T.drank[lo], nc = T.crank[hi] - T.crank[lo];
    S.seeds = seeds + 3 * seed_slice(T, lo, k); S.seed_cap = 8 * nd + 2 * nc + 4;
    S.margins = margins + (2ll * T.drank[lo] + T.crank[lo]); S.margin_cap = 2 * nd + nc;
    S.flags = flags; S.dead = false;
    for (int ri = lo; ri < hi && !S.dead; ++ri) step(T, P, S, ri, false, k > 0 && ri == lo);
    if (k + 1 < np && !S.dead) step(T, P, S, hi, true, false);
    if (wv::lane() == 0) {
        int32_t* o = report + REPORT * k;
        o[R_RL] = S.RL; o[R_PREV0] = S.prev0; o[R_MARK_START] = S.mark_start; o[R_MARK_CHR] = S.mark_chr; o[R_DIS_RIGHT] = S.dis_right; o[R_OTHER_RIGHT] = S.other_right; o[R_BITS] = S.bits;
        o[R_MINPOS_DIS] = S.minpos_dis; o[R_MINPOS_OTH] = S.minpos_oth; o[R_READS] = S.nreads; o[R_SEEDS] = S.nseeds; o[R_FLUSH_NODES] = S.flush_nodes; o[R_FLUSHES] = S.flushes;
        o[R_COVER_FAILS] = S.cover_fails; o[R_MARKS_CLOSED] = S.marks_closed; o[R_SPARE] = (int32_t)seed_slice(T, lo, k);  // (where the stretch's seeds start, in seeds)
    }
}
// lane-local behind the exclusive scan of the seed counts (at): the seeds of stretch k, strung together in stretch order; the row then
// says where they start in `out`
WV_FN void gather_seeds(int32_t np, int32_t* report, const int32_t* at, const int32_t* seeds, int32_t* out, int64_t k) {
    if (k >= np) return;
    int32_t* row = report + REPORT * k;
    const int32_t* s = seeds + 3 * (int64_t)row[R_SPARE];
    int32_t* o = out + 3 * (int64_t)at[k];
    for (int i = 0; i < 3 * row[R_SEEDS]; ++i) o[i] = s[i];
    row[R_SPARE] = at[k];
}
}  // namespace bwn
