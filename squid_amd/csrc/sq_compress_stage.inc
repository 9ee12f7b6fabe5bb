// FurtherCompressNode's walk cut at independent windows (sq_compress_windows_on_device): the kernels that decide where a wave of
// k_further_compress (sq_graph_kernels.inc) may start from the state of a chromosome start, the window table, and the id offsets behind the
// walk.  Bodies only, written against sq_wave.h, so that tools/fc_windows_emu.cpp runs this source on the CPU (SQ_WAVE_EMU); the __global__
// wrappers and the host side (dev_further_compress) are in sq_graph_kernels.inc.  DESIGN.md section 3 has the rule and why it is sound.
//
// Inputs: chr[] of the node list and what k_fc_summary wrote: hasdisc[v] (v has a discordant edge), maxfar[v] (the largest node index v's
// concordant edges touch, -1: none).  For a node i > 0 on the chromosome of i - 1:
//   p(i)    the last v < i on this chromosome with hasdisc[v]              (none: the chromosome has no such node in front of i)
//   q(i)    the first v >= i on this chromosome with hasdisc[v]            (only asked for q - p < 20, so it lies at most 18 nodes ahead)
//   run(i)  max maxfar[k] over p(i) < k < i, from the chromosome's first node when there is no p(i); -1: no such k
//   i starts a window  <=>  run(i) < i  and not  (p and q exist and q - p < 20)
// Node 0 and every node whose chr differs from its predecessor's start a window whatever the rest says.
//
//   tile_state / tile_prefix / tile_flags   p and run are one scan: every node is an element (tag, rm) -- tag != 0: the element resets what
//                                           is in front of it (1: a chromosome start without a discordant edge, v + 2: the discordant node v,
//                                           whose own concordant edges are dropped with everything before), rm: the reach it leaves -- under
//                                           combine(a, b) = b.tag ? b : (a.tag, max(a.rm, b.rm)), which is associative and not commutative.
//                                           Tile-local (DESIGN.md section 3): one wave reduces each tile of TILE nodes, one wave scans the
//                                           tiles' states, one wave per tile applies them.  q is read from the ballots of hasdisc and of the
//                                           chromosome starts over the 64 nodes of a round and the 64 behind them.
//   scatter                                 behind the inclusive sum of the flags (winc[i]; window_of[i] = winc[i] - 1): win[window_of[i]] = i
//                                           at every flagged i, win[nwin] = n
//   window_ids / add_offsets                a window's wave counted its ids from 0 and they never decrease: it used merge[last node] + 1 of
//                                           them; behind the exclusive sum of that over the windows (off[]) every node adds off[window_of[i]]
#pragma once
#include "sq_wave.h"
namespace fcw {
constexpr int TILE_ROUNDS = 16, TILE = 64 * TILE_ROUNDS;  // nodes per wave
constexpr int REACH = 20;                                 // the literal `i + 20` of SegmentGraph.cpp:2750 (not Concord_Dist_Idx)
struct In { int32_t n; const int32_t *chr, *hasdisc, *maxfar; };
struct El { int32_t tag, rm; };
WV_FN El combine(El a, El b) { return b.tag ? b : El{a.tag, a.rm > b.rm ? a.rm : b.rm}; }
WV_FN bool chr_start(const In& G, int64_t v) { return v == 0 || G.chr[v] != G.chr[v - 1]; }
WV_FN El element(const In& G, int64_t v) {
    if (v >= G.n) return El{0, -1};
    if (G.hasdisc[v]) return El{(int32_t)v + 2, -1};
    return El{chr_start(G, v) ? 1 : 0, G.maxfar[v]};
}
WV_FN El shfl_el(El e, int src) { return El{(int32_t)wv::shfl((uint32_t)e.tag, src), (int32_t)wv::shfl((uint32_t)e.rm, src)}; }
WV_FN El scan_incl(El e) {
    for (int d = 1; d < 64; d <<= 1) { const El o = shfl_el(e, wv::lane() - d); if (wv::lane() >= d) e = combine(o, e); }
    return e;
}
// pass 1, one wave per tile: state[2 t], state[2 t + 1] = the tile's elements combined
WV_FN void tile_state(const In& G, int64_t tile, int32_t* state) {
    El run{0, -1};
    for (int it = 0; it < TILE_ROUNDS && tile * TILE + it * 64 < G.n; ++it) run = combine(run, shfl_el(scan_incl(element(G, tile * TILE + it * 64 + wv::lane())), 63));
    if (wv::lane() == 0) { state[2 * tile] = run.tag; state[2 * tile + 1] = run.rm; }
}
// pass 2, one wave: front[2 t], front[2 t + 1] = the tiles in front of tile t combined
WV_FN void tile_prefix(int64_t ntiles, const int32_t* state, int32_t* front) {
    El run{0, -1};
    for (int64_t base = 0; base < ntiles; base += 64) {
        const int64_t t = base + wv::lane();
        const El s = scan_incl(t < ntiles ? El{state[2 * t], state[2 * t + 1]} : El{0, -1});
        const El before = shfl_el(s, wv::lane() - 1);
        const El x = wv::lane() ? combine(run, before) : run;
        if (t < ntiles) { front[2 * t] = x.tag; front[2 * t + 1] = x.rm; }
        run = combine(run, shfl_el(s, 63));
    }
}
// the 64 bits of `cur` from this lane on, then those of `nx`
WV_FN unsigned long long ahead(unsigned long long cur, unsigned long long nx) { const int l = wv::lane(); return l ? (cur >> l) | (nx << (64 - l)) : cur; }
// pass 3, one wave per tile: flag[i] = 1 where a window starts
WV_FN void tile_flags(const In& G, int64_t tile, const int32_t* front, int32_t* flag) {
    El run{front[2 * tile], front[2 * tile + 1]};
    for (int it = 0; it < TILE_ROUNDS && tile * TILE + it * 64 < G.n; ++it) {  // (the last tile stops behind the last node)
        const int64_t v = tile * TILE + it * 64 + wv::lane(), w = v + 64;
        const bool cs = v < G.n && chr_start(G, v);
        const unsigned long long hd0 = wv::ballot(v < G.n && G.hasdisc[v] != 0), hd1 = wv::ballot(w < G.n && G.hasdisc[w] != 0);
        const unsigned long long cs0 = wv::ballot(cs), cs1 = wv::ballot(w < G.n && chr_start(G, w));
        const El s = scan_incl(element(G, v));
        const El before = shfl_el(s, wv::lane() - 1);
        const El x = wv::lane() ? combine(run, before) : run;  // what the nodes in front of v leave: x.tag - 2 = p(v), x.rm = run(v)
        const int d = wv::ctz64(ahead(hd0, hd1));                 // q(v) = v + d
        const int c = wv::ctz64(ahead(cs0, cs1) & ~1ull);         // the next chromosome starts at v + c
        const bool near = x.tag >= 2 && d < REACH - 1 && d < c && v + d - (x.tag - 2) < REACH;
        if (v < G.n) flag[v] = (cs || (x.rm < v && !near)) ? 1 : 0;
        run = combine(run, shfl_el(s, 63));
    }
}
// lane-local
WV_FN void scatter(int32_t n, const int32_t* flag, const int32_t* winc, int32_t* win, int64_t i) {
    if (i >= n) return;
    if (flag[i]) win[winc[i] - 1] = (int32_t)i;
    if (i == n - 1) win[winc[i]] = n;
}
WV_FN int32_t window_ids(const int32_t* win, const int32_t* merge, int64_t w) { return merge[win[w + 1] - 1] + 1; }
WV_FN void add_offsets(int32_t n, const int32_t* winc, const int32_t* off, int32_t* merge, int64_t i) {
    if (i < n) merge[i] += off[winc[i] - 1];
}
}  // namespace fcw
