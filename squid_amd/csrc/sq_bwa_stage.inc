// `squid --bwa` on the device (sq_bwa_on_device): the class byte of every record of the resident table and the node depth loop of
// BuildNode_BWA (SegmentGraph.cpp:1180-1200, ledger W6) as kernels.  Everything here is either lane-local (one lane = one record) or one
// wave per tile of blocks, written in the operations of sq_wave.h, so that tools/bwa_stage_emu.cpp runs this source on the CPU
// (SQ_WAVE_EMU) against the host loops of sq_bwa.cpp; the __global__ wrappers and the host entry points (dev_bwa_*) are in sq_kernels.hip.
//
// The depth loop walks the nodes in order with a cursor into Reads (every block of every READS record, in record order, then block
// order) that never goes back: at node i a block is counted and consumed when it lies wholly inside the node, stops the node (and is
// kept) when it starts at or behind the node's end or lies on another chromosome, and is consumed and dropped otherwise.  Without the
// cursor: g(j) = the smallest node i on block j's chromosome with pos_i + len_i > refpos_j (n_nodes: none) is the first node that can
// consume block j; the cursor reaches block j only behind the blocks in front of it, so j is consumed at m(j) = max g(0..j), an
// inclusive prefix maximum in Reads order, and counted there iff it lies inside that node.  A maximum of n_nodes is a block no node
// consumes: nothing behind it is counted.  The identity needs the chromosomes of Reads in non-decreasing order (a node m(j) > g(j)
// then lies on block j's chromosome or is n_nodes); the kernels check that and raise a flag, and the caller takes the host loop.
//
// Three launches, tile-local instead of chained (DESIGN.md section 3): depth_tile_max (one wave per tile: the largest g and the largest
// chromosome of the tile), depth_prefix (one wave: what lies in front of every tile), depth_tile_apply (the tile again with its prefix:
// wave max-scan, the test, runs of equal m reduced inside the wave, one atomic add per (wave, node) for the count and one for the sum).
#pragma once
#include "sq_wave.h"
#include "sq_stage_layout.h"
namespace bws {
using sq::RecCols;
// C_READS: the record feeds Reads (:871-881, seed_record_passes).  C_P3: ExactBPConcordantSupport looks at it (:3136-3142, decide() of
// bwa_breakpoint_support); in_names (may be null: no name is in the set): one byte per record, the raw QNAME is a rebuilt fragment's
WV_FN uint8_t class_of(const RecCols& R, int min_mapqual, const uint8_t* in_names, int64_t r) {
    const int flag = R.flag[r], rid = R.refid[r], mapq = R.mapq[r];
    if ((R.aux[r] & SQ_AUX_MULTI) || (flag & 0x400) || (flag & 0x4) || rid == -1) return 0;
    uint8_t cl = 0;
    if (mapq != 0 && R.blk_off[r + 1] != R.blk_off[r]) cl |= sq::C_READS;
    if (mapq >= min_mapqual) {
        const int mp = R.mpos[r], p = R.pos[r];
        const bool same_chr_mate = !(flag & 0x8) && R.mrefid[r] == rid;
        const bool left = same_chr_mate && (mp > p || (mp == p && (flag & 0x80)));  // (at equal positions the second mate is the one dropped)
        if (!left && !(in_names && in_names[r])) cl |= sq::C_P3;
    }
    return cl;
}
// one lane per record: the class byte, and per block of the record the chromosome (-1: the record does not feed Reads)
WV_FN void classify(const RecCols& R, int min_mapqual, const uint8_t* in_names, uint8_t* cls, int32_t* blk_chr, int64_t r) {
    const uint8_t cl = class_of(R, min_mapqual, in_names, r);
    cls[r] = cl;
    if (!blk_chr) return;
    const int32_t c = (cl & sq::C_READS) ? R.refid[r] : -1;
    for (uint32_t b = R.blk_off[r], e = R.blk_off[r + 1]; b < e; ++b) blk_chr[b] = c;
}

// chr_start: n_ref + 1, first node of every chromosome; fine / fine_off: NodeView's position index (fine == null: bisection over the chromosome)
struct Nodes { int32_t n, n_ref; const int32_t *chr, *pos, *len, *chr_start, *fine, *fine_off; };
// Reads as the block arrays hold it: chr[j] < 0 = not in Reads; pack = refpos, matchref, -, - (b_pack)
struct Blocks { int64_t nb; const int32_t* chr; const uint32_t* pack; };

WV_FN int imax(int a, int b) { return a > b ? a : b; }
// the smallest node on chromosome c whose end lies behind p (n: none); the nodes of a chromosome are sorted and do not overlap
WV_FN int first_node_behind(const Nodes& N, int c, int p) {
    if (c < 0 || c >= N.n_ref) return N.n;
    const int end = N.chr_start[c + 1];
    int lo, hi;
    if (N.fine) {
        const int first = N.fine_off[c], last = N.fine_off[c + 1] - 2;
        int b = first + (p < 0 ? 0 : (p >> sq::NODE_FINE_SHIFT));
        if (b > last) b = last;
        lo = N.fine[b]; hi = N.fine[b + 1];
    } else {
        lo = N.chr_start[c]; hi = end - 1;
        if (hi < lo) return N.n;
    }
    while (hi > lo) {  // last node with pos <= p (the chromosome's first when there is none)
        const int mid = (lo + hi + 1) >> 1;
        if (N.pos[mid] <= p) lo = mid; else hi = mid - 1;
    }
    if (N.pos[lo] + N.len[lo] > p) return lo;
    return lo + 1 < end ? lo + 1 : N.n;
}
WV_FN int wave_max(int v) {
    for (int d = 1; d < 64; d <<= 1) v = imax(v, (int)wv::shfl((uint32_t)v, wv::lane() ^ d));
    return v;
}
struct Lane { bool in; int c, p, len, g; };
WV_FN Lane load_lane(const Nodes& N, const Blocks& B, int64_t j) {
    Lane l;
    l.in = false; l.c = -1; l.p = 0; l.len = 0; l.g = -1;
    if (j < B.nb) {
        l.c = B.chr[j];
        if (l.c >= 0) {
            const wv::u32x4 q = wv::load16(B.pack + 4 * j);
            l.in = true; l.p = (int)q.x; l.len = (int)q.y; l.g = first_node_behind(N, l.c, l.p);
        }
    }
    return l;
}
// pass 1, one wave per tile: tmax[2 t] = largest g, tmax[2 t + 1] = largest chromosome of the tile's Reads blocks (-1: none)
WV_FN void depth_tile_max(const Nodes& N, const Blocks& B, int64_t tile, int32_t* tmax) {
    int g = -1, c = -1;
    for (int it = 0; it < TILE_ROUNDS; ++it) {
        const Lane l = load_lane(N, B, tile * TILE_BLOCKS + it * 64 + wv::lane());
        g = imax(g, l.g); c = imax(c, l.c);
    }
    g = wave_max(g); c = wave_max(c);
    if (wv::lane() == 0) { tmax[2 * tile] = g; tmax[2 * tile + 1] = c; }
}
// pass 2, one wave: front[2 t], front[2 t + 1] = the two maxima over the tiles in front of tile t
WV_FN void depth_prefix(int64_t ntiles, const int32_t* tmax, int32_t* front) {
    int run_g = -1, run_c = -1;
    for (int64_t base = 0; base < ntiles; base += 64) {
        const int64_t t = base + wv::lane();
        const int g = t < ntiles ? tmax[2 * t] : -1, c = t < ntiles ? tmax[2 * t + 1] : -1;
        const int sg = wv::scan_incl_max(g), sc = wv::scan_incl_max(c);
        const int eg = imax(run_g, (int)wv::shfl_up1((uint32_t)sg, (uint32_t)-1)), ec = imax(run_c, (int)wv::shfl_up1((uint32_t)sc, (uint32_t)-1));
        if (t < ntiles) { front[2 * t] = eg; front[2 * t + 1] = ec; }
        run_g = imax(run_g, (int)wv::bcast((uint32_t)sg, 63)); run_c = imax(run_c, (int)wv::bcast((uint32_t)sc, 63));
    }
}
// pass 3, one wave per tile: support[i] / sum[i] += the blocks counted for node i; counters[CNT_HELD] += blocks with m != g,
// counters[CNT_DECREASING] |= 1 when a block's chromosome is smaller than one in front of it
WV_FN void depth_tile_apply(const Nodes& N, const Blocks& B, int64_t tile, const int32_t* front, uint32_t* support, uint32_t* sum, uint32_t* counters) {
    int run_g = front[2 * tile], run_c = front[2 * tile + 1];
    uint32_t held = 0;
    bool decreasing = false;
    for (int it = 0; it < TILE_ROUNDS; ++it) {
        const Lane l = load_lane(N, B, tile * TILE_BLOCKS + it * 64 + wv::lane());
        const int sg = wv::scan_incl_max(l.g), sc = wv::scan_incl_max(l.c);
        const int m = imax(run_g, sg);
        const int c_front = imax(run_c, (int)wv::shfl_up1((uint32_t)sc, (uint32_t)-1));
        const int m_prev = imax(run_g, (int)wv::shfl_up1((uint32_t)sg, (uint32_t)-1));  // (lane 0: the run in front; it opens a run here anyway)
        if (l.in && l.c < c_front) decreasing = true;
        if (l.in && m != l.g) ++held;
        bool counted = false;
        if (l.in && m < N.n) counted = l.c == N.chr[m] && l.p >= N.pos[m] && l.p + l.len <= N.pos[m] + N.len[m];
        // runs of equal m are contiguous (m is monotone over the lanes): inclusive sums, and the last lane of a run takes the run's share
        const uint32_t icnt = wv::scan_incl_add(counted ? 1u : 0u), isum = wv::scan_incl_add(counted ? (uint32_t)l.len : 0u);
        const unsigned long long heads = wv::ballot(wv::lane() == 0 || m_prev != m);
        const int start = 63 - wv::clz64(heads & (wv::lanemask_lt() | (1ull << wv::lane())));
        const uint32_t bcnt = wv::shfl(icnt, (start - 1) & 63), bsum = wv::shfl(isum, (start - 1) & 63);
        const bool tail = wv::lane() == 63 || ((heads >> (wv::lane() + 1)) & 1ull);
        const uint32_t rcnt = icnt - (start > 0 ? bcnt : 0u), rsum = isum - (start > 0 ? bsum : 0u);
        if (tail && rcnt) { wv::glb_atomic_add(support + m, rcnt); wv::glb_atomic_add(sum + m, rsum); }
        run_g = imax(run_g, (int)wv::bcast((uint32_t)sg, 63)); run_c = imax(run_c, (int)wv::bcast((uint32_t)sc, 63));
    }
    const uint32_t h = wv::scan_incl_add(held);
    if (wv::lane() == 63 && h) wv::glb_atomic_add(counters + CNT_HELD, h);
    if (wv::any(decreasing) && wv::lane() == 0) wv::glb_atomic_or(counters + CNT_DECREASING, 1u);
}
}  // namespace bws
