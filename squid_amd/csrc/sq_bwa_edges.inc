// `squid --bwa` on the device (sq_bwa_edges_on_device): the BAM loop of RawEdges (SegmentGraph.cpp:1712-1880, run() of bwa_raw_edges in
// sq_bwa.cpp) as kernels over the resident record table.  Everything here is lane-local (one lane = one record), written in the
// operations of sq_wave.h, so that tools/bwa_edges_emu.cpp runs this source on the CPU (SQ_WAVE_EMU) against the host loop; the
// __global__ wrappers, the scans (device_scan) and the host entry point dev_bwa_raw_edges are in sq_kernels.hip.
//
// The loop carries ONE value from record to record: the node LocateRead starts from, changed only by `if (rn[0] != -1) hint = rn[0]`.
// That is the position chain of the chimeric stages (sq_chim_stage.inc: deep / none / soft first blocks, two scans, runs of soft
// fragments walked by one lane), so the records are first turned into the fragment table of that stage -- one entry per record, what
// prepare() and finish_prepare() of sq_bwa.cpp hand to LocateRead: count_record -> exclusive scan -> fill_record -- and chs::classify,
// chs::soft_list, chs::soft_resolve and chs::hint_of then give every record its exact incoming position.  edge_fragment restates the
// body of the loop behind LocateRead; its edges go into the (key -> count) table of chs::hash_add, the three lists of the loop
// (PartialAlign, FirstDisInserted, the multi-aligned second mates with a discordant would-be edge) come out as one byte per record and
// are compacted in record order (scatter_lists behind three exclusive scans).
#pragma once
#include "sq_wave.h"
#include "sq_chim_stage.inc"
namespace bwe {
using sq::RecCols;
// chs::Frags while it is being written
struct FragsW {
    uint32_t *off, *na;
    int32_t *atot, *btot;
    uint8_t* low;
    int32_t* refid;
    uint8_t* rev;
    int32_t *refpos, *readpos, *matchref, *matchread;
};

// prepare() up to the kind and `part`; cnt[r] = blocks of the record's entry
WV_FN void count_record(const RecCols& R, uint8_t* meta, int32_t* cnt, uint32_t* flags, int64_t r) {
    if (r >= R.n) return;
    meta[r] = 0; cnt[r] = 0;
    const int flag = R.flag[r];
    if ((flag & 0x400) || (flag & 0x4)) return;
    const bool first = (flag & 0x40) != 0, multi = (R.aux[r] & SQ_AUX_MULTI) != 0, low = (R.aux[r] & SQ_AUX_LOWPHRED) != 0;
    if (first ? (multi || R.mapq[r] == 0) : !multi) return;  // :1723-1726 (W5)
    const uint32_t b0 = R.blk_off[r], nown = R.blk_off[r + 1] - b0;
    if (nown == 0) return;
    bool inc = true, dec = true;
    uint32_t kmin = 0, kmax = 0;
    for (uint32_t k = 1; k < nown; ++k) {
        const int p = R.b_readpos[b0 + k], q = R.b_readpos[b0 + k - 1];
        if (!(p > q)) inc = false;
        if (!(p < q)) dec = false;
        if (p < (int)R.b_readpos[b0 + kmin]) kmin = k;
        if (p > (int)R.b_readpos[b0 + kmax]) kmax = k;
    }
    const uint8_t order = inc ? 0 : dec ? 1 : 2;
    if (order == 2) {
        bool tie = false;
        for (uint32_t k = 1; k < nown && !tie; ++k)
            for (uint32_t j = 0; j < k; ++j) if (R.b_readpos[b0 + j] == R.b_readpos[b0 + k]) { tie = true; break; }
        if (tie) wv::glb_atomic_or(flags, FLAG_TIE);
    }
    const int front = R.b_readpos[b0 + kmin], tail = (int)R.totlen[r] - (int)R.b_readpos[b0 + kmax] - (int)R.b_matchread[b0 + kmax];
    const bool part = !multi && !low && (front > 15 || tail > 15);  // clipped_end of the full, uncut own blocks
    const uint8_t kind = first ? ((front <= 15 || low) ? 1 : 0) : 2;
    const bool stub = !(flag & 0x8) && R.mrefid[r] != -1;
    meta[r] = (uint8_t)(kind | (part ? M_PART : 0) | (stub ? M_STUB : 0) | (order << M_ORDER_SHIFT));
    cnt[r] = kind == 0 ? 0 : (kind == 1 ? (int32_t)nown : 1) + (stub ? 1 : 0);
}
// the own block that stands at place k of the read-offset order (ties, flagged by count_record, by index)
WV_FN uint32_t own_at(const RecCols& R, uint32_t b0, uint32_t nown, uint8_t order, uint32_t k) {
    if (order == 0) return k;
    if (order == 1) return nown - 1 - k;
    for (uint32_t j = 0; j < nown; ++j) {
        uint32_t rank = 0;
        const int pj = R.b_readpos[b0 + j];
        for (uint32_t i = 0; i < nown; ++i) { const int pi = R.b_readpos[b0 + i]; if (pi < pj || (pi == pj && i < j)) ++rank; }
        if (rank == k) return j;
    }
    return 0;
}
// the entry of record r behind the scan of the counts (off[r] is there; off[n] is the scan's total): what finish_prepare leaves
WV_FN void fill_record(const RecCols& R, const uint8_t* meta, const FragsW& F, int64_t r) {
    if (r >= R.n) return;
    const uint8_t m = meta[r], kind = m & M_KIND, order = m >> M_ORDER_SHIFT;
    const bool stub = (m & M_STUB) != 0;
    const int flag = R.flag[r];
    const bool first = (flag & 0x40) != 0, low = (R.aux[r] & SQ_AUX_LOWPHRED) != 0;
    F.na[r] = kind == 1 ? R.blk_off[r + 1] - R.blk_off[r] : (kind == 2 && stub ? 1u : 0u);
    F.atot[r] = first ? (int32_t)R.totlen[r] : 0; F.btot[r] = first ? 0 : (int32_t)R.totlen[r];
    F.low[r] = (uint8_t)(low ? (first ? 1 : 2) : 0);
    if (kind == 0) return;
    const uint32_t b0 = R.blk_off[r], nown = R.blk_off[r + 1] - b0;
    uint32_t o = F.off[r];
    const bool rev = (flag & 0x10) != 0;
    if (kind == 2 && stub) { F.refid[o] = R.mrefid[r]; F.rev[o] = (flag & 0x20) ? 1 : 0; F.refpos[o] = R.mpos[r]; F.readpos[o] = 0; F.matchref[o] = 15; F.matchread[o] = 15; ++o; }
    const uint32_t take = kind == 1 ? nown : 1u;
    for (uint32_t k = 0; k < take; ++k, ++o) {
        const uint32_t b = b0 + own_at(R, b0, nown, order, k);
        F.refid[o] = R.refid[r]; F.rev[o] = rev ? 1 : 0; F.refpos[o] = R.b_refpos[b]; F.readpos[o] = R.b_readpos[b];
        F.matchref[o] = kind == 2 ? 15 : R.b_matchref[b]; F.matchread[o] = kind == 2 ? 15 : (int32_t)R.b_matchread[b];
    }
    if (kind == 1 && stub) { F.refid[o] = R.mrefid[r]; F.rev[o] = (flag & 0x20) ? 1 : 0; F.refpos[o] = R.mpos[r]; F.readpos[o] = 0; F.matchref[o] = 15; F.matchread[o] = 15; }
}

// the would-be edge of a multi-aligned second mate (:1852): stub = block o, own block = o + 1
WV_FN unsigned long long second_key(const chs::Frags& F, const int32_t* rn, uint32_t o) { return chs::edge_key(rn[o], F.rev[o] != 0, rn[o + 1], F.rev[o + 1] != 0); }

// run() of bwa_raw_edges behind prepare / finish_prepare, one lane per record.  final_pos: the position behind the last record (W4)
WV_FN void edge_fragment(const chs::Nodes& N, const chs::Frags& F, const chs::Trim& T, int32_t* rn, const chs::Chain& C, const chs::Params& P, const uint8_t* meta,
                         unsigned long long* hk, uint32_t* hv, uint32_t mask, uint32_t* flags, uint8_t* bits, int32_t* final_pos, int64_t q) {
    if (q >= F.nf) return;
    const uint8_t m = meta[q], kind = m & M_KIND;
    uint8_t out = (m & M_PART) ? B_PART : 0;
    bits[q] = out;
    const uint32_t o = F.off[q], nblk = F.off[q + 1] - o, na = F.na[q], nb = nblk - na;
    int hint = chs::hint_of(C, q);
    if (kind != 0 && nblk != 0) {
        int i = hint;
        for (uint32_t k = 0; k < nblk; ++k) {
            chs::Blk b = chs::load_blk(F, F.refpos, F.readpos, F.matchref, F.matchread, o + k);
            rn[o + k] = chs::locate_one(N, i, hint, b);
            chs::store_trimmed(T, o + k, b);
        }
        if (rn[o] != -1) hint = rn[o];
    }
    if (q == F.nf - 1) *final_pos = hint;
    if (kind == 0 || nblk == 0) return;
    if (kind == 1) {
        const int n = N.n;
        for (uint32_t k = 0; k < nblk; ++k)
            if (rn[o + k] == -1) {
                const int h = chs::home_node(N, hint, F.refid[o + k], T.refpos[o + k]);
                if (h < 0 || h + 1 >= n) { wv::glb_atomic_or(flags, chs::FLAG_ASSERT); return; }
                chs::hash_add(hk, hv, mask, chs::edge_key(h, false, h + 1, true), flags);
            }
        for (int mate = 0; mate < 2; ++mate) {
            const uint32_t base = mate ? o + na : o, cnt = mate ? nb : na;
            for (uint32_t k = base; k + 1 < base + cnt; ++k) {
                const int a = rn[k], b = rn[k + 1];
                if (a == b || a == -1 || b == -1) continue;
                chs::hash_add(hk, hv, mask, chs::edge_key(a, F.rev[k] != 0, b, F.rev[k + 1] == 0), flags);
            }
        }
        if (na > 0 && nb > 0) {
            const bool enda = chs::end_discordant(F, T, o, na), endb = chs::end_discordant(F, T, o + na, nb);
            if (!enda && !endb) {
                const int a = rn[o + na - 1], b = rn[o + nblk - 1];
                if (a != b && a != -1 && b != -1 && !chs::pair_overlap(rn + o, (int)na, (int)nb, enda, endb, a, b)) {
                    const unsigned long long key = chs::edge_key(a, F.rev[o + na - 1] != 0, b, F.rev[o + nblk - 1] != 0);
                    chs::hash_add(hk, hv, mask, key, flags);
                    if (chs::edge_discordant(N, P, key)) out |= B_FIRST_DIS;
                }
            }
        }
    } else if (na > 0) {  // (the stub alone is mate a: never end-discordant; `j among rn[0..na)` and `i == rn[na]` are both i == j)
        const int a = rn[o], b = rn[o + 1];
        if (a != b && a != -1 && b != -1 && chs::edge_discordant(N, P, second_key(F, rn, o))) out |= B_SECOND;
    }
    bits[q] = out;
}

// one lane per record behind the three exclusive scans of the list bits: the record's index into every list it is on, in record order
WV_FN void scatter_lists(const chs::Frags& F, const int32_t* rn, const uint8_t* bits, const int32_t* at_part, const int32_t* at_first, const int32_t* at_second, uint32_t* l_part,
                         uint32_t* l_first, uint32_t* l_second, unsigned long long* second_keys, int64_t q) {
    if (q >= F.nf) return;
    const uint8_t b = bits[q];
    if (b & B_PART) l_part[at_part[q]] = (uint32_t)q;
    if (b & B_FIRST_DIS) l_first[at_first[q]] = (uint32_t)q;
    if (b & B_SECOND) { l_second[at_second[q]] = (uint32_t)q; second_keys[at_second[q]] = second_key(F, rn, F.off[q]); }
}
}  // namespace bwe
