// The table layouts of the device stages, defined once: what a kernel writes into a row, a flag word or a class byte, and what the host
// code that walks those tables reads out of them.  Plain C++ (enums, constexpr values, POD structs, small size functions; nothing that
// needs HIP or sq_wave.h), so the kernel sources (sq_*_stage.inc, sq_bwa_edges.inc, sq_bwa_nodes.inc), their launchers in sq_kernels.hip,
// the host walks (sq_bwa.cpp, sq_segment.cpp) and the CPU harnesses (tools/*_emu.cpp) all read this text, through sq_internal.h.
#pragma once
#include <cstdint>
#include "../../include/squid_hip.h"

namespace sq {
// the columns of a record table (device: RecView::cols, host: HostBatch::cols): what the --bwa record kernels read
struct RecCols {
    int64_t n;
    const int32_t *refid, *pos, *mrefid, *mpos;
    const uint16_t *flag, *totlen;
    const uint8_t *mapq, *aux;  // aux: SQ_AUX_* bits
    const uint32_t* blk_off;
    const int32_t *b_refpos, *b_matchref;
    const uint16_t *b_readpos, *b_matchread;
};

// per-record summary of the kept pass-1 stream, produced on the GPU for the segmentation automaton (host: sq_segment.cpp, device: sgs)
struct StreamRec {
    int32_t refid, pos;      // record.RefID / record.Position
    int32_t fb_refpos, fb_matchref;  // first aligned block in CIGAR order (ReadsMain / window element)
    uint16_t fb_readpos;
    uint8_t flags;           // SR_* bits
    uint8_t nrest;           // number of further blocks (saturated at 255)
    uint32_t rest_off;       // offset of the further blocks in the rest arrays
};
enum : uint8_t { SR_HASBLK = 1, SR_CONC = 2, SR_PART = 4, SR_REV = 8, SR_MATE = 16 /* 0x40 or 0x80 set */ };

// bits of the class byte of a record (cls).  C_P2 ... C_HASSTUB are the record kernels'; C_READS is the --bwa stage's (the record feeds
// Reads), which shares C_P3 with them: dev_breakpoint_support reads it
enum : uint8_t { C_P2 = 1, C_P1 = 2, C_P3 = 4, C_CONC = 8, C_PART = 16, C_HASSTUB = 32, C_READS = 64 };

// the two position indexes over a chromosome: 16 KiB buckets (breakpoint table, cluster table), 1 KiB stretches (node table)
constexpr int NODE_BUCKET_SHIFT = 14, NODE_FINE_SHIFT = 10;
}  // namespace sq

// ---- the chimeric stages (sq_chim_stage.inc)
namespace chs {
enum : uint8_t { CLS_NONE = 0, CLS_DEEP = 1, CLS_SOFT = 2 };  // first block of a fragment
enum : uint32_t { FLAG_FULL = 4, FLAG_ASSERT = 8 };
}  // namespace chs

// ---- --bwa: class byte and node depth (sq_bwa_stage.inc)
namespace bws {
constexpr int TILE_ROUNDS = 16, TILE_BLOCKS = 64 * TILE_ROUNDS;  // blocks of one wave
enum : uint32_t { CNT_HELD = 0, CNT_DECREASING = 1 };
}  // namespace bws

// ---- --bwa: RawEdges' record loop (sq_bwa_edges.inc)
namespace bwe {
// the byte count_record leaves per record: kind (0 = skipped or locates nothing, 1 = first mate, 2 = multi-aligned second mate), `part`,
// the mate stub, and how the own blocks stand in read-offset order (0 = as stored, 1 = reversed, 2 = neither: ranked in fill_record)
enum : uint8_t { M_KIND = 3, M_PART = 4, M_STUB = 8, M_ORDER_SHIFT = 4 };
// the byte edge_fragment leaves per record: which of the three lists it joins
enum : uint8_t { B_PART = 1, B_FIRST_DIS = 2, B_SECOND = 4 };
// next to chs::FLAG_FULL / chs::FLAG_ASSERT: two own blocks of one record share a read offset (std::sort's order is then not defined)
enum : uint32_t { FLAG_TIE = 16 };
static_assert((FLAG_TIE & (chs::FLAG_FULL | chs::FLAG_ASSERT)) == 0, "one flag word");
}  // namespace bwe

// ---- --bwa: BuildNode_BWA's record automaton (sq_bwa_nodes.inc)
namespace bwn {
// the class byte: PASS1 = behind the filter of :871 (seed_step's first return), PASS = it also has a block (seed_record_passes), DISC = not
// pair_concordant, CLIP = concordant and clipped (the partial window), REV, RP15 = first block at a read offset above 15, CUT = gap record
enum : uint8_t { N_PASS1 = 1, N_PASS = 2, N_DISC = 4, N_CLIP = 8, N_REV = 16, N_RP15 = 32, N_CUT = 64 };
constexpr uint8_t W_MASK = N_PASS | N_DISC | N_CLIP, W_CONC = N_PASS, W_PART = N_PASS | N_CLIP, W_DIS = N_PASS | N_DISC;
enum : uint32_t { FLAG_UNSORTED = 1, FLAG_SEEDS_FULL = 2, FLAG_MARGINS_FULL = 4, FLAG_GUARD = 8 };
constexpr int TILE_ROUNDS = 16, TILE_RECS = 64 * TILE_ROUNDS;  // records of one wave of the tile kernels
// one row per stretch (R_SPARE: behind gather_seeds, where the stretch's seeds start in the strung list, in seeds)
enum { R_RL = 0, R_PREV0, R_MARK_START, R_MARK_CHR, R_DIS_RIGHT, R_OTHER_RIGHT, R_BITS, R_MINPOS_DIS, R_MINPOS_OTH, R_READS, R_SEEDS, R_FLUSH_NODES, R_FLUSHES, R_COVER_FAILS, R_MARKS_CLOSED, R_SPARE, REPORT };
enum { B_DIS_SET = 1, B_OTH_SET = 2, B_CLOSING_ZERO = 4 };  // R_BITS
constexpr int THRESH = 3;
// the slices of the stretches together, from nd discordant and nc clipped concordant records in np stretches: seeds (of three words), margins
constexpr int64_t seed_slots(int64_t nd, int64_t nc, int64_t np) { return 8 * nd + 2 * nc + 4 * np; }
constexpr int64_t margin_slots(int64_t nd, int64_t nc) { return 2 * nd + nc; }
// the one row an empty table reports (a zeroed row of REPORT words): one empty stretch
inline void empty_report(int32_t* row, int32_t read_len) {
    row[R_RL] = read_len; row[R_MARK_START] = -1; row[R_MARK_CHR] = -1; row[R_BITS] = B_CLOSING_ZERO; row[R_MINPOS_DIS] = INT32_MAX; row[R_MINPOS_OTH] = INT32_MAX;
}
}  // namespace bwn

// ---- BuildNode_STAR's segmentation automaton (sq_segment_stage.inc)
namespace sgs {
constexpr int THRESH = 3, NEAR = 60;  // thresh, thresh * 20 (SegmentGraph.cpp:286)
constexpr int M_CAP = 1024;           // entries of one margin list (a power of two: the sort pads to it)
constexpr int SENS_CAP = 4;
using Rec = sq::StreamRec;
enum : uint8_t { W_CONC = sq::SR_CONC, W_PART = sq::SR_PART, W_REV = sq::SR_REV, W_MASK = W_CONC | W_PART, W_C = W_CONC, W_P = W_CONC | W_PART };
// the report row of one stretch
enum { R_FLAGS = 0, R_NODES, R_MINCHR, R_BOUND, R_NSENS, R_SENS, R_EXT = R_SENS + SENS_CAP, R_CLUSTERS = R_EXT + 3, R_SUBS, R_MMAX, R_SPARE, REPORT };
enum : int32_t { F_CONSULTED = 1, F_EXIST = 2, F_M_FULL = 4, F_NODES_FULL = 8, F_SENS_FULL = 16, F_GUARD = 32, F_CAPACITY = F_M_FULL | F_NODES_FULL | F_SENS_FULL | F_GUARD };
// one row per active stretch: kept indices (lo, hi] (lo = -1: the head of the stream; hi = K_eff: the stream ends inside), its first cluster,
// kept index that recs[0] would have, the running (otherChr, otherright) in front of record hi, where its nodes go and how many fit
enum { S_LO = 0, S_HI, S_KC, S_SHIFT, S_OCHR, S_ORIGHT, S_NODE_OFF, S_NODE_CAP, STRETCH };
enum { T_MARGIN = 0, T_SUB, T_DENSE, T_REST_FAIL, T_CHR_CHANGE, T_CLIP, T_BLOCKS };  // SGS_TRACE kinds
}  // namespace sgs
