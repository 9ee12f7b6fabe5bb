// Fused record-streaming kernels of the graph pass (included by sq_kernels.hip, inside namespace sq).
//
// SURVEY.md section 8(d) counts three passes over the concordant records -- BuildNode_STAR (SegmentGraph.cpp:293-347), RawEdgesOther
// (:1570-1686), ExactBPConcordantSupport (:3126-3166) -- and prices the path at 80 + 24 b bytes per record.  Round 2 ran every step of
// a pass as its own kernel (classify, dedup, two scans, summarise, max-scan, zero coverage, scan, gather, rest candidates: ten reads
// of the record rows for pass 1 alone).  Here a pass is ONE kernel: a workgroup takes a tile of records and keeps them in registers.
// Tiles never wait for each other (the first form of this file chained them with decoupled look-back; polling status words across
// the eight L2s cost more than it saved): what runs along the stream -- rank among the kept records, the running (otherChr,
// otherrightmost) pair, the depth cursor, the breakpoint cursor -- is formed per tile and combined by a small second kernel, derived
// from a monotone key, or assumed, checked and corrected (DESIGN.md section 3).
//
//   k_pass1   filters + concordant/partial classification (:297-303,651-683,1579-1585,3131-3142), consecutive-duplicate drop
//             (ReadRec_t::Equal, :304-318,1587-1600), rank of the kept records, running other-pair (:655-667), zero-coverage records
//             (:616-620), trigger record of every discordant cluster (:353), ConcordRest candidates (:387-389,471-473,690-699)
//   k_summarise_tiles  the 24-byte window elements (:320-337,668-699) of just the stretches the host automaton replays
//   k_depth2  depth sweep cursor (:787-799) + per-node Support / AvgDepth sums (:781-826)
//   k_bp2     breakpoint cursor bound + concordant-fragment support (:3129-3166)

// ------------------------------------------------------------------------------------------------ pass 1
// filter bits of a record from its raw fields (SegmentGraph.cpp:297-303 / :1579-1585): C_P2 | C_P1
__device__ __forceinline__ uint8_t pass_bits(int flag, int aux, int mapq, int refid, int min_mapq) {
    const bool p2 = !(aux & SQ_AUX_MULTI) && !(aux & SQ_AUX_INCHIM) && !(flag & 0x400) && !(flag & 0x4) && mapq >= min_mapq;
    return p2 ? (uint8_t)(C_P2 | (refid != -1 ? C_P1 : 0)) : (uint8_t)0;
}
__device__ __forceinline__ uint8_t pass_bits_at(const RecView& R, int64_t q, int min_mapq) { return pass_bits(R.flag[q], R.aux[q], R.mapq[q], R.refid[q], min_mapq); }
// last record at or below q that passes `bit`, or -1 (the slow path of the duplicate drop: the neighbour did not pass)
__device__ int64_t prev_passing(const RecView& R, int64_t q, uint8_t bit, int min_mapq) {
    while (q >= 0 && !(pass_bits_at(R, q, min_mapq) & bit)) --q;
    return q;
}
// what the next shard has to know about the last pass-1 / pass-2 record of this one (chromosome-sharded runs, exchange 1)
__global__ void k_last_info_raw(RecView R, int min_mapq, int32_t* out) {
    for (int p = 0; p < 2; ++p) {
        const int64_t q = prev_passing(R, R.n - 1, p ? C_P2 : C_P1, min_mapq);
        out[2 * p] = q >= 0 ? 1 : 0;
        bool empty = false;
        if (q >= 0) { ListRec l = list_rec(R, q); empty = l.nown == 0 && !l.stub; }
        out[2 * p + 1] = empty ? 1 : 0;
    }
}

// pass 1 is k_pass1w -- ONE WAVE per tile of 64 * P1_ITEMS records, no LDS, no barrier, the hot path without branches
constexpr int P1_THREADS = 64, P1_ITEMS = 4, P1_TILE = P1_THREADS * P1_ITEMS;
// scalar results of pass 1 (int32 slots of P1Args::sc); k_pass1w writes FLAGS / ZC / REST, k_tile_scan the others
enum { P1S_FLAGS = 0, P1S_KEPT = 1, P1S_ZC = 2, P1S_REST = 3, P1S_FIRST_REFID = 4, P1S_FIRST_POS = 5, P1S_OTHER_LO = 6, P1S_OTHER_HI = 7, P1S_WORDS = 8 };
// bits of sc[P1S_FLAGS]
enum { P1F_UNSORTED = 1, P1F_NEGATIVE_END = 2 };
constexpr int P1_ZFIX = P1_TILE >= 512 ? 4 : (P1_TILE == 256 ? 2 : 1);  // zero-coverage candidates a tile can store without asking for a run of slots
constexpr int P1_VSHIFT = P1_TILE == 512 ? 9 : P1_TILE == 256 ? 8 : 7;
static_assert((1 << P1_VSHIFT) == P1_TILE, "a record inside a tile is addressed with P1_VSHIFT bits");  // a kept record inside the kernels: tile << P1_VSHIFT | rank inside the tile (ascending along the stream)
struct P1Args {
    int min_mapq, prior_mask, RL, ablate;  // ablate (SQUID_P1_ABLATE, timing only): leave the kernel after that many of its sections
    uint8_t *cls, *keep;
    int32_t* tile_cnt;         // [ntiles] kept records of every tile
    int32_t* tile_K;           // [ntiles] k_pass1w: clusters passed by every kept record of the tile (-1: no kept record, or the records have spoken for themselves)
    unsigned long long* tile_ob;       // [ntiles] running (otherChr, otherrightmost) pair over the tile (key + 1, 0: none)
    long long *tile_first, *tile_max;  // sort key of the first kept record of a tile / largest kept key inside it (LLONG_MIN: no kept record)
    // zero-coverage CANDIDATES: the records that have zero coverage with the running pair of their own tile alone (the pair in front
    // of the tile can only take candidates away: k_zfinal); one run of slots per tile, in stream order inside the run
    int32_t *zc_v, *zc_K, *zc_refid, *zc_pos;  // record (tile << P1_VSHIFT | rank in tile), clusters it has passed, its RefID and position
    unsigned long long* zc_ob;         // running pair in front of it inside its tile
    int32_t *tile_zbase, *tile_zcnt;   // [ntiles] first slot and length of a tile's run
    int zcap, zfix_end;                // slots in all; the first zfix_end = ntiles * P1_ZFIX are the tiles' fixed ones
    int32_t* trig;             // [ncl] first kept record (as above) among those that have passed exactly clusters 0..c (INT_MAX-ish: none)
    int32_t *rc_cluster, *rc_pos, *rc_len;  // ConcordRest candidates, unordered
    int rc_cap;
    int32_t* sc;
};
// What ReadRec_t::Equal (ReadRec.cpp:119-141) needs of a record when it has at most one own block -- nearly always enough to tell two
// neighbours apart: number of own blocks, flags (first 1, rev 2, stub 4, filter bits << 4), RefID, mate RefID / position (the 15-base
// stub), first own block in read order
struct NKey { int nown, bits, rid, mrid, mp, e0x, e0y; };
__device__ __forceinline__ NKey nkey_empty() { return NKey{0, 1, 0, 0, 0, 0, 0}; }  // the empty initial lastreadrec
__device__ __forceinline__ NKey nkey_at(const RecView& R, int64_t q, int min_mapq) {
    if (q < 0) return nkey_empty();
    const RecKey k = rec_key(R, q);
    return NKey{k.nown, (k.first ? 1 : 0) | (k.rev ? 2 : 0) | (k.stub ? 4 : 0) | ((int)pass_bits_at(R, q, min_mapq) << 4), k.rid, k.mrid, k.mp, k.e0.x, k.e0.y};
}
// 0: not Equal, 1: Equal, 2: both have the same first own block, the same stub and more than one own block: the other blocks decide.
// Equal tries both assignments of the two lists: own blocks against own blocks (and stub against stub), or own blocks against the
// other record's stub
__device__ __forceinline__ int equal_fast(const NKey& q, const NKey& r) {
    const bool sq = q.bits & 4, sr = r.bits & 4;
    const bool a = q.nown == r.nown && sq == sr && (q.nown == 0 || (q.rid == r.rid && q.e0x == r.e0x && q.e0y == r.e0y)) && (!sq || (q.mrid == r.mrid && q.mp == r.mp));
    const bool b = q.nown == (sr ? 1 : 0) && r.nown == (sq ? 1 : 0) && (q.nown == 0 || (q.rid == r.mrid && q.e0x == r.mp && q.e0y == 15)) &&
                   (r.nown == 0 || (r.rid == q.mrid && r.e0x == q.mp && r.e0y == 15));
    if (b) return 1;
    if (!a) return 0;
    return q.nown > 1 ? 2 : 1;
}
__device__ __forceinline__ long long sort_key(int refid, int pos) { return (long long)(((unsigned long long)(uint32_t)refid << 32) | (uint32_t)((uint32_t)pos ^ 0x80000000u)); }  // signed compare == (refid, pos) compare
// #clusters with (chr, right) < (c, p)
__device__ __forceinline__ int clusters_before(const ClusterView& C, int c, int p) {
    int lo = 0, hi = C.n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (C.chr[mid] < c || (C.chr[mid] == c && C.right[mid] < p)) lo = mid + 1; else hi = mid; }
    return lo;
}
// the same through the position index (k_cluster_buckets): one entry per 16 KiB stretch, the few clusters inside it are walked
__device__ __forceinline__ int clusters_passed_idx(const ClusterView& C, int c, int p) {
    const int first = C.bucket_off[c], last = C.bucket_off[c + 1] - 1;
    int bk = first + (p <= 0 ? 0 : (p >> NODE_BUCKET_SHIFT));
    if (bk > last) bk = last;
    int K = C.bucket[bk];
    while (K < C.n && (C.chr[K] < c || (C.chr[K] == c && C.right[K] < p))) ++K;
    return K;
}
// position index of the cluster table: the answer of clusters_before for the first base of every 16 KiB stretch of every reference
__global__ void k_cluster_buckets(ClusterView C, int total, int32_t* bucket) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    int lo = 0, hi = C.n_ref;  // chromosome of this bucket: last c with bucket_off[c] <= g
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (C.bucket_off[mid] <= g) lo = mid; else hi = mid; }
    bucket[g] = clusters_before(C, lo, (g - C.bucket_off[lo]) << NODE_BUCKET_SHIFT);
}
// the zero-coverage test of SegmentGraph.cpp:616-620 for a kept record at (refid, pos) that has passed K clusters; `pay` = running
// (otherChr, otherrightmost) pair in front of it as key + 1 (0: none), `seed` = the pair of earlier shards.  `uni`: the cluster
// neighbourhood of K is already in u_*
__device__ __forceinline__ bool zero_coverage(const ClusterView& C, int K, bool uni, int u_disChr, int u_disRight, int u_dnChr, int u_dnPos, unsigned long long pay, long long seed, int refid, int pos, int RL,
                                              int* o_chr = nullptr, int* o_right = nullptr) {
    int disChr = u_disChr, disRight = u_disRight, dnChr = u_dnChr, dnPos = u_dnPos;
    if (!uni) {
        disChr = K > 0 ? C.chr[K - 1] : 0; disRight = K > 0 ? C.right[K - 1] : 0;
        dnChr = K < C.n ? C.chr[K] : 0; dnPos = K < C.n ? C.start[K] : 0;  // zero sentinel after the last cluster (ledger B21)
    }
    long long ob = pay ? (long long)(pay - 1) : LLONG_MIN;
    if (ob < seed) ob = seed;
    if (ob < 0) ob = 0;  // initial otherChr = 0, otherrightmost = 0
    const int oChr = (int)(ob >> 32), oRight = (int)(ob & 0xffffffffll);
    if (o_chr) { *o_chr = oChr; *o_right = oRight; }
    const bool disLead = disChr > oChr || (disChr == oChr && disRight > oRight);
    const int curRight = disLead ? disRight : oRight, curChr = disChr > oChr ? disChr : oChr;
    return (refid != curChr || pos > curRight + RL) && (curChr < dnChr || (curChr == dnChr && curRight + RL < dnPos));
}
// #clusters with (chr, right) < (refid, pos), all lanes of the wave working on the same query: 64 probes per round
__device__ __forceinline__ int wave_clusters_passed(const ClusterView& C, int refid, int pos) {
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = C.n;  // the answer lies in [lo, hi]
    while (hi > lo) {
        const int span = hi - lo, step = (span + 63) >> 6;
        const int idx = lo + lane * step;
        bool less = false;
        if (idx < hi) { const int ch = C.chr[idx]; less = ch < refid || (ch == refid && C.right[idx] < pos); }
        const int cnt = (int)__popcll(__ballot(less));  // monotone: the first cnt probes are below the query
        if (cnt == 0) { hi = lo; break; }
        const int nlo = lo + (cnt - 1) * step + 1, nhi = lo + cnt * step;
        lo = nlo; hi = nhi < hi ? nhi : hi;
    }
    return lo;
}
__device__ __forceinline__ bool key_equal_full(const RecView& R, int64_t q, int64_t r) { return key_equal(R, rec_key(R, q), rec_key(R, r)); }
// the duplicate drop of one record in full generality (the neighbour failed a filter, the first record of the stream, sharded runs):
// eq1 / eq2 = Equal to the last record that passed filter 1 / filter 2.  (a real call costs the whole kernel its registers: inlined; the hot path of k_pass1 is the neighbour case)
__device__ __forceinline__ void dedup_general(const RecView& R, int64_t r, uint8_t c, const NKey& km, const NKey& kr, int prior_mask, int min_mapq, bool& eq1, bool& eq2) {
    const uint8_t pm = (uint8_t)(km.bits >> 4);
    auto same_as_prev = [&](uint8_t bit, int64_t& q, int prior) -> bool {
        NKey kq = km;
        q = r - 1;
        if (!(r > 0 && (pm & bit))) {  // the neighbour did not pass: walk back over the raw fields
            q = prev_passing(R, r - 2, bit, min_mapq);
            if (q < 0) q = -1;
            kq = nkey_at(R, q, min_mapq);
        }
        if (q < 0 && prior) return false;  // (sharded run: a record with non-empty lists precedes this shard, on another chromosome)
        const int e = equal_fast(kq, kr);
        return e == 2 ? key_equal_full(R, q, r) : e == 1;
    };
    int64_t p1 = -1, p2 = -1;
    eq1 = true; eq2 = true;
    if (c & C_P1) eq1 = same_as_prev(C_P1, p1, prior_mask & 1);
    if (c & C_P2) {
        eq2 = same_as_prev(C_P2, p2, prior_mask & 2);
        if ((c & C_P1) && p2 >= 0 && p1 == p2) eq2 = eq1;
    }
}
// ---- wave-level data movement on the vector ALU (DPP) instead of ds_bpermute: a value from the lane below, a 32-bit max-scan, sums
// and maxima over the wave.  (gfx9 DPP controls: row_shr:n 0x110+n inside rows of 16, row_bcast:15 / :31 0x142 / 0x143 carry a row's
// last lane into the next row(s), wave_shr:1 0x138 shifts the whole wave; lanes without a source read 0 = the identity of every use here.)
__device__ __forceinline__ int dpp_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }  // lane l <- lane l - 1, lane 0 <- 0
#define SQ_DPP_SCAN(x, OP)                                                              \
    x = OP(x, __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true));                \
    x = OP(x, __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true));                \
    x = OP(x, __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true));                \
    x = OP(x, __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true));                \
    x = OP(x, __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false));               \
    x = OP(x, __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false));
__device__ __forceinline__ int sq_maxu(int a, int b) { return (int)((unsigned int)a > (unsigned int)b ? (unsigned int)a : (unsigned int)b); }
__device__ __forceinline__ int sq_add(int a, int b) { return a + b; }
__device__ __forceinline__ unsigned int wave_maxscan_incl_u32(unsigned int v) { int x = (int)v; SQ_DPP_SCAN(x, sq_maxu) return (unsigned int)x; }  // identity 0
__device__ __forceinline__ int wave_sum_i32(int v) { int x = v; SQ_DPP_SCAN(x, sq_add) return __builtin_amdgcn_readlane(x, 63); }             // same value in every lane (scalar)
__device__ __forceinline__ unsigned int wave_max_u32(unsigned int v) { int x = (int)v; SQ_DPP_SCAN(x, sq_maxu) return (unsigned int)__builtin_amdgcn_readlane(x, 63); }
// exclusive max-scan of a 64-bit payload (0 = identity) over the wave with DPP row shifts (no LDS traffic); `total` = wave maximum
__device__ __forceinline__ unsigned long long wave_maxscan_excl_u64(unsigned long long x, unsigned long long& total) {
    uint32_t h = (uint32_t)(x >> 32), l = (uint32_t)x;
#define SQ_MAX_STEP(ctrl, rmask)                                                                     \
    {                                                                                                \
        const uint32_t h2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)h, ctrl, rmask, 0xf, false); \
        const uint32_t l2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)l, ctrl, rmask, 0xf, false); \
        if (h2 > h || (h2 == h && l2 > l)) { h = h2; l = l2; }                                         \
    }
    SQ_MAX_STEP(0x111, 0xf)  // row_shr:1
    SQ_MAX_STEP(0x112, 0xf)  // row_shr:2
    SQ_MAX_STEP(0x114, 0xf)  // row_shr:4
    SQ_MAX_STEP(0x118, 0xf)  // row_shr:8
    SQ_MAX_STEP(0x142, 0xa)  // row_bcast:15 -> rows 1, 3
    SQ_MAX_STEP(0x143, 0xc)  // row_bcast:31 -> rows 2, 3
#undef SQ_MAX_STEP
    total = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)h, 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)l, 63);
    return ((unsigned long long)(uint32_t)dpp_shr1((int)h) << 32) | (uint32_t)dpp_shr1((int)l);  // (lane 0: 0)
}
// ------------------------------------------------------------------------------------------------ pass 1, one wave per tile
// Round 5.  The four-wave form of rounds 3/4 (k_pass1, a workgroup per tile of 512 records; removed) issued 1291 vector + 960 scalar instructions per wave of 128 records (SQ counters, round 4): with
// five waves per SIMD each "issuing" a quarter of its life, the SIMD's issue port is busy all the time -- the kernel is bound by the
// NUMBER OF INSTRUCTIONS, not by memory (its loads alone run at 5.9 TB/s) and not by latency.  Two thirds of them were control flow and
// bookkeeping of the workgroup form: 393 exec-mask branches in the code, (item, wave) slots combined through LDS behind two barriers,
// SGPRs spilled into VGPR lanes.  Here a tile IS a wave: lane l holds records base + i * 64 + l, the stream order inside the tile is
// (item, lane), everything that runs along the stream inside the tile moves through DPP / readlane, nothing through LDS; the common
// case of every step is straight-line predicated code and every rare case (the neighbour failed a filter, equal first blocks, a record
// outside the tile's cluster bracket, a ConcordRest candidate, a chromosome change inside the tile) sits behind ONE wave-uniform test.
// NKey with nown and the flag bits in one word -- bits 0..5 as NKey::bits (first 1, rev 2, stub 4, pass bits << 4), nown << 8 -- and the
// SECOND own block in read order of a record that has exactly two (o1x, o1y; else 0): two such records with equal first blocks -- a
// spliced pair read twice -- are told apart in registers; only three and more blocks send Equal to memory
struct PKey { int kb, rid, mrid, mp, e0x, e0y, o1x, o1y; };
__device__ __forceinline__ NKey pkey_n(const PKey& k) { return NKey{(int)((uint32_t)k.kb >> 8), k.kb & 0xff, k.rid, k.mrid, k.mp, k.e0x, k.e0y}; }
__device__ __forceinline__ PKey pkey_of(const int4& w0, const int4& w1, const int4& qa, const int4& qb, int pbits) {
    const int flag = (int)((uint32_t)w1.x & 0xffffu), nown = (int)((uint32_t)w1.y >> 16);
    const int rev = (flag >> 4) & 1, stub = (int)(!(flag & 0x8) & (w0.z != -1));
    const int4 e0 = rev ? qb : qa;  // the first own block in read order
    PKey k;
    k.kb = ((flag >> 6) & 1) | (rev << 1) | (stub << 2) | (pbits << 4) | (nown << 8);
    k.rid = w0.x; k.mrid = w0.z; k.mp = w0.w; k.e0x = nown > 0 ? e0.x : 0; k.e0y = nown > 0 ? e0.y : 0;
    const int4 o1 = rev ? qa : qb;  // (two own blocks: the other one)
    k.o1x = nown == 2 ? o1.x : 0; k.o1y = nown == 2 ? o1.y : 0;
    return k;
}
// equal_fast on packed keys, straight-line: 0 not Equal, 1 Equal, 2 the other own blocks decide
__device__ __forceinline__ int pequal_fast(const PKey& q, const PKey& r) {
    const int qn = (int)((uint32_t)q.kb >> 8), rn = (int)((uint32_t)r.kb >> 8);
    const int sq_ = (q.kb >> 2) & 1, sr = (r.kb >> 2) & 1;
    const int blk_same = (int)((q.rid == r.rid) & (q.e0x == r.e0x) & (q.e0y == r.e0y));
    const int stub_same = (int)((q.mrid == r.mrid) & (q.mp == r.mp));
    const int a = (int)((qn == rn) & (sq_ == sr)) & ((int)(qn == 0) | blk_same) & ((sq_ ^ 1) | stub_same);
    const int b = (int)((qn == sr) & (rn == sq_)) & ((int)(qn == 0) | (int)((q.rid == r.mrid) & (q.e0x == r.mp) & (q.e0y == 15))) &
                  ((int)(rn == 0) | (int)((r.rid == q.mrid) & (r.e0x == q.mp) & (r.e0y == 15)));
    const int two_same = (int)((q.o1x == r.o1x) & (q.o1y == r.o1y));
    return b ? 1 : (a ? (qn > 2 ? 2 : (qn == 2 ? two_same : 1)) : 0);
}
// lane l <- lane l - 1, lane 0 <- `first` (wave_shr:1 with the old value kept where no source lane exists)
__device__ __forceinline__ int dpp_shr1_from(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ unsigned int wave_maxscan_incl_u32_total(unsigned int v, unsigned int& total) { int x = (int)v; SQ_DPP_SCAN(x, sq_maxu) total = (unsigned int)__builtin_amdgcn_readlane(x, 63); return (unsigned int)x; }
template <int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_pass1w(RecView R, ClusterView C, P1Args A) {
    constexpr int IT = P1_ITEMS;
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int64_t tbase = (int64_t)tile * P1_TILE;
    const unsigned long long ltmask = (1ull << lane) - 1;
    // ---- loads, every one unconditional (indices clamped into the arrays): the two 16-byte words of every record, then its first and
    // last block; the record in front of the tile the same way (wave-uniform addresses)
    int4 w0[IT], w1[IT], qa[IT], qb[IT];
    bool live[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int64_t r = tbase + i * 64 + lane;
        live[i] = r < R.n;
        const int64_t rc = live[i] ? r : R.n - 1;  // (the grid exists only for R.n > 0)
        w0[i] = R.r_pack[2 * rc]; w1[i] = R.r_pack[2 * rc + 1];
    }
    const int64_t rp = tbase > 0 ? tbase - 1 : 0;
    const int4 pw0 = R.r_pack[2 * rp], pw1 = R.r_pack[2 * rp + 1];
    const bool have_blocks = R.nb > 0;  // (uniform)
    int4 pqa = make_int4(0, 0, 0, 0), pqb = pqa;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const uint32_t bo = (uint32_t)w1[i].z, nblk = (uint32_t)w1[i].y >> 16;
        qa[i] = make_int4(0, 0, 0, 0); qb[i] = qa[i];
        if (have_blocks) { qa[i] = R.b_pack[nblk > 0 ? bo : 0u]; qb[i] = R.b_pack[nblk > 1 ? bo + nblk - 1 : (nblk > 0 ? bo : 0u)]; }
    }
    if (have_blocks) {
        const uint32_t bo = (uint32_t)pw1.z, nblk = (uint32_t)pw1.y >> 16;
        pqa = R.b_pack[nblk > 0 ? bo : 0u]; pqb = R.b_pack[nblk > 1 ? bo + nblk - 1 : (nblk > 0 ? bo : 0u)];
    }
    // ---- the tile's cluster bracket (SegmentGraph.cpp:353: #clusters with (chr, right) < (RefID, position)): the answers for the tile's
    // first and last record bracket everybody's on a sorted stream and nearly always agree; uniform (scalar) loads, issued beside the
    // vector loads above
    const bool have_cl = C.n > 0;  // (uniform)
    bool t_uni = false;
    int t_K = 0, t_dc = 0, t_dr = 0, t_uc = 0, t_us = 0, t_ur = 0;
    long long t_key0 = 0, t_key1 = 0;
    {
        const int64_t ra = tbase, rb = (tbase + P1_TILE < R.n ? tbase + P1_TILE : R.n) - 1;
        const int ref_a = R.refid[ra], pos_a = R.pos[ra], ref_b = R.refid[rb], pos_b = R.pos[rb];
        t_key0 = sort_key(ref_a, pos_a); t_key1 = sort_key(ref_b, pos_b);
        if (have_cl && ref_a >= 0 && ref_a < C.n_ref && ref_b >= 0 && ref_b < C.n_ref && t_key0 <= t_key1) {
            const int K0 = clusters_passed_idx(C, ref_a, pos_a), K1 = clusters_passed_idx(C, ref_b, pos_b);
            if (K0 == K1) {
                t_uni = true; t_K = K0;
                if (K0 > 0) { t_dc = C.chr[K0 - 1]; t_dr = C.right[K0 - 1]; }
                if (K0 < C.n) { t_uc = C.chr[K0]; t_us = C.start[K0]; t_ur = C.right[K0]; }  // (zero sentinel after the last cluster, ledger B21)
            }
        }
    }
    if (A.ablate == 1) {
#pragma unroll
        for (int i = 0; i < IT; ++i) if (live[i]) A.cls[tbase + i * 64 + lane] = (uint8_t)(w0[i].x ^ w0[i].y ^ w0[i].z ^ w0[i].w ^ w1[i].x ^ w1[i].y ^ qa[i].x ^ qb[i].y ^ qa[i].z ^ pqa.x ^ pw0.x ^ t_K);
        return;
    }
    // key of the record in front of the tile (nothing precedes the first record of the stream: the empty record without a filter bit)
    PKey kprev = pkey_of(pw0, pw1, pqa, pqb, pass_bits((int)((uint32_t)pw1.x & 0xffffu), (int)(((uint32_t)pw1.y >> 8) & 0xffu), (int)((uint32_t)pw1.y & 0xffu), pw0.x, A.min_mapq));
    if (tbase == 0) kprev = PKey{1, 0, 0, 0, 0, 0, 0, 0};
    // the last record in front of the tile that passed the filters, if it is the record right in front (else: unknown without a walk)
    PKey carry = kprev;
    bool carry_ok = tbase > 0 && ((kprev.kb >> 4) & 3) == (C_P1 | C_P2), filters_differ = tbase > 0 && ((kprev.kb >> 4) & 3) == C_P2;  // (uniform)
    // ---- along the tile
    int kept_before = 0;                      // kept records of the earlier items (uniform)
    unsigned long long ob_carry = 0;          // running (otherChr, otherrightmost) pair over the earlier items (key + 1, 0: none)
    unsigned long long key_carry = 0;         // largest kept sort key so far, + 1 (0: none)
    long long tile_first = LLONG_MIN;
    bool unsorted = false, negend = false;
    int rank_in[IT], Kc[IT];
    unsigned long long ob_front[IT];          // running pair in front of the record inside its tile
    unsigned long long zmask[IT];             // (uniform) zero-coverage candidates of the item
    int K_last_kept = -1;                     // (uniform) clusters passed by the last kept record so far (general trigger path)
    bool tile_nonuni = false;                 // (uniform) some kept record lies outside the tile's cluster bracket
    int K_first_kept = -1;                    // (uniform) clusters passed by the tile's first kept record
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int64_t r = tbase + i * 64 + lane;
        const int refid = w0[i].x, pos = w0[i].y, mrefid = w0[i].z, mpos = w0[i].w;
        const int flag = (int)((uint32_t)w1[i].x & 0xffffu), totlen = (int)((uint32_t)w1[i].x >> 16);
        const int mapq = (int)((uint32_t)w1[i].y & 0xffu), aux = (int)(((uint32_t)w1[i].y >> 8) & 0xffu), nblk = (int)((uint32_t)w1[i].y >> 16);
        // ---- classification (SegmentGraph.cpp:297-303,651-683,1579-1585,3131-3142), straight-line
        const int mapped = (~flag >> 2) & 1, matemapped = (~flag >> 3) & 1, rev = (flag >> 4) & 1, materev = (flag >> 5) & 1, proper = (flag >> 1) & 1, mate12 = (int)((flag & 0xC0) != 0);
        const int p2 = (int)(!(aux & (SQ_AUX_MULTI | SQ_AUX_INCHIM)) & !(flag & 0x404) & (mapq >= A.min_mapq)) & (int)live[i];
        const int p1 = p2 & (int)(refid != -1);
        const int samechr = (int)(mrefid == refid);
        const int skip3 = matemapped & samechr & ((int)(mpos > pos) | ((int)(mpos == pos) & ((flag >> 7) & 1)));
        const unsigned int d = rev ? (unsigned int)pos - (unsigned int)mpos : (unsigned int)mpos - (unsigned int)pos;  // (rev && !materev: pos - mpos in [0, 750000]; !rev && materev: mpos - pos)
        const int conc = (int)live[i] & mapped & matemapped & (int)(mrefid != -1) & samechr & proper & (rev ^ materev) & (int)(d <= 750000u) & (int)(nblk > 0);
        const int4 f4 = rev ? qb[i] : qa[i], b4 = rev ? qa[i] : qb[i];  // first / last block in read-offset order
        const int f_readpos = (int)((uint32_t)f4.z & 0xffffu), b_readpos = (int)((uint32_t)b4.z & 0xffffu), b_matchread = (int)((uint32_t)b4.z >> 16);
        const int part = conc & mate12 & (int)!(aux & SQ_AUX_LOWPHRED) & ((int)(f_readpos > 15) | (int)(totlen - b_readpos - b_matchread > 15));
        const int hasstub = (int)live[i] & matemapped & (int)(mrefid != -1);
        const int c = p2 * C_P2 | p1 * C_P1 | (p1 & (skip3 ^ 1)) * C_P3 | conc * C_CONC | part * C_PART | hasstub * C_HASSTUB;
        // ---- the key ReadRec_t::Equal looks at, and the one of the record in front (lane below; lane 0: the last lane of the 64 in front)
        PKey kq = pkey_of(w0[i], w1[i], qa[i], qb[i], c & (C_P1 | C_P2));
        if (!live[i]) kq = PKey{1, 0, 0, 0, 0, 0, 0, 0};
        // ---- consecutive-duplicate drop: Equal to the previous record that passes the same filter.  That record is nearly always the
        // neighbour; when the neighbour failed a filter (a multi-mapper, a name of the chimeric file: 2 % of the records, so most waves hold one)
        // it is the nearest lane below that passed, or the last passing record of the 64 in front -- all of them in registers.  Memory is
        // walked (dedup_general) only when the record in front of the TILE failed, when the two filters disagree somewhere in the tile (a
        // mapped record without a reference), or when two records share their first block and their mate (the other blocks decide).
        const unsigned long long m2 = __ballot(p2 != 0), m1 = __ballot(p1 != 0);
        if (m1 != m2) filters_differ = true;  // (uniform, sticky)
        const unsigned long long b2 = m2 & ltmask;
        const int src = b2 ? 63 - __clzll((long long)b2) : 0;
        PKey kp;
        kp.kb = __shfl(kq.kb, src, 64); kp.rid = __shfl(kq.rid, src, 64); kp.mrid = __shfl(kq.mrid, src, 64);
        kp.mp = __shfl(kq.mp, src, 64); kp.e0x = __shfl(kq.e0x, src, 64); kp.e0y = __shfl(kq.e0y, src, 64);
        kp.o1x = __shfl(kq.o1x, src, 64); kp.o1y = __shfl(kq.o1y, src, 64);
        if (!b2) kp = carry;
        const int e = pequal_fast(kp, kq);
        const int simple = (int)((b2 != 0ull) | carry_ok) & (int)(e != 2) & (int)!filters_differ;
        bool eq1 = e == 1, eq2 = e == 1;
        const bool slow = p2 && !simple && !(A.ablate & 2);
        if (__ballot(slow)) {  // (uniform; dedup_general wants the NEIGHBOUR's key -- all lanes fetch it -- and walks by itself when the neighbour did not pass)
            PKey km = kq;
            km.kb = dpp_shr1_from(kprev.kb, kq.kb); km.rid = dpp_shr1_from(kprev.rid, kq.rid); km.mrid = dpp_shr1_from(kprev.mrid, kq.mrid);
            km.mp = dpp_shr1_from(kprev.mp, kq.mp); km.e0x = dpp_shr1_from(kprev.e0x, kq.e0x); km.e0y = dpp_shr1_from(kprev.e0y, kq.e0y);
            if (slow) dedup_general(R, r, (uint8_t)c, pkey_n(km), pkey_n(kq), A.prior_mask, A.min_mapq, eq1, eq2);
        }
        kprev.kb = __builtin_amdgcn_readlane(kq.kb, 63); kprev.rid = __builtin_amdgcn_readlane(kq.rid, 63); kprev.mrid = __builtin_amdgcn_readlane(kq.mrid, 63);
        kprev.mp = __builtin_amdgcn_readlane(kq.mp, 63); kprev.e0x = __builtin_amdgcn_readlane(kq.e0x, 63); kprev.e0y = __builtin_amdgcn_readlane(kq.e0y, 63);
        if (m2) {  // (uniform) the last passing record so far
            const int l2 = 63 - __clzll((long long)m2);
            carry.kb = __builtin_amdgcn_readlane(kq.kb, l2); carry.rid = __builtin_amdgcn_readlane(kq.rid, l2); carry.mrid = __builtin_amdgcn_readlane(kq.mrid, l2);
            carry.mp = __builtin_amdgcn_readlane(kq.mp, l2); carry.e0x = __builtin_amdgcn_readlane(kq.e0x, l2); carry.e0y = __builtin_amdgcn_readlane(kq.e0y, l2);
            carry.o1x = __builtin_amdgcn_readlane(kq.o1x, l2); carry.o1y = __builtin_amdgcn_readlane(kq.o1y, l2);
            carry_ok = true;
        }
        // whetherbuildedge (SegmentGraph.cpp:1601-1605) on the stub-augmented, sorted record: the stub side always has ReadPos 0 <= 15;
        // the own side is tested with its own low-Phred flag
        const int build = (int)(nblk == 0) | (((kq.kb >> 2) & 1) ^ 1) | (int)(f_readpos <= 15) | (int)((aux & SQ_AUX_LOWPHRED) != 0);
        const int k1 = p1 & (int)!eq1, k2 = p2 & (int)!eq2;
        const int k = k1 * K_1 | k2 * K_2 | (k2 & build) * K_BUILD | ((c & C_P3) ? K_P3 : 0);
        if (live[i] && !(A.ablate & 128)) { A.cls[r] = (uint8_t)c; A.keep[r] = (uint8_t)k; }
        // ---- along the kept stream: rank, running (otherChr, otherrightmost) pair (SegmentGraph.cpp:655-667; a max-scan on a sorted
        // stream), order of the kept records (the stream must be coordinate sorted: README.md:23)
        const bool kept = k1;
        const unsigned long long km64 = __ballot(kept);
        rank_in[i] = kept_before + (int)__popcll(km64 & ltmask);
        const bool pays = kept && conc && mate12;
        const int end = qa[i].x + qa[i].y;
        if (pays && (end < 0 || refid < 0)) negend = true;
        // one chromosome over the kept records of the item (the rule; anything else: the 64-bit scans): the high words of all keys are the
        // same.  Keys travel as biased unsigned numbers (sort_key ^ 2^63: unsigned order == (refid, pos) order) + 1, 0 = none
        const int ref0 = km64 ? __builtin_amdgcn_readlane(refid, __ffsll((long long)km64) - 1) : 0;
        const bool one_chr = __ballot(kept && refid != ref0) == 0ull && ref0 >= 0;  // (uniform)
        const long long sk = sort_key(refid, pos);
        const unsigned long long uk1 = ((unsigned long long)sk ^ 0x8000000000000000ull) + 1ull;
        unsigned long long ob_excl, ob_tot, key_excl, key_tot;
        if (A.ablate & 64) { ob_excl = 0; ob_tot = 0; key_excl = 0; key_tot = 0; }
        else if (one_chr) {
            unsigned int tot32;
            const unsigned int pl = pays ? (unsigned int)end + 1u : 0u;
            const unsigned int incl = wave_maxscan_incl_u32_total(pl, tot32);
            const unsigned int ex = (unsigned int)dpp_shr1((int)incl);
            ob_excl = ex ? (((unsigned long long)(uint32_t)ref0 << 32) | ex) : 0ull;
            ob_tot = tot32 ? (((unsigned long long)(uint32_t)ref0 << 32) | tot32) : 0ull;
            // (low word of sort_key: pos ^ 0x80000000 -- 0 only for pos == INT_MIN, which no kept record has: + 1 would overflow for pos == -1 only)
            const unsigned int kl = kept ? ((uint32_t)pos ^ 0x80000000u) : 0u;
            unsigned int ktot32;
            const unsigned int kincl = wave_maxscan_incl_u32_total(kl, ktot32);
            const unsigned int kex = (unsigned int)dpp_shr1((int)kincl);
            const unsigned long long hi = (unsigned long long)((uint32_t)ref0 ^ 0x80000000u) << 32;
            key_excl = kex ? (hi | kex) + 1ull : 0ull;
            key_tot = ktot32 ? (hi | ktot32) + 1ull : 0ull;
        } else {
            const unsigned long long pay = pays ? ((((unsigned long long)(uint32_t)refid << 32) | (uint32_t)end) + 1ull) : 0ull;
            ob_excl = wave_maxscan_excl_u64(pay, ob_tot);
            key_excl = wave_maxscan_excl_u64(kept ? uk1 : 0ull, key_tot);
        }
        ob_front[i] = ob_excl > ob_carry ? ob_excl : ob_carry;
        const unsigned long long key_before = key_excl > key_carry ? key_excl : key_carry;
        if (kept && uk1 < key_before) unsorted = true;
        if (km64 && tile_first == LLONG_MIN) {  // (uniform) first kept record of the tile
            const int fl_ = __ffsll((long long)km64) - 1;
            tile_first = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(sk >> 32), fl_) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)sk, fl_));
        }
        ob_carry = ob_tot > ob_carry ? ob_tot : ob_carry;
        key_carry = key_tot > key_carry ? key_tot : key_carry;
        kept_before += (int)__popcll(km64);
        // ---- clusters passed, zero coverage (SegmentGraph.cpp:616-620) with the running pair of this tile alone (k_zfinal repeats the test with
        // the pair in front of the tile: it can only turn false when the pair grows), ConcordRest candidates (:690-699 pushes, :387-389 pops)
        int K = t_K, dc = t_dc, dr = t_dr, uc = t_uc, us = t_us, ur = t_ur;
        const bool uni = !have_cl || (t_uni && sk >= t_key0 && sk <= t_key1);
        if (kept && !uni && !(A.ablate & 4)) {  // (rare: an unsorted stretch of filtered-out records in front, or a tile that a cluster ends in)
            if (refid < 0 || refid >= C.n_ref) negend = true;
            else {
                K = clusters_passed_idx(C, refid, pos);
                dc = K > 0 ? C.chr[K - 1] : 0; dr = K > 0 ? C.right[K - 1] : 0;
                uc = K < C.n ? C.chr[K] : 0; us = K < C.n ? C.start[K] : 0; ur = K < C.n ? C.right[K] : 0;
            }
        }
        Kc[i] = kept ? K : 0;
        const bool z = kept && !(A.ablate & 32) && zero_coverage(C, K, true, dc, dr, uc, us, ob_front[i], LLONG_MIN, refid, pos, A.RL);
        zmask[i] = __ballot(z);
        // a non-first block of a concordant record is a candidate for the first cluster whose right end lies beyond it when it starts
        // at or behind that cluster's start - ReadLen; blocks ascend, so a record whose LAST block lies in front of both cluster K's right
        // end and its start - ReadLen has none
        if (kept && conc && mate12 && nblk > 1 && K < C.n && uc == refid && !(qb[i].x < ur && qb[i].x < us - A.RL) && !(A.ablate & 8)) {
            const uint32_t bo = (uint32_t)w1[i].z;
            for (int b = 1; b < nblk; ++b) {
                const int4 q = b == nblk - 1 ? qb[i] : R.b_pack[bo + (uint32_t)b];
                const int p = q.x;
                int lo = K, l_chr = uc, l_start = us;
                if (ur <= p) {  // first cluster on this chromosome whose right end lies beyond p
                    int hi = C.n;
                    ++lo;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (C.chr[mid] < refid || (C.chr[mid] == refid && C.right[mid] <= p)) lo = mid + 1; else hi = mid; }
                    if (lo < C.n) { l_chr = C.chr[lo]; l_start = C.start[lo]; }
                }
                if (lo < C.n && l_chr == refid && p >= l_start - A.RL) {
                    const int s = atomicAdd(&A.sc[P1S_REST], 1);
                    if (s < A.rc_cap) { A.rc_cluster[s] = lo; A.rc_pos[s] = p; A.rc_len[s] = q.y; }
                }
            }
        }
        // ---- trigger of cluster K - 1 (SegmentGraph.cpp:353): the first kept record with K clusters behind it.  A tile whose kept records
        // have all passed the tile's t_K clusters only reports that number (tile_K): k_tile_scan lets the first tile of every run of equal
        // numbers speak for the run.  (Round 5's first form asked trig[] from every tile: thousands of tiles in flight found the initial
        // value there and queued on the same few words with their atomics -- 1.2 ms of a 2.6 ms kernel.)  Records outside the bracket
        // speak for themselves; any superset of the true triggers may try (atomicMin)
        if (km64 && !(A.ablate & 16)) {  // (uniform)
            const unsigned long long nonuni = __ballot(kept && !uni);
            if (K_first_kept < 0) K_first_kept = __builtin_amdgcn_readlane(K, __ffsll((long long)km64) - 1);
            if (nonuni || tile_nonuni) {
                tile_nonuni = true;
                const unsigned long long below = km64 & ltmask;
                const int Kshf = __shfl(K, below ? 63 - __clzll((long long)below) : 0, 64);  // (unconditional: every source lane takes part)
                const int Kp = below ? Kshf : K_last_kept;
                const int v = (tile << P1_VSHIFT) | rank_in[i];
                if (kept && K > 0 && K != Kp && A.trig[K - 1] > v) atomicMin(&A.trig[K - 1], v);
            }
            K_last_kept = __builtin_amdgcn_readlane(K, 63 - __clzll((long long)km64));
        }
    }
    if (unsorted) atomicOr(&A.sc[P1S_FLAGS], P1F_UNSORTED);
    if (negend) atomicOr(&A.sc[P1S_FLAGS], P1F_NEGATIVE_END);
    // ---- the zero-coverage candidates of the tile take one run of slots, in stream order (a tile with at most P1_ZFIX of them uses its
    // own fixed slots: no round trip to a counter)
    int tile_z = 0;
#pragma unroll
    for (int i = 0; i < IT; ++i) tile_z += (int)__popcll(zmask[i]);
    int zb = tile * P1_ZFIX;
    if (tile_z > P1_ZFIX) {  // (uniform)
        int b = 0;
        if (lane == 0) b = A.zfix_end + atomicAdd(&A.sc[P1S_ZC], tile_z);
        zb = __builtin_amdgcn_readfirstlane(b);
    }
    if (lane == 0) {
        A.tile_first[tile] = tile_first; A.tile_max[tile] = key_carry ? (long long)((key_carry - 1ull) ^ 0x8000000000000000ull) : LLONG_MIN;
        A.tile_cnt[tile] = kept_before; A.tile_ob[tile] = ob_carry;
        A.tile_zbase[tile] = zb; A.tile_zcnt[tile] = tile_z;
        // (a tile with records outside its bracket reports nothing: from the first such record on its records have tried above, and the
        // tile's first kept record -- rank 0 -- tries here)
        A.tile_K[tile] = kept_before && !tile_nonuni ? t_K : -1;
        if (tile_nonuni && K_first_kept > 0 && A.trig[K_first_kept - 1] > (tile << P1_VSHIFT)) atomicMin(&A.trig[K_first_kept - 1], tile << P1_VSHIFT);
    }
    if (tile_z) {  // (uniform)
        int zrun = 0;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            if ((zmask[i] >> lane) & 1ull) {
                const int slot = zb + zrun + (int)__popcll(zmask[i] & ltmask);
                if (slot < A.zcap) { A.zc_v[slot] = (tile << P1_VSHIFT) | rank_in[i]; A.zc_K[slot] = Kc[i]; A.zc_ob[slot] = ob_front[i]; A.zc_refid[slot] = w0[i].x; A.zc_pos[slot] = w0[i].y; }
            }
            zrun += (int)__popcll(zmask[i]);
        }
    }
}
// What runs along the stream, from the per-tile results of k_pass1: kept records and running pair in front of every tile, the
// totals, the first kept record, the order of neighbouring tiles.  A workgroup scans 1024 tiles (a million records) and first reduces
// everything in front of them itself -- coalesced reads of a few hundred KB out of L2 -- so no workgroup waits for another.
constexpr int TS_THREADS = 1024;
// sums / maxima of this workgroup's 1024 tiles (k_tile_scan combines the groups in front of its own)
__global__ __launch_bounds__(TS_THREADS) void k_tile_partial(int ntiles, const int32_t* tile_cnt, const unsigned long long* tile_ob, const long long* tile_max, TilePart* part) {
    __shared__ int s_cnt[TS_THREADS / 64];
    __shared__ unsigned long long s_ob[TS_THREADS / 64];
    __shared__ long long s_mx[TS_THREADS / 64];
    __shared__ int s_first[TS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x * TS_THREADS + tid;
    const bool in = t < ntiles;
    int cnt = in ? tile_cnt[t] : 0;
    unsigned long long ob = in ? tile_ob[t] : 0;
    long long mx = in ? tile_max[t] : LLONG_MIN;
    int firstt = mx != LLONG_MIN ? t : INT_MAX;
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
        const unsigned long long yo = __shfl_xor(ob, d, 64); ob = yo > ob ? yo : ob;
        const long long ym = __shfl_xor(mx, d, 64); mx = ym > mx ? ym : mx;
        const int yf = __shfl_xor(firstt, d, 64); firstt = yf < firstt ? yf : firstt;
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_ob[wave] = ob; s_mx[wave] = mx; s_first[wave] = firstt; }
    __syncthreads();
    if (tid == 0) {
        TilePart p{0, LLONG_MIN, 0, INT_MAX};
        for (int w = 0; w < TS_THREADS / 64; ++w) { p.cnt += s_cnt[w]; p.ob = s_ob[w] > p.ob ? s_ob[w] : p.ob; p.mx = s_mx[w] > p.mx ? s_mx[w] : p.mx; p.first = s_first[w] < p.first ? s_first[w] : p.first; }
        part[blockIdx.x] = p;
    }
}
__global__ __launch_bounds__(TS_THREADS) void k_tile_scan(int ntiles, const int32_t* tile_cnt, const unsigned long long* tile_ob, const long long* tile_first, const long long* tile_max, const TilePart* part,
                                                         int32_t* tile_rank /* ntiles + 1 */, unsigned long long* tile_obpre, int32_t* sc, const int32_t* tile_K, int32_t* trig) {
    __shared__ int s_cnt[TS_THREADS / 64];
    __shared__ unsigned long long s_ob[TS_THREADS / 64];
    __shared__ long long s_mx[TS_THREADS / 64];
    __shared__ int s_first[TS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cbase = blockIdx.x * TS_THREADS;
    // ---- everything in front of this workgroup's tiles: the groups of 1024 tiles before it (a few hundred at most)
    int cnt = 0, firstt = INT_MAX;  // firstt: first tile with a kept record
    unsigned long long ob = 0;
    long long mx = LLONG_MIN;
    for (int g = tid; g < (int)blockIdx.x; g += TS_THREADS) {
        const TilePart p = part[g];
        cnt += p.cnt;
        ob = p.ob > ob ? p.ob : ob;
        mx = p.mx > mx ? p.mx : mx;
        firstt = p.first < firstt ? p.first : firstt;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
        const unsigned long long yo = __shfl_xor(ob, d, 64); ob = yo > ob ? yo : ob;
        const long long ym = __shfl_xor(mx, d, 64); mx = ym > mx ? ym : mx;
        const int yf = __shfl_xor(firstt, d, 64); firstt = yf < firstt ? yf : firstt;
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_ob[wave] = ob; s_mx[wave] = mx; s_first[wave] = firstt; }
    __syncthreads();
    int p_cnt = 0, p_first = INT_MAX;
    unsigned long long p_ob = 0;
    long long p_mx = LLONG_MIN;
    for (int w = 0; w < TS_THREADS / 64; ++w) { p_cnt += s_cnt[w]; p_ob = s_ob[w] > p_ob ? s_ob[w] : p_ob; p_mx = s_mx[w] > p_mx ? s_mx[w] : p_mx; p_first = s_first[w] < p_first ? s_first[w] : p_first; }
    __syncthreads();
    // ---- the workgroup's own tiles, one per thread: exclusive scans of the count (sum), the pair (max), the largest key (max)
    const int t = cbase + tid;
    const bool in = t < ntiles;
    const int c0 = in ? tile_cnt[t] : 0;
    const unsigned long long o0 = in ? tile_ob[t] : 0;
    const long long m0 = in ? tile_max[t] : LLONG_MIN, f0 = in ? tile_first[t] : LLONG_MIN;
    int x_cnt = c0;
    unsigned long long x_ob = o0;
    long long x_mx = m0;
    for (int d = 1; d < 64; d <<= 1) {
        const int yc = __shfl_up(x_cnt, d, 64);
        const unsigned long long yo = __shfl_up(x_ob, d, 64);
        const long long ym = __shfl_up(x_mx, d, 64);
        if (lane >= d) { x_cnt += yc; x_ob = yo > x_ob ? yo : x_ob; x_mx = ym > x_mx ? ym : x_mx; }
    }
    const unsigned long long km = __ballot(m0 != LLONG_MIN);
    if (lane == 63) { s_cnt[wave] = x_cnt; s_ob[wave] = x_ob; s_mx[wave] = x_mx; }
    if (lane == 0) s_first[wave] = km ? t + __ffsll((long long)km) - 1 : INT_MAX;
    int e_cnt = __shfl_up(x_cnt, 1, 64);
    unsigned long long e_ob = __shfl_up(x_ob, 1, 64);
    long long e_mx = __shfl_up(x_mx, 1, 64);
    if (lane == 0) { e_cnt = 0; e_ob = 0; e_mx = LLONG_MIN; }
    __syncthreads();
    e_cnt += p_cnt; e_ob = p_ob > e_ob ? p_ob : e_ob; e_mx = p_mx > e_mx ? p_mx : e_mx;
    int tot = p_cnt, g_first = p_first;
    unsigned long long tot_ob = p_ob;
    for (int w = 0; w < TS_THREADS / 64; ++w) {
        if (w < wave) { e_cnt += s_cnt[w]; e_ob = s_ob[w] > e_ob ? s_ob[w] : e_ob; e_mx = s_mx[w] > e_mx ? s_mx[w] : e_mx; }
        tot += s_cnt[w]; tot_ob = s_ob[w] > tot_ob ? s_ob[w] : tot_ob;
        if (s_first[w] < g_first) g_first = s_first[w];
    }
    if (in && tile_K) {  // (k_pass1w) cluster triggers of the tiles: the first tile of a run of equal numbers
        const int K = tile_K[t];
        if (K > 0 && (t == 0 || tile_K[t - 1] != K)) { const int v = t << P1_VSHIFT; if (trig[K - 1] > v) atomicMin(&trig[K - 1], v); }
    }
    if (in) {
        tile_rank[t] = e_cnt; tile_obpre[t] = e_ob;
        if (f0 != LLONG_MIN && e_mx > f0) atomicOr(&sc[P1S_FLAGS], P1F_UNSORTED);  // a kept record of an earlier tile lies behind this tile's first one
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        tile_rank[ntiles] = tot;
        sc[P1S_KEPT] = tot;
        const long long key = tot_ob ? (long long)(tot_ob - 1) : LLONG_MIN;  // the running pair over the whole local stream
        sc[P1S_OTHER_LO] = (int32_t)(uint32_t)((unsigned long long)key & 0xffffffffull); sc[P1S_OTHER_HI] = (int32_t)(uint32_t)((unsigned long long)key >> 32);
        if (g_first != INT_MAX) { const long long gf = tile_first[g_first]; sc[P1S_FIRST_REFID] = (int32_t)(gf >> 32); sc[P1S_FIRST_POS] = (int32_t)((uint32_t)((unsigned long long)gf & 0xffffffffull) ^ 0x80000000u); }
    }
}
// cluster triggers: record (tile << P1_VSHIFT | rank in tile) -> kept index
__global__ void k_trig_rank(int ncl, int ntiles, const int32_t* tile_rank, int32_t* trig) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ncl) return;
    const int v = trig[q];
    if (v < (ntiles << P1_VSHIFT)) trig[q] = tile_rank[v >> P1_VSHIFT] + (v & ((1 << P1_VSHIFT) - 1));
}
// The zero-coverage records among the candidates of every tile, with the running pair in front of the tile added (and that of
// earlier shards: `seed`): one wave per tile, the survivors written in stream order from the first slot of the tile's run
// (tile_zcnt2 = how many).  zidx = kept index, zchr / zright = the running pair in front of the record.
__global__ __launch_bounds__(256) void k_zfinal(int ntiles, ClusterView C, long long seed, int RL, const int32_t* tile_rank, const unsigned long long* tile_obpre,
                                               const int32_t* tile_zbase, const int32_t* tile_zcnt, int zcap, const int32_t* zc_v, const int32_t* zc_K, const unsigned long long* zc_ob,
                                               const int32_t* refid_of, const int32_t* pos_of, int32_t* tile_zcnt2, int32_t* zidx, int32_t* zchr, int32_t* zright) {
    // a wave looks at 64 tiles and works, all lanes together, on those that hold candidates (with the one-wave tiles of k_pass1w most hold none)
    const int t0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64, lane = threadIdx.x & 63;
    if (t0 >= ntiles) return;
    const int my_cnt = t0 + lane < ntiles ? tile_zcnt[t0 + lane] : 0;
    if (t0 + lane < ntiles && my_cnt == 0) tile_zcnt2[t0 + lane] = 0;
    constexpr int SOLO = 4;  // a tile with up to that many candidates is settled by its own lane, one candidate after the other
    if (my_cnt > 0 && my_cnt <= SOLO) {
        const int t = t0 + lane, base = tile_zbase[t];
        int out = 0;
        if (base + my_cnt <= zcap) {
            const unsigned long long pre = tile_obpre[t];
            const int rank0 = tile_rank[t];
            int v[SOLO], K[SOLO], rf[SOLO], ps[SOLO];
            unsigned long long ob[SOLO];
#pragma unroll
            for (int e = 0; e < SOLO; ++e) { const int q = base + (e < my_cnt ? e : 0); v[e] = zc_v[q]; K[e] = zc_K[q]; ob[e] = zc_ob[q]; rf[e] = refid_of[q]; ps[e] = pos_of[q]; }  // (all loads up front)
#pragma unroll
            for (int e = 0; e < SOLO; ++e) {
                if (e >= my_cnt) break;
                int oc = 0, orr = 0;
                if (zero_coverage(C, K[e], false, 0, 0, 0, 0, pre > ob[e] ? pre : ob[e], seed, rf[e], ps[e], RL, &oc, &orr)) {
                    zidx[base + out] = rank0 + (v[e] & ((1 << P1_VSHIFT) - 1)); zchr[base + out] = oc; zright[base + out] = orr;
                    ++out;
                }
            }
        }
        tile_zcnt2[t] = out;
    }
    unsigned long long todo = __ballot(my_cnt > SOLO);
    while (todo) {
        const int tl = __ffsll((long long)todo) - 1, t = t0 + tl;
        todo &= todo - 1;
        const int base = tile_zbase[t], cnt = __shfl(my_cnt, tl, 64);
        int out = 0;
        if (base + cnt <= zcap) {
            const unsigned long long pre = tile_obpre[t];
            const int rank0 = tile_rank[t];
            for (int e0 = 0; e0 < cnt; e0 += 64) {
                const int e = e0 + lane;
                bool z = false;
                int v = 0, oc = 0, orr = 0;
                if (e < cnt) {
                    v = zc_v[base + e];
                    const unsigned long long ob = zc_ob[base + e];
                    z = zero_coverage(C, zc_K[base + e], false, 0, 0, 0, 0, pre > ob ? pre : ob, seed, refid_of[base + e], pos_of[base + e], RL, &oc, &orr);
                }
                const unsigned long long m = __ballot(z);
                if (z) {
                    const int slot = base + out + (int)__popcll(m & ((1ull << lane) - 1));
                    zidx[slot] = rank0 + (v & ((1 << P1_VSHIFT) - 1)); zchr[slot] = oc; zright[slot] = orr;
                }
                out += (int)__popcll(m);
            }
        }
        if (lane == 0) tile_zcnt2[t] = out;
    }
}

// the survivors of every tile's run, strung together in stream order (zoff = exclusive scan of tile_zcnt2): what the host needs of the
// zero-coverage lists, instead of the runs with their gaps plus two per-tile arrays to find them (round 5: 7 MB less per pass over PCIe and no
// host loop over 2 * 10^5 tiles)
__global__ void k_zcompact(int ntiles, const int32_t* tile_zbase, const int32_t* tile_zcnt2, const int32_t* zoff, const int32_t* zidx, const int32_t* zchr, const int32_t* zright, int32_t* out /* 3 x nz */, int nz) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const int n = tile_zcnt2[t];
    if (!n) return;
    const int b = tile_zbase[t], o = zoff[t];
    for (int e = 0; e < n; ++e) { out[o + e] = zidx[b + e]; out[nz + o + e] = zchr[b + e]; out[2 * (size_t)nz + o + e] = zright[b + e]; }
}

// Window elements of the segmentation automaton (SegmentGraph.cpp:320-337,668-699) for the kept records with index in [lo, hi) that
// lie in one tile of k_pass1: the host replays only the stretches of the stream that hold a cluster trigger, so only those tiles
// are summarised (round 2 wrote 32 bytes for every kept record of the stream).
__global__ __launch_bounds__(P1_THREADS) void k_summarise_tiles(RecView R, const uint8_t* cls, const uint8_t* keep, const SumItem* items, StreamRec* out) {
    __shared__ int s_w[P1_THREADS / 64];
    const SumItem it = items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = it.rank_base;  // kept records in front of the current 256 records
    for (int i = 0; i < P1_ITEMS; ++i) {
        const int64_t r = it.rec_base + i * P1_THREADS + tid;
        const bool kept = r < R.n && (keep[r] & K_1);
        const unsigned long long m = __ballot(kept);
        if (lane == 0) s_w[wave] = (int)__popcll(m);
        __syncthreads();
        int rank = run + (int)__popcll(m & ((1ull << lane) - 1)), tot = 0;
        for (int w = 0; w < P1_THREADS / 64; ++w) { if (w < wave) rank += s_w[w]; tot += s_w[w]; }
        __syncthreads();
        run += tot;
        if (kept && rank >= it.lo && rank < it.hi) {
            StreamRec s;
            s.refid = R.refid[r]; s.pos = R.pos[r];
            const uint32_t b0 = R.blk_off[r];
            const int nblk = (int)(R.blk_off[r + 1] - b0);
            const uint8_t c = cls[r];
            const int flag = R.flag[r];
            uint8_t fl = 0;
            s.fb_refpos = 0; s.fb_matchref = 0; s.fb_readpos = 0; s.nrest = 0; s.rest_off = 0;
            if (nblk > 0) {
                const int4 q = R.b_pack[b0];
                fl |= SR_HASBLK;
                s.fb_refpos = q.x; s.fb_matchref = q.y; s.fb_readpos = (uint16_t)((uint32_t)q.z & 0xffffu);
            }
            if (c & C_CONC) fl |= SR_CONC;
            if (c & C_PART) fl |= SR_PART;
            if (flag & 0x10) fl |= SR_REV;
            if (flag & 0xC0) fl |= SR_MATE;
            if ((c & C_CONC) && nblk > 1) s.nrest = (uint8_t)(nblk - 1 > 255 ? 255 : nblk - 1);
            s.flags = fl;
            out[it.dst + (rank - it.lo)] = s;
        }
    }
}
// record index of the kept record with rank `target` inside the tile that holds it (the consumed prefix of the stream ends there,
// ledger B12): written to *out
__global__ __launch_bounds__(P1_THREADS) void k_find_rank(int64_t n, const uint8_t* keep, int64_t rec_base, int32_t rank_base, int32_t target, long long* out) {
    __shared__ int s_w[P1_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = rank_base;
    for (int i = 0; i < P1_ITEMS; ++i) {
        const int64_t r = rec_base + i * P1_THREADS + tid;
        const bool kept = r < n && (keep[r] & K_1);
        const unsigned long long m = __ballot(kept);
        if (lane == 0) s_w[wave] = (int)__popcll(m);
        __syncthreads();
        int rank = run + (int)__popcll(m & ((1ull << lane) - 1)), tot = 0;
        for (int w = 0; w < P1_THREADS / 64; ++w) { if (w < wave) rank += s_w[w]; tot += s_w[w]; }
        __syncthreads();
        run += tot;
        if (kept && rank == target) *out = (long long)r;
    }
}

// ------------------------------------------------------------------------------------------------ striped tiles (k_depth2, k_bp2)
// A workgroup of 256 threads takes ST_ITEMS x 256 consecutive records, item i of thread t being record base + i * 256 + t: every
// load is a coalesced one and a wave works on 64 neighbouring records of the sorted stream (they share their node / breakpoints, so
// the wave-combined atomics of the bodies below stay cheap).  Stream order = (item, wave, lane).
// (round 5: one wave per tile of 256 records -- no barrier waits, k_depth2 0.50 -> 0.43 ms at C3)
constexpr int ST_THREADS = 64, ST_ITEMS = 4, ST_TILE = ST_THREADS * ST_ITEMS, ST_SLOTS = ST_ITEMS * (ST_THREADS / 64);
// max-scan of non-negative payloads (0 = identity) over the tile in stream order; v[i] in, EXCLUSIVE prefix inside the tile out;
// returns the tile aggregate.  s_agg: ST_SLOTS words of LDS.
__device__ __forceinline__ unsigned int st_tile_maxscan(unsigned int (&v)[ST_ITEMS], unsigned int* s_agg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int incl[ST_ITEMS];
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const unsigned int x = wave_maxscan_incl_u32(v[i]);
        incl[i] = x;
        if (lane == 63) s_agg[i * (ST_THREADS / 64) + wave] = x;
    }
    __syncthreads();
    unsigned int run = 0, total = 0;
    unsigned int before[ST_ITEMS];
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) before[i] = 0;
#pragma unroll
    for (int s = 0; s < ST_SLOTS; ++s) {
        const unsigned int a = s_agg[s];
#pragma unroll
        for (int i = 0; i < ST_ITEMS; ++i) if (s == i * (ST_THREADS / 64) + wave) before[i] = run;  // (s is a compile-time constant after unrolling; wave is not)
        run = a > run ? a : run;
        total = run;
    }
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const unsigned int e = (unsigned int)dpp_shr1((int)incl[i]);  // (lane 0: 0)
        v[i] = e > before[i] ? e : before[i];
    }
    __syncthreads();
    return total;
}

// ------------------------------------------------------------------------------------------------ K3 fused: depth
// k_early + scan_depth_cursor + k_depth of round 2 in one kernel.  `r_break`: records at or behind it are not consumed (ledger B12).
//
// The sweep cursor of ReadsMain (SegmentGraph.cpp:787-799) in front of a record is the largest "early node" of the first blocks of
// all records before it.  On a sorted stream that maximum is nearly always reached inside the tile -- the early node of a record is
// its home node or, for a first block of <= 3 bases right behind a node boundary, the node in front, and homes ascend with the
// positions -- so the tiles are worked on independently of each other, each assuming that nothing in front of it lies ahead of its
// own first record (FIX == false; it leaves its largest early node and the cursor at its first record).  k_depth_check then forms
// the true maximum in front of every tile from those values and lists the tiles where the assumption fails (a tiny first block at a
// tile's start, or a record whose first kept block lies far behind its position and holds the cursor ahead); for them FIX == true
// takes the contributions back that were made at a wrong cursor and makes them at the right one.  Exact on any input; on the test
// sets a handful of tiles per sample.
struct DepthTiles { unsigned int* agg; unsigned int* first_cur; const int32_t* n_flagged; const int32_t* flagged; const unsigned int* front; int ablate; /* SQUID_D2_ABLATE, timing only */
                    const int32_t* list; const int32_t* n_list; /* (FIX == false) only these tiles: the ones k_pass2w could not settle; null: all */ };
template <bool FIX>
__global__ __launch_bounds__(ST_THREADS) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_depth2(RecView R, NodeView N, const uint8_t* keep, const long long* r_break_p, DepthTiles T, int ntiles,
                                                      int32_t* main_cnt, int32_t* main_sum, int32_t* other_cnt, int32_t* other_sum, int32_t* amb_plus, int32_t* amb_minus, int32_t* flags, int32_t* stripes) {
    __shared__ unsigned int s_agg[ST_SLOTS];
    __shared__ unsigned int s_first, s_tile_flags;
    __shared__ NodeAcc s_acc[2];  // [0] ReadsMain, [1] ReadsOther
  const bool listed = !FIX && T.list != nullptr;  // (uniform)
  for (int work = blockIdx.x; work < (FIX ? *T.n_flagged : (listed ? *T.n_list : ntiles)); work += gridDim.x) {  // (FIX == false without a list: one tile per workgroup)
    const int tile = FIX ? T.flagged[work] : (listed ? T.list[work] : work);
    if (FIX || listed) __syncthreads();
    if (threadIdx.x < 8) { s_acc[threadIdx.x >> 2].key[threadIdx.x & 3] = -1; s_acc[threadIdx.x >> 2].cnt[threadIdx.x & 3] = 0; s_acc[threadIdx.x >> 2].sum[threadIdx.x & 3] = 0; }
    if (threadIdx.x == 0) s_first = 0xffffffffu;
    const long long r_break = *r_break_p;
    const int64_t tbase = (int64_t)tile * ST_TILE;
    int nblk[ST_ITEMS], chr[ST_ITEMS];
    uint32_t b0[ST_ITEMS];
    int4 q0[ST_ITEMS], q1[ST_ITEMS];
    unsigned int ev[ST_ITEMS];  // early node + 1 of the record's first block (0: the record takes no part)
    // ---- phase 1: everything a record needs is requested up front, every load unconditional (indices clamped into the arrays: a load
    // inside a per-lane branch is waited for before the next one is issued); the node the sweep cursor first accepts its first block at
    const bool have_blocks = R.nb > 0;  // (uniform)
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const int64_t r = tbase + i * ST_THREADS + threadIdx.x;
        const bool inr = r < R.n;
        const int64_t rc = inr ? r : R.n - 1;  // (the grid exists only for R.n > 0)
        const uint8_t kp = keep[rc];
        const uint32_t o0 = R.blk_off[rc], o1 = R.blk_off[rc + 1];
        chr[i] = R.refid[rc];
        b0[i] = o0;
        const bool live = inr && (kp & K_1) && r < r_break;
        nblk[i] = live ? (int)(o1 - o0) : 0;
    }
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        if (nblk[i] > 0 && (chr[i] < 0 || chr[i] >= N.n_ref)) { atomicOr(&flags[0], 1); nblk[i] = 0; }
        q0[i] = make_int4(0, 0, 0, 0); q1[i] = q0[i];
        if (have_blocks) {
            q0[i] = R.b_pack[nblk[i] > 0 ? b0[i] : 0];
            q1[i] = R.b_pack[nblk[i] > 1 ? b0[i] + 1 : 0];
        }
    }
    if (!FIX && T.ablate == 1) {  // (timing only: the loads of phase 1 alone)
        int x = 0;
#pragma unroll
        for (int i = 0; i < ST_ITEMS; ++i) x ^= q0[i].x ^ q1[i].y ^ nblk[i] ^ chr[i];
        if (x == 0x12345678) T.agg[tile] = 1;
        continue;
    }
    // Nodes are few next to records: nearly always the whole tile lies inside one node, and then every block of every record of the
    // tile has that node as its home.  It is found once, with uniform (scalar) loads, for a bracket around the tile's first and last
    // record; a block outside the bracket, or within 8 bases of the node's start (the <= 3-base corner of the sweep cursor), takes the
    // per-block lookup.
    bool t_uni = false;
    int t_H = 0, t_np = 0, t_ne = 0;  // the node, its start and end
    long long t_klo = 0, t_khi = 0;
    {
        const int64_t ra = tbase, rb = (tbase + ST_TILE < R.n ? tbase + ST_TILE : R.n) - 1;
        const int ref_a = R.refid[ra], pos_a = R.pos[ra], ref_b = R.refid[rb], pos_b = R.pos[rb];
        if (ref_a >= 0 && ref_a < N.n_ref && ref_b >= 0 && ref_b < N.n_ref && sort_key(ref_a, pos_a) <= sort_key(ref_b, pos_b)) {
            const long long hi_p = (long long)pos_b + 65536;
            const int lo_pos = pos_a < 0 ? 0 : pos_a, hi_pos = hi_p > INT_MAX / 2 ? INT_MAX / 2 : (int)hi_p;
            const int H0 = node_home(N, ref_a, lo_pos), H1 = node_home(N, ref_b, hi_pos);
            if (H0 == H1) {
                const int4 nh = N.pack[H0];
                t_uni = true; t_H = H0; t_np = nh.y; t_ne = nh.y + nh.z; t_klo = sort_key(ref_a, lo_pos > nh.y + 8 ? lo_pos : nh.y + 8); t_khi = sort_key(ref_b, hi_pos);
            }
        }
    }
    auto in_tile_node = [&](int c, int p) { const long long k = sort_key(c, p); return t_uni && k >= t_klo && k <= t_khi; };
    // ---- the whole tile inside one node (round 5; at C3 a thousand nodes meet fifty thousand tiles: nearly every tile): when every block of
    // every record of the tile lies inside the tile's node, more than 8 bases behind its start, the sweep cursor stands on that node for the
    // whole tile, every block is counted for it, and nothing of the general path below -- the cursor scan through LDS, the node tables, the
    // per-block lookups -- has anything to decide.  One test per block, three sums per wave; the general path takes the other tiles.
    if (!FIX) {
        bool simple = t_uni;
        int s_oc = 0, s_os = 0, s_mc = 0, s_ms = 0, s_no = 0;
        bool has = false;
#pragma unroll
        for (int i = 0; i < ST_ITEMS; ++i) {
            const int nb = nblk[i], c = chr[i];
            if (nb > 0) {
                has = true;
                simple = simple && in_tile_node(c, q0[i].x);
                const bool hit = q0[i].x >= t_np - 3 && q0[i].x + q0[i].y <= t_ne + 3;  // the first block against the node the cursor is on (:787-799)
                s_mc += hit ? 1 : 0; s_ms += hit ? q0[i].y : 0;
            }
            if (nb > 1) {
                simple = simple && in_tile_node(c, q1[i].x);
                const bool hit = q1[i].x + q1[i].y <= t_ne + 3;  // ReadsOther: consumed at its home node (:803-826)
                s_oc += hit ? 1 : 0; s_os += hit ? q1[i].y : 0;
                s_no += nb - 1;
            }
            if (nb > 2) {  // (a record of three or more blocks: its further blocks, up to the fifth; longer ones go the general way)
                if (nb > 5) simple = false;
                else
                    for (int k = 2; k < nb; ++k) {
                        const int4 q = R.b_pack[b0[i] + (uint32_t)k];
                        simple = simple && in_tile_node(c, q.x);
                        const bool hit = q.x + q.y <= t_ne + 3;
                        s_oc += hit ? 1 : 0; s_os += hit ? q.y : 0;
                    }
            }
        }
        const unsigned long long bad = __ballot(!simple), any = __ballot(has);
        if (threadIdx.x == 0) s_tile_flags = 0;
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && (bad || any)) atomicOr(&s_tile_flags, (bad ? 2u : 0u) | (any ? 1u : 0u));
        __syncthreads();
        const unsigned int tf = s_tile_flags;
        if (!(tf & 2u)) {  // (uniform over the workgroup)
            if ((tf & 1u) && T.ablate != 2) {
                s_oc = wave_sum_i32(s_oc); s_os = wave_sum_i32(s_os); s_mc = wave_sum_i32(s_mc); s_ms = wave_sum_i32(s_ms); s_no = wave_sum_i32(s_no);
                if ((threadIdx.x & 63) == 0) {
                    const size_t so = (size_t)((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (NODE_STRIPES - 1)) * (size_t)N.n + (size_t)t_H;
                    if (s_mc) { atomicAdd(&main_cnt[so], s_mc); atomicAdd(&main_sum[so], s_ms); }
                    if (s_oc) { atomicAdd(&other_cnt[so], s_oc); atomicAdd(&other_sum[so], s_os); }
                    if (s_no) stripe_add(stripes, s_no);
                }
            }
            if (threadIdx.x == 0) { const unsigned int cur = (tf & 1u) ? (unsigned int)(t_H + 1) : 0u; T.agg[tile] = cur; T.first_cur[tile] = cur; }
            continue;
        }
    }
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        int e = t_H;
        if (nblk[i] > 0 && !in_tile_node(chr[i], q0[i].x)) { int home; e = depth_early(N, chr[i], q0[i].x, q0[i].y, home); }
        ev[i] = nblk[i] > 0 ? (unsigned int)(e + 1) : 0u;
    }
    unsigned int own[ST_ITEMS];
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) own[i] = ev[i];
    const unsigned int tile_agg = st_tile_maxscan(ev, s_agg);  // ev[i] := max over the earlier records of the tile
    int n_other = 0;  // |ReadsOther| of this lane's records
    int fo_cnt = 0, fo_sum = 0, fm_cnt = 0, fm_sum = 0;  // contributions to the tile's own node (t_H): ReadsOther / ReadsMain
    // ---- phase 2: the sums.  ReadsOther first (sorted by (chr,pos) in the reference => consumed at its home node, no cursor)
    if (!FIX) {
    auto ambiguous = [&](int early, int home, int len, bool hit) {
        atomicOr(&flags[0], 2);
        for (int q = early; q < home; ++q) atomicAdd(&amb_plus[q], len);
        if (hit) atomicAdd(&amb_minus[home], len);
    };
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const int c = chr[i], nb = nblk[i];
        const uint32_t o0 = b0[i];
        int geo0 = 0, geo1 = 2;
        if (nb > 1 && !(t_uni && in_tile_node(c, q1[i].x) && nb == 2)) { geo0 = N.fine_off[c]; geo1 = N.fine_off[c + 1]; }
        const int maxb = (int)wave_max_u32((unsigned int)nb);
        // a <=3-base block right behind a node boundary: the reference counts it for whichever node its sweep cursor is on, which
        // depends on the tie order of an unstable sort (SegmentGraph.cpp:781): the bounds are recorded (`ambiguous`).
        // blocks 1..3 of every record are located together (independent load chains overlap), then added
        constexpr int UNR = 3;
        int hk[UNR], ek[UNR], lk[UNR];
        bool hitk[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            hk[j] = 0; ek[j] = 0; lk[j] = 0; hitk[j] = false;
            if (j + 1 < nb) {
                const int4 q = j == 0 ? q1[i] : R.b_pack[o0 + j + 1];
                const int p = q.x;
                lk[j] = q.y;
                if (in_tile_node(c, p)) { hk[j] = t_H; ek[j] = t_H; hitk[j] = p + lk[j] <= t_ne + 3; }
                else {
                    hk[j] = node_home_geo(N, geo0, geo1, p);
                    ek[j] = hk[j];
                    if (lk[j] <= 3) ek[j] = depth_early(N, c, p, lk[j], hk[j]);  // (only a block of <= 3 bases can be accepted before its home node)
                    const int4 nh = N.pack[hk[j]];
                    hitk[j] = p + lk[j] <= nh.y + nh.z + 3;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            if (j + 1 >= maxb) break;  // wave-uniform
            if (j + 1 < nb && ek[j] != hk[j]) ambiguous(ek[j], hk[j], lk[j], hitk[j]);
            // (a tile inside one node: what goes to that node is summed in registers and added once per wave at the end)
            const bool mine = t_uni && hitk[j] && hk[j] == t_H;
            fo_cnt += mine ? 1 : 0; fo_sum += mine ? lk[j] : 0;
            const bool rest = hitk[j] && !mine;
            if (__ballot(rest)) node_add_lds(s_acc[1], other_cnt, other_sum, N.n, rest, hk[j], lk[j]);
        }
        for (int k = UNR + 1; k < maxb; ++k) {  // wave-uniform trip count
            bool hit = false;
            int home = 0, len = 0;
            if (k < nb) {
                const int4 q = R.b_pack[o0 + k];
                const int p = q.x;
                len = q.y;
                int early = depth_early(N, c, p, len, home);
                hit = p + len <= N.pos[home] + N.len[home] + 3;
                if (early != home) ambiguous(early, home, len, hit);
            }
            node_add_lds(s_acc[1], other_cnt, other_sum, N.n, hit, home, len);
        }
        n_other += nb > 1 ? nb - 1 : 0;
    }
    n_other = wave_sum_i32(n_other);
    if ((threadIdx.x & 63) == 0 && n_other) stripe_add(stripes, n_other);
    }  // !FIX
    // ---- ReadsMain: consumed at the prefix-max cursor (SegmentGraph.cpp:787-799)
    const unsigned int front = FIX ? T.front[work] : 0u;
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const int c = chr[i], nb = nblk[i];
        unsigned int w = ev[i] > own[i] ? ev[i] : own[i];  // (own value back in: the cursor at a record's first block is the INCLUSIVE maximum)
        const unsigned int m = w > front ? w : front;
        auto at_cursor = [&](unsigned int mm, bool& hit) {  // the record's first block against the node the cursor is on
            const int cur = (int)mm - 1;
            int4 ncur = make_int4(c, t_np, t_ne - t_np, 0);
            if (!(t_uni && cur == t_H && in_tile_node(c, q0[i].x))) ncur = N.pack[cur];
            const int p = q0[i].x, len = q0[i].y;
            if (ncur.x != c) atomicOr(&flags[0], 1);  // cursor stuck on another chromosome: stream not sorted
            else hit = p >= ncur.y - 3 && p + len <= ncur.y + ncur.z + 3;
        };
        if (!FIX) {
            bool hit = false;
            if (nb > 0) {
                at_cursor(m, hit);
                const unsigned long long lv = __ballot(true);
                if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)lv) - 1)) atomicMin(&s_first, m);  // (the cursor ascends along the stream: the smallest one is the first record's)
            }
            const bool mine = t_uni && hit && (int)m - 1 == t_H;
            fm_cnt += mine ? 1 : 0; fm_sum += mine ? q0[i].y : 0;
            const bool rest = hit && !mine;
            if (__ballot(rest)) node_add_lds(s_acc[0], main_cnt, main_sum, N.n, rest, (int)m - 1, nb > 0 ? q0[i].y : 0);
        } else if (nb > 0 && m != w) {  // made at cursor w by the first pass: taken back; made again at m
            bool hit_w = false, hit_m = false;
            at_cursor(w, hit_w);
            at_cursor(m, hit_m);
            if (hit_w) { atomicAdd(&main_cnt[(int)w - 1], -1); atomicAdd(&main_sum[(int)w - 1], -q0[i].y); }
            if (hit_m) { atomicAdd(&main_cnt[(int)m - 1], 1); atomicAdd(&main_sum[(int)m - 1], q0[i].y); }
        }
    }
    if (!FIX && t_uni) {  // (uniform) the wave's sums for the tile's node: one entry of the workgroup's table
        fo_cnt = wave_sum_i32(fo_cnt); fo_sum = wave_sum_i32(fo_sum); fm_cnt = wave_sum_i32(fm_cnt); fm_sum = wave_sum_i32(fm_sum);
        if ((threadIdx.x & 63) == 0) {
            if (fm_cnt) node_add_bulk(s_acc[0], main_cnt, main_sum, N.n, t_H, fm_cnt, fm_sum);
            if (fo_cnt) node_add_bulk(s_acc[1], other_cnt, other_sum, N.n, t_H, fo_cnt, fo_sum);
        }
    }
    __syncthreads();
    if (!FIX && threadIdx.x == 0) { T.agg[tile] = tile_agg; T.first_cur[tile] = s_first == 0xffffffffu ? 0u : s_first; }
    if (FIX) continue;
    if (threadIdx.x < 8) {  // the workgroup's table -> the striped global accumulators
        const NodeAcc& A = s_acc[threadIdx.x >> 2];
        const int q = threadIdx.x & 3, k = A.key[q];
        if (k >= 0) {
            const size_t so = (size_t)(tile & (NODE_STRIPES - 1)) * (size_t)N.n;
            int32_t *gc = threadIdx.x < 4 ? main_cnt : other_cnt, *gs = threadIdx.x < 4 ? main_sum : other_sum;
            atomicAdd(&gc[so + k], A.cnt[q]); atomicAdd(&gs[so + k], A.sum[q]);
        }
    }
  }
}
// ------------------------------------------------------------------------------------------------ pass 2, one wave per tile (round 5)
// The two kernels that stream the records once the node table exists -- the depth sweep (k_depth2) and the first pass of the edge
// stage (k_edges_near, sq_kernels.hip) -- read the same rows and the same blocks; both decide nearly every record against ONE node,
// the one the whole tile lies in.  k_pass2w reads a record once for both: per tile of 256 records (one wave, four per lane) the node
// bracket with uniform loads, then
//   depth: when every block of every consumed record lies inside the tile's node, more than 8 bases behind its start, the sums of the
//          tile (ReadsMain at the cursor, ReadsOther at home, SegmentGraph.cpp:781-826) and its cursor words; any other tile goes on
//          a list and k_depth2 -- the general sweep -- takes just those;
//   edges: the records that cannot emit an edge (block 0 deep inside its home node, every other element within LocateRead's +-5 of
//          that node, :1213,1601-1686) are dropped, the others go on the work list of k_edges; a record inside the bracket is tested
//          against the tile's node without a lookup of its own; the per-256-record keys of the breakpoint cursor are left as before.
// At C3 this is one read of 3.3 GB where the two kernels read 4.4 GB (PMC), and one launch of ~0.6 ms for 0.50 + 0.49 ms.
struct P2Args {
    const uint8_t* keep; const long long* r_break_p;
    DepthTiles T;
    int32_t *main_cnt, *main_sum, *other_cnt, *other_sum, *flags, *stripes;
    int32_t *depth_list, *depth_n;      // tiles for the general sweep
    unsigned long long* bp_block_key;   // largest (chromosome, fragment start) among the pass-3 records of every 256 records
    uint32_t* list; int32_t* count;     // work list of k_edges
    int all;                            // SQUID_EDGES_ALL: every record takes the full rule set
};
static_assert(ST_THREADS != 64 || ST_TILE == 256, "k_pass2w leaves one cursor word and one breakpoint key per 256 records");
template <int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_pass2w(RecView R, NodeView N, P2Args A) {
    constexpr int IT = 4, TILE = 256;
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int64_t tbase = (int64_t)tile * TILE;
    const unsigned long long ltmask = (1ull << lane) - 1;
    const long long r_break = *A.r_break_p;
    int kp[IT];
    int4 w0[IT], w1[IT], qa[IT], qb[IT];
    bool inr[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int64_t r = tbase + i * 64 + lane;
        inr[i] = r < R.n;
        const int64_t rc = inr[i] ? r : R.n - 1;  // (the grid exists only for R.n > 0)
        kp[i] = A.keep[rc];
        w0[i] = R.r_pack[2 * rc]; w1[i] = R.r_pack[2 * rc + 1];
    }
    const bool have_blocks = R.nb > 0;  // (uniform)
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const uint32_t bo = (uint32_t)w1[i].z, nblk = (uint32_t)w1[i].y >> 16;
        qa[i] = make_int4(0, 0, 0, 0); qb[i] = qa[i];
        if (have_blocks) { qa[i] = R.b_pack[nblk > 0 ? bo : 0u]; qb[i] = R.b_pack[nblk > 1 ? bo + nblk - 1 : (nblk > 0 ? bo : 0u)]; }
    }
    // ---- the tile's node (as k_depth2): found once for a bracket around the tile's first and last record
    bool t_uni = false;
    int t_H = 0, t_c = 0, t_np = 0, t_ne = 0;
    long long t_klo = 0, t_khi = 0;
    {
        const int64_t ra = tbase, rb = (tbase + TILE < R.n ? tbase + TILE : R.n) - 1;
        const int ref_a = R.refid[ra], pos_a = R.pos[ra], ref_b = R.refid[rb], pos_b = R.pos[rb];
        if (ref_a >= 0 && ref_a < N.n_ref && ref_b >= 0 && ref_b < N.n_ref && sort_key(ref_a, pos_a) <= sort_key(ref_b, pos_b)) {
            const long long hi_p = (long long)pos_b + 65536;
            const int lo_pos = pos_a < 0 ? 0 : pos_a, hi_pos = hi_p > INT_MAX / 2 ? INT_MAX / 2 : (int)hi_p;
            const int H0 = node_home(N, ref_a, lo_pos), H1 = node_home(N, ref_b, hi_pos);
            if (H0 == H1) {
                const int4 nh = N.pack[H0];
                t_uni = true; t_H = H0; t_c = nh.x; t_np = nh.y; t_ne = nh.y + nh.z; t_klo = sort_key(ref_a, lo_pos > nh.y + 8 ? lo_pos : nh.y + 8); t_khi = sort_key(ref_b, hi_pos);
            }
        }
    }
    auto in_tile_node = [&](int c, int p) { const long long k = sort_key(c, p); return t_uni && k >= t_klo && k <= t_khi; };
    // ---- depth: the tile inside one node
    bool simple = t_uni, has = false;
    int s_oc = 0, s_os = 0, s_mc = 0, s_ms = 0, s_no = 0;
    // ---- edges
    unsigned long long bkey = 0;
    bool need[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int64_t r = tbase + i * 64 + lane;
        const int rid = w0[i].x, rpos = w0[i].y, mrid = w0[i].z, mp = w0[i].w;
        const int flag = (int)((uint32_t)w1[i].x & 0xffffu), nblk = (int)((uint32_t)w1[i].y >> 16);
        const uint32_t bo = (uint32_t)w1[i].z;
        // depth (SegmentGraph.cpp:781-826): the consumed prefix of the kept stream
        const int nb = (inr[i] && (kp[i] & K_1) && r < r_break) ? nblk : 0;
        if (nb > 0) {
            has = true;
            simple = simple && in_tile_node(rid, qa[i].x);
            const bool hit = qa[i].x >= t_np - 3 && qa[i].x + qa[i].y <= t_ne + 3;  // the first block against the node the cursor is on (:787-799)
            s_mc += hit ? 1 : 0; s_ms += hit ? qa[i].y : 0;
        }
        if (nb > 1) {
            s_no += nb - 1;
            if (nb > 5) simple = false;
            else
                for (int k = 1; k < nb; ++k) {  // ReadsOther: consumed at its home node (:803-826)
                    const int4 q = k == nb - 1 ? qb[i] : R.b_pack[bo + (uint32_t)k];
                    simple = simple && in_tile_node(rid, q.x);
                    const bool hit = q.x + q.y <= t_ne + 3;
                    s_oc += hit ? 1 : 0; s_os += hit ? q.y : 0;
                }
        }
        // edges, pass 1 (k_edges_near): does the record need the full rule set?
        need[i] = false;
        if (inr[i]) {
            const uint8_t cl = (kp[i] & K_P3) ? C_P3 : 0;
            const unsigned long long bk = bp_record_key(cl, flag, rid, rpos, mrid, mp);
            bkey = bk > bkey ? bk : bkey;
            if (kp[i] & K_BUILD) {
                const int nown = nblk;
                const bool first = flag & 0x40, rev = flag & 0x10, stub = !(flag & 0x8) && mrid != -1;
                if (nown + (stub ? 1 : 0) > 0) {
                    bool nd = true;
                    const bool own0 = first ? nown > 0 : !stub;  // is block 0 an own block?  (rec_block0)
                    const int4 q0 = rev ? qb[i] : qa[i];         // the first own block in read-offset order
                    const int c0 = own0 ? rid : mrid, p0 = own0 ? q0.x : mp, e0 = own0 ? q0.x + q0.y : mp + 15;
                    if (c0 >= 0 && c0 < N.n_ref) {
                        int4 nh = make_int4(t_c, t_np, t_ne - t_np, 0);
                        if (!in_tile_node(c0, p0)) nh = N.pack[node_home(N, c0, p0)];
                        const int hp = nh.y, he = hp + nh.z;
                        auto fits = [&](int c, int p, int end) { return c == nh.x && p >= hp - 5 && end <= he + 5; };
                        if (!A.all && e0 > hp + 5 && p0 < he - 5 && e0 <= he + 5) {  // deep inside its node
                            bool ok = !stub || fits(mrid, mp, mp + 15);
                            if (nown > 0) ok = ok && fits(rid, qa[i].x, qa[i].x + qa[i].y) && fits(rid, qb[i].x, qb[i].x + qb[i].y);
                            for (int k = 1; ok && k + 1 < nown; ++k) { const int4 q = R.b_pack[bo + (uint32_t)k]; ok = fits(rid, q.x, q.x + q.y); }
                            nd = !ok;
                        }
                    }
                    need[i] = nd;
                }
            }
        }
    }
    // ---- depth: the sums of a settled tile, or the tile on the list of the general sweep
    const unsigned long long bad = __ballot(!simple), any = __ballot(has);
    if (!bad) {  // (uniform)
        if (any) {
            s_oc = wave_sum_i32(s_oc); s_os = wave_sum_i32(s_os); s_mc = wave_sum_i32(s_mc); s_ms = wave_sum_i32(s_ms); s_no = wave_sum_i32(s_no);
            if (lane == 0) {
                const size_t so = (size_t)(tile & (NODE_STRIPES - 1)) * (size_t)N.n + (size_t)t_H;
                if (s_mc) { atomicAdd(&A.main_cnt[so], s_mc); atomicAdd(&A.main_sum[so], s_ms); }
                if (s_oc) { atomicAdd(&A.other_cnt[so], s_oc); atomicAdd(&A.other_sum[so], s_os); }
                if (s_no) atomicAdd(&A.stripes[tile & (NSTRIPE - 1)], s_no);
            }
        }
        if (lane == 0) { const unsigned int cur = any ? (unsigned int)(t_H + 1) : 0u; A.T.agg[tile] = cur; A.T.first_cur[tile] = cur; }
    } else if (lane == 0) A.depth_list[atomicAdd(A.depth_n, 1)] = tile;
    // ---- edges: the key of the breakpoint cursor, the work list
    bkey = wave_max_u64(bkey);
    if (lane == 0) A.bp_block_key[tile] = bkey;
    unsigned long long nm[IT];
    int total = 0;
#pragma unroll
    for (int i = 0; i < IT; ++i) { nm[i] = __ballot(need[i]); total += (int)__popcll(nm[i]); }
    if (total) {  // (uniform)
        int base = 0;
        if (lane == 0) base = atomicAdd(A.count, total);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            if (need[i]) A.list[base + (int)__popcll(nm[i] & ltmask)] = (uint32_t)(tbase + i * 64 + lane);
            base += (int)__popcll(nm[i]);
        }
    }
}
// the largest early node in front of every tile (exclusive max-scan of the tiles' own maxima; a workgroup reduces what lies in front of
// its 1024 tiles itself) and the list of tiles whose first record's cursor lies below it
// (the maximum of every 1024 tiles first: with the one-wave tiles of round 5 there are 2 * 10^5 of them at C3, and every workgroup of the
// check reading everything in front of it was 2 * 10^7 loads)
__global__ __launch_bounds__(1024) void k_depth_partial(const unsigned int* agg, int ntiles, unsigned int* part) {
    __shared__ unsigned int s_w[16];
    const int t = threadIdx.x, i = blockIdx.x * 1024 + t;
    unsigned int m = i < ntiles ? agg[i] : 0u;
    for (int d = 32; d >= 1; d >>= 1) { const unsigned int o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
    if ((t & 63) == 0) s_w[t >> 6] = m;
    __syncthreads();
    if (t == 0) { unsigned int b = 0; for (int w = 0; w < 16; ++w) b = s_w[w] > b ? s_w[w] : b; part[blockIdx.x] = b; }
}
__global__ __launch_bounds__(1024) void k_depth_check(const unsigned int* agg, const unsigned int* part, const unsigned int* first_cur, int ntiles, int32_t* n_flagged, int32_t* flagged, unsigned int* front, int cap) {
    __shared__ unsigned int s_w[16];
    __shared__ unsigned int s_before;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int base = blockIdx.x * 1024, i = base + t;
    unsigned int m = 0;
    for (int k = t; k < (int)blockIdx.x; k += 1024) { const unsigned int a = part[k]; m = a > m ? a : m; }
    for (int d = 32; d >= 1; d >>= 1) { const unsigned int o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
    if (lane == 0) s_w[wave] = m;
    __syncthreads();
    if (t == 0) { unsigned int b = 0; for (int w = 0; w < 16; ++w) b = s_w[w] > b ? s_w[w] : b; s_before = b; }
    __syncthreads();
    const unsigned int before = s_before;
    unsigned int x = i < ntiles ? agg[i] : 0u;
    for (int d = 1; d < 64; d <<= 1) { const unsigned int y = __shfl_up(x, d, 64); if (lane >= d && y > x) x = y; }
    __syncthreads();
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    unsigned int run = before;
    for (int w = 0; w < wave; ++w) run = s_w[w] > run ? s_w[w] : run;
    unsigned int e = __shfl_up(x, 1, 64);
    if (lane == 0) e = 0;
    e = e > run ? e : run;
    if (i < ntiles) {
        const unsigned int f = first_cur[i];
        if (f && e > f) { const int slot = atomicAdd(n_flagged, 1); if (slot < cap) { flagged[slot] = i; front[slot] = e; } }
    }
}

// ------------------------------------------------------------------------------------------------ K10 fused: breakpoint support
// k_bp_m + scan_bp_cursor + k_bp_count of round 2 in one kernel; nothing is written per record (the walks below recompute the few m
// values they need).  ev_by_M[M] = record of the event with that M, ev_before[M] = cursor bound in front of it; agg[0] = max of m over
// all pass-3 records (INT_MIN: none).
__global__ __launch_bounds__(ST_THREADS) void k_bp2(RecView R, BPView B, const uint8_t* cls, int cur0, const unsigned long long* front_key, int ntiles, int32_t* ev_by_M, int32_t* ev_before, int32_t* diff, int32_t* agg_out) {
    __shared__ unsigned int s_agg[ST_SLOTS];
    const int tile = blockIdx.x;  // tiles are independent: what runs along the stream (the largest m in front of the tile) comes from front_key
    const int64_t tbase = (int64_t)tile * ST_TILE;
    int chr[ST_ITEMS], st[ST_ITEMS], en[ST_ITEMS], m[ST_ITEMS];
    bool live[ST_ITEMS];
    unsigned int mv[ST_ITEMS];
    // (every load unconditional, indices clamped into the arrays: a load inside a per-lane branch is waited for before the next one is issued)
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const int64_t r = tbase + i * ST_THREADS + threadIdx.x;
        const bool inr = r < R.n;
        const int64_t rc = inr ? r : R.n - 1;  // (the grid exists only for R.n > 0)
        const uint8_t c = cls[rc];
        const int flag = R.flag[rc], rid = R.refid[rc], p = R.pos[rc], mrid = R.mrefid[rc], mp = R.mpos[rc];
        en[i] = R.endpos[rc];
        live[i] = inr && (c & C_P3);
        chr[i] = rid;
        st[i] = (!(flag & 0x8) && mrid == rid) ? mp : p;  // SegmentGraph.cpp:3147-3150
    }
    // Breakpoints are few next to records: nearly always none lies anywhere near the tile, and then every lookup of every record of
    // the tile has one and the same answer.  That answer is found once, with uniform (scalar) loads, for a bracket around the tile's
    // first and last record; a record whose three queries do not all lie inside the bracket takes the per-record lookups.
    bool t_uni = false;
    int t_J = 0;
    long long t_klo = 0, t_khi = 0;
    {
        const int64_t ra = tbase, rb = (tbase + ST_TILE < R.n ? tbase + ST_TILE : R.n) - 1;
        const int ref_a = R.refid[ra], pos_a = R.pos[ra], ref_b = R.refid[rb], pos_b = R.pos[rb];
        const int n_ref_b = B.n_ref;
        if (ref_a >= 0 && ref_a < n_ref_b && ref_b >= 0 && ref_b < n_ref_b && sort_key(ref_a, pos_a) <= sort_key(ref_b, pos_b)) {
            const long long lo_p = (long long)pos_a - B.dp - 65536, hi_p = (long long)pos_b + 65536;
            const int lo_pos = lo_p < INT_MIN / 2 ? INT_MIN / 2 : (int)lo_p, hi_pos = hi_p > INT_MAX / 2 ? INT_MAX / 2 : (int)hi_p;
            const int J0 = bp_lower_bound(B, ref_a, lo_pos), J1 = bp_lower_bound(B, ref_b, hi_pos);
            if (J0 == J1) { t_uni = true; t_J = J0; t_klo = sort_key(ref_a, lo_pos); t_khi = sort_key(ref_b, hi_pos); }
        }
    }
    int lo[ST_ITEMS], hi[ST_ITEMS];
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        // #j with c > chr_j || (c == chr_j && st > pos_j + dp)  ==  first j with (chr_j, pos_j) >= (c, st - dp); and the breakpoints the
        // fragment covers: [first at or behind its start, first at or behind its end)
        int mm = t_J, l = t_J, h = t_J;
        if (live[i] && !(t_uni && sort_key(chr[i], st[i] - B.dp) >= t_klo && sort_key(chr[i], en[i]) <= t_khi && st[i] <= en[i])) {
            mm = bp_lower_bound(B, chr[i], st[i] - B.dp); l = bp_lower_bound(B, chr[i], st[i]); h = bp_lower_bound(B, chr[i], en[i]);
        }
        m[i] = live[i] ? mm : INT_MIN;
        mv[i] = live[i] ? (unsigned int)mm + 1u : 0u;
        lo[i] = live[i] ? l : 0; hi[i] = live[i] ? h : 0;
    }
    const unsigned int tile_agg = st_tile_maxscan(mv, s_agg);  // mv[i] := max of m + 1 over the earlier records of the tile
    // the largest m (+ 1) in front of the tile: m is monotone in (chromosome, fragment start), so it is the m of the largest such pair
    // among the earlier pass-3 records (k_edges_near / k_bp_key_prefix); uniform loads
    unsigned int front = 0;
    {
        const unsigned long long fk = front_key[tile];
        if (fk) { const unsigned long long k = fk - 1; front = (unsigned int)bp_lower_bound(B, (int)(k >> 32), (int)((uint32_t)k ^ 0x80000000u) - B.dp) + 1u; }
    }
    if (threadIdx.x == 0 && tile == ntiles - 1) { const unsigned int all = front > tile_agg ? front : tile_agg; agg_out[0] = all ? (int)(all - 1) : INT_MIN; }
#pragma unroll
    for (int i = 0; i < ST_ITEMS; ++i) {
        const int64_t r = tbase + i * ST_THREADS + threadIdx.x;
        const unsigned int pm = mv[i] > front ? mv[i] : front;
        const int Mx = pm ? (int)(pm - 1) : -1;  // max of m over the earlier records (nothing before: below every cursor)
        int before = 0, M = 0;
        if (live[i]) {
            before = Mx > cur0 ? Mx : cur0; M = m[i] > before ? m[i] : before;
            if (M > before) {
                ev_by_M[M] = (int32_t)r; ev_before[M] = before;  // M values of events are distinct and increase along the stream
                if (Mx <= cur0) ev_by_M[0] = (int32_t)r;         // slot 0 (no event has M == 0): the first event of the stream
            }
        }
        // +-1 into the difference array for breakpoints [max(first covered, cursor), first not covered)
        int l = 0, h = 0;
        if (live[i] && before < B.n) { l = lo[i] < M ? M : lo[i]; h = hi[i]; }  // (else: the reference has left its loop, SegmentGraph.cpp:3144-3145)
        const bool on = l < h;
        wave_add(diff, on, l, 1); wave_add(diff, on, h, -1);
    }
}
// one wave per event: APPLY == false records where the cursor catches up, APPLY == true corrects the passed records
template <bool APPLY>
__global__ __launch_bounds__(64) void k_bp_walk2(RecView R, BPView B, const uint8_t* cls, int cur0, const int32_t* ev_by_M, const int32_t* ev_before, int32_t* end_by_M, const int32_t* valid, int32_t* diff, int32_t* lag_end) {
    const int v = blockIdx.x + 1, lane = threadIdx.x;
    const int64_t r0 = ev_by_M[v];
    if (r0 < 0) return;
    if (APPLY && !valid[v]) return;
    int cur = ev_before[v];
    int run = cur;  // max(cursor bound at r0, m of the records walked so far)
    int64_t end = R.n;
    for (int64_t base = r0; base < R.n; base += 64) {
        const int64_t r = base + lane;
        const bool ok = r < R.n && (cls[r] & C_P3);
        int mm = INT_MIN, MM = 0, before_a = 0;
        if (ok) mm = bp_lower_bound(B, R.refid[r], bp_start(R, r) - B.dp);
        {   // exclusive max of mm over the lower lanes, on top of `run`
            int x = mm;
            for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x = y > x ? y : x; }
            int e = __shfl_up(x, 1, 64);
            if (lane == 0) e = INT_MIN;
            before_a = e > run ? e : run;
            const int tot = __shfl(x, 63, 64);
            run = tot > run ? tot : run;
        }
        if (ok) MM = mm > before_a ? mm : before_a;
        int mycur = -1, mybefore = 0, done = -1;
        unsigned long long todo = __ballot(ok);
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int mk = __builtin_amdgcn_readlane(mm, k), Mk = __builtin_amdgcn_readlane(MM, k);
            const int b4 = cur;
            cur += cur < mk ? 1 : 0;
            if (lane == k) { mycur = cur; mybefore = b4; }
            if (cur == Mk) { done = k; break; }
        }
        if (APPLY && mycur >= 0 && (mycur != MM || mybefore != before_a)) {
            bp_contribute<false>(R, B, r, true, before_a, MM, -1, diff);
            bp_contribute<false>(R, B, r, true, mybefore, mycur, 1, diff);
        }
        if (done >= 0) { end = base + done; break; }
    }
    if (!APPLY && lane == 0) end_by_M[v] = (int32_t)(end < R.n ? end : R.n);
    if (APPLY && lane == 0 && end >= R.n) *lag_end = cur;  // the stream ended before the cursor caught up (only the last valid walk can)
}
