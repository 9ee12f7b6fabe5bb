// K6 / K7: the small-graph stages on the device (SURVEY.md section 8(a) rows a11-a15).  Included at the end of sq_kernels.hip,
// inside namespace sq.  Line references are into the reference's src/SegmentGraph.cpp.
//
//   k_edge_derive          end positions / discordance / chromosome of every edge (helpers of all the filters)
//   k_filter_weight        FilterbyWeight        :1968-2123   one wave per Chr(Ind1): groups never cross it (:2000,2036)
//   k_filter_interleave    FilterbyInterleaving  :2161-2277   one wave per Chr(Ind1)
//   k_fe_nodes / k_fe_edges  GroupConnection / GroupSelect / FilterEdges :2394-2526   node-parallel, then edge-parallel
//   k_cn_* / k_fc_*        CompressNode :2528-2604 (flag, scan, gather), FurtherCompressNode :2693-2892 (one sequential walk,
//                          its per-node edge tests wave-parallel)
//
// The two group filters are order- and state-dependent sweeps (a `HasInspected` bitmap, boxes that grow as members join,
// the index slips of ledger B14): they are reproduced literally.  What a wave adds is width, not reordering: 64 candidates
// are tested against the current box at once, the first one (in the reference's scan order) that breaks the loop or joins the
// group is found with a ballot, its effect is applied, and the test repeats behind it -- a stretch without joins costs one round.
struct GNodes { int n; const int32_t *chr, *pos, *len; };
struct GEdgeView { int m; const int32_t *a, *b, *w; const uint8_t* h; const int32_t *q1, *q2, *chr1; const uint8_t* disc; };

__device__ __forceinline__ bool g_edge_discordant(const GNodes& N, int a, int b, int ha, int hb, int dp, int di) {  // :159-190
    if (N.chr[a] != N.chr[b]) return true;
    if (N.pos[b] - N.pos[a] - N.len[a] > dp && b - a > di) return true;
    return ha != 0 || hb != 1;
}
__global__ void k_edge_derive(GNodes N, int m, const int32_t* ea, const int32_t* eb, const uint8_t* eh, int dp, int di, int32_t* q1, int32_t* q2, int32_t* chr1, uint8_t* disc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int a = ea[i], b = eb[i], ha = eh[i] & 1, hb = (eh[i] >> 1) & 1;
    q1[i] = ha ? N.pos[a] : N.pos[a] + N.len[a];
    q2[i] = hb ? N.pos[b] : N.pos[b] + N.len[b];
    chr1[i] = N.chr[a];
    disc[i] = g_edge_discordant(N, a, b, ha, hb, dp, di) ? 1 : 0;
}
// words that one lane of a wave writes and other lanes of the same wave read later in the same kernel: device-scope relaxed
// accesses (they bypass the CU's vector L1, which is not refreshed by stores)
__device__ __forceinline__ int g_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void g_st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_wave_sum(int v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
__device__ __forceinline__ int g_lower_bound(const int32_t* a, int n, int key) { int lo = 0, hi = n; while (lo < hi) { int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; } return lo; }

struct GBox { int i1lo, i1hi, p1lo, p1hi, i2lo, i2hi, p2lo, p2hi; };

// FilterbyWeight: GroupWeight of every edge.  stamp[] = scratch (group membership of the current seed), seen[] = HasInspected.
// FilterbyWeight, the part that has no order in it (round 5).  A seed that takes the reference's second branch (:2090-2111: Head1 false, Head2
// true, one chromosome) sums the weights of its near-identical neighbours -- a function of the sorted edge list alone: cw[i] for every such
// edge, one thread each.  An edge of that kind that is not discordant either (IsDiscordant false) can never join a group of the first branch
// (:2004,2019,2039,2054 all ask IsDiscordant(j)), so nothing ever looks at its HasInspected flag or touches its GroupWeight again: its group
// weight is final here and the sweep kernel never visits it (kind 0).  kind 1: second-branch seed that IS discordant (far apart on one
// chromosome): the sweep assigns cw[i] when it gets there unvisited; kind 2: first-branch seed.
__global__ void k_filter_weight_conc(GNodes N, GEdgeView E, int DI, int DP, int32_t* cw, int32_t* gw, int32_t* seen, uint8_t* kind) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E.m) return;
    const int sa = E.a[i], sb = E.b[i], sha = E.h[i] & 1, shb = (E.h[i] >> 1) & 1, sq1 = E.q1[i], sq2 = E.q2[i];
    const int chr1 = E.chr1[i], chr2 = N.chr[sb];
    if (sha || !shb || chr1 != chr2) { kind[i] = 2; return; }
    auto alike = [&](int j) {
        const int ha = E.h[j] & 1, hb = (E.h[j] >> 1) & 1, eb = E.b[j];
        int db = eb - sb; if (db < 0) db = -db;
        int d1 = E.q1[j] - sq1; if (d1 < 0) d1 = -d1;
        int d2 = E.q2[j] - sq2; if (d2 < 0) d2 = -d2;
        return sha == ha && shb == hb && N.chr[eb] == chr2 && db <= DI && d1 <= DP && d2 <= DP;
    };
    int sum = E.w[i];
    for (int j = i - 1; j >= 0 && E.chr1[j] == chr1; --j) {
        const int ea = E.a[j];
        if (!(ea >= sa - DI && N.pos[ea] + N.len[ea] >= sq1 - DP)) break;
        if (E.b[j] > sa && alike(j)) sum += E.w[j];
    }
    for (int j = i + 1; j < E.m && E.chr1[j] == chr1; ++j) {
        const int ea = E.a[j];
        if (!(ea <= sa + DI && N.pos[ea] <= sq1 + DP)) break;
        if (ea < sb && alike(j)) sum += E.w[j];
    }
    cw[i] = sum;
    if (E.disc[i]) kind[i] = 1;
    else { kind[i] = 0; gw[i] = sum; seen[i] = 1; }
}
// One wave per WINDOW of the sorted edge list (edge_windows below): a stretch of edges of one Chr(Ind1) with more than Concord_Dist_Pos bases
// between the node of its first edge and the node of the edge in front -- no sweep of either group filter can cross such a gap.
__global__ __launch_bounds__(64) void k_filter_weight(GNodes N, GEdgeView E, const int32_t* win, const uint8_t* kind, const int32_t* cw, int DI, int DP, int32_t* gw, int32_t* seen, int32_t* stamp) {
    const int lane = threadIdx.x;
    const int lo = win[blockIdx.x], hi = win[blockIdx.x + 1];
    if (lo >= hi) return;
    const int chr1 = E.chr1[lo];
    // the seeds, 64 edges at a time: only the ones the sweep has to visit in order (kinds 1 and 2) cost a turn of the loop
    for (int sbase = lo; sbase < hi; sbase += 64) {
      unsigned long long todo = __ballot(sbase + lane < hi && kind[sbase + lane] != 0);
      while (todo) {
        const int i = sbase + __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        if (g_ld(&seen[i])) continue;  // (uniform: written behind a wave_sync below)
        if (kind[i] == 1) {  // second branch (:2090-2111), sums made by k_filter_weight_conc: an assignment, whatever an earlier group left
            if (lane == 0) { g_st(&gw[i], cw[i]); g_st(&seen[i], 1); }
            wave_sync();
            continue;
        }
        const int sa = E.a[i], sb = E.b[i], sha = E.h[i] & 1, shb = (E.h[i] >> 1) & 1, sq1 = E.q1[i], sq2 = E.q2[i];
        const int chr2 = N.chr[sb];
        if (sha || !shb || chr1 != chr2) {
            GBox bx[2];
            bx[0] = GBox{sa, sa, sq1, sq1, sb, sb, sq2, sq2};
            bx[1] = bx[0];
            bool longgroup = false;
            int jmin = i, jmax = i;
            if (lane == 0) g_st(&stamp[i], i + 1);
            // ---- towards smaller indices
            for (int base = i - 1; base >= lo;) {
                const int j = base - lane;
                const bool valid = j >= lo;
                int ea = 0, eb = 0, eq1 = 0, eq2 = 0, o = -1;
                bool dsc = false;
                if (valid) {
                    ea = E.a[j]; eb = E.b[j]; eq1 = E.q1[j]; eq2 = E.q2[j]; dsc = E.disc[j];
                    const int ha = E.h[j] & 1, hb = (E.h[j] >> 1) & 1;
                    o = (ha == sha && hb == shb) ? 0 : ((ha != sha && hb != shb) ? 1 : -1);
                }
                const int m_i1lo = bx[0].i1lo < bx[1].i1lo ? bx[0].i1lo : bx[1].i1lo, m_p1lo = bx[0].p1lo < bx[1].p1lo ? bx[0].p1lo : bx[1].p1lo;
                const bool brk = !valid || sa < m_i1lo - DI || eq1 < m_p1lo - DP;  // s.a, not e.a: ledger B14
                bool join = false;
                if (!brk && o >= 0 && dsc) {
                    const GBox& b = bx[o];
                    join = eb >= b.i2lo - DI && sb <= b.i2hi + DI && eq2 >= b.p2lo - DP && eq2 <= b.p2hi + DP;  // s.b: B14
                }
                const unsigned long long ev = __ballot(brk || join);
                if (!ev) { base -= 64; continue; }
                const int L = __ffsll((long long)ev) - 1;
                const bool is_brk = __shfl((int)brk, L, 64);
                if (is_brk) break;
                const int jo = __shfl(o, L, 64), ja = __shfl(ea, L, 64), jb = __shfl(eb, L, 64), j1 = __shfl(eq1, L, 64), j2 = __shfl(eq2, L, 64), jj = base - L;
                GBox& b = bx[jo];
                if (lane == 0) g_st(&stamp[jj], i + 1);
                jmin = jj;
                b.i1lo = ja < b.i1lo ? ja : b.i1lo; b.p1lo = j1 < b.p1lo ? j1 : b.p1lo;
                b.i2lo = jb < b.i2lo ? jb : b.i2lo; b.i2hi = jb > b.i2hi ? jb : b.i2hi; b.p2lo = j2 < b.p2lo ? j2 : b.p2lo; b.p2hi = j2 > b.p2hi ? j2 : b.p2hi;
                if (b.i1hi >= b.i2lo) longgroup = true;
                base = jj - 1;
            }
            // ---- towards larger indices
            for (int base = i + 1; base < hi;) {
                const int j = base + lane;
                const bool valid = j < hi;
                int ea = 0, eb = 0, eq1 = 0, eq2 = 0, o = -1;
                bool dsc = false;
                if (valid) {
                    ea = E.a[j]; eb = E.b[j]; eq1 = E.q1[j]; eq2 = E.q2[j]; dsc = E.disc[j];
                    const int ha = E.h[j] & 1, hb = (E.h[j] >> 1) & 1;
                    o = (ha == sha && hb == shb) ? 0 : ((ha != sha && hb != shb) ? 1 : -1);
                }
                const int m_i1hi = bx[0].i1hi > bx[1].i1hi ? bx[0].i1hi : bx[1].i1hi, m_p1hi = bx[0].p1hi > bx[1].p1hi ? bx[0].p1hi : bx[1].p1hi;
                const bool brk = !valid || ea > m_i1hi + DI || eq1 > m_p1hi + DP;
                bool join = false;
                if (!brk && o >= 0 && dsc) {
                    const GBox& b = bx[o];
                    const int upper = o == 0 ? eb : sb;  // :2042 vs :2056 (B14)
                    join = eb >= b.i2lo - DI && upper <= b.i2hi + DI && eq2 >= b.p2lo - DP && eq2 <= b.p2hi + DP;
                }
                const unsigned long long ev = __ballot(brk || join);
                if (!ev) { base += 64; continue; }
                const int L = __ffsll((long long)ev) - 1;
                const bool is_brk = __shfl((int)brk, L, 64);
                if (is_brk) break;
                const int jo = __shfl(o, L, 64), ja = __shfl(ea, L, 64), jb = __shfl(eb, L, 64), j1 = __shfl(eq1, L, 64), j2 = __shfl(eq2, L, 64), jj = base + L;
                GBox& b = bx[jo];
                if (lane == 0) g_st(&stamp[jj], i + 1);
                jmax = jj;
                if (jo == 0) { b.i1hi = ja > b.i1hi ? ja : b.i1hi; b.p1hi = j1 > b.p1hi ? j1 : b.p1hi; }
                else { b.i1lo = ja < b.i1lo ? ja : b.i1lo; b.p1lo = j1 < b.p1lo ? j1 : b.p1lo; }  // :2060-2061 updates the lower side
                b.i2lo = jb < b.i2lo ? jb : b.i2lo; b.i2hi = jb > b.i2hi ? jb : b.i2hi; b.p2lo = j2 < b.p2lo ? j2 : b.p2lo; b.p2hi = j2 > b.p2hi ? j2 : b.p2hi;
                if (b.i1hi >= b.i2lo) longgroup = true;
                base = jj + 1;
            }
            wave_sync();
            // ---- group weight: members carry the seed's stamp
            int sum = 0;
            for (int k = jmin + lane; k <= jmax; k += 64) if (g_ld(&stamp[k]) == i + 1) sum += E.w[k];
            sum = g_wave_sum(sum);
            for (int k = jmin + lane; k <= jmax; k += 64)
                if (g_ld(&stamp[k]) == i + 1) { const int g = g_ld(&gw[k]); g_st(&gw[k], longgroup ? E.w[k] : (g > sum ? g : sum)); g_st(&seen[k], 1); }
            wave_sync();
        } else {
            // near-identical concordant neighbours (:2090-2111): no state, every candidate is judged against the seed alone
            // (unreachable since round 5 -- kinds 0 and 1 never get here -- kept as the wave-wide form of k_filter_weight_conc)
            int sum = 0;
            auto alike = [&](int j) {
                const int ha = E.h[j] & 1, hb = (E.h[j] >> 1) & 1, eb = E.b[j];
                int db = eb - sb; if (db < 0) db = -db;
                int d1 = E.q1[j] - sq1; if (d1 < 0) d1 = -d1;
                int d2 = E.q2[j] - sq2; if (d2 < 0) d2 = -d2;
                return sha == ha && shb == hb && N.chr[eb] == chr2 && db <= DI && d1 <= DP && d2 <= DP;
            };
            for (int base = i - 1; base >= lo; base -= 64) {
                const int j = base - lane;
                bool cont = j >= lo, hit = false;
                if (cont) { const int ea = E.a[j]; cont = ea >= sa - DI && N.pos[ea] + N.len[ea] >= sq1 - DP; hit = cont && E.b[j] > sa && alike(j); }
                const unsigned long long stop = __ballot(!cont);
                const int L = stop ? __ffsll((long long)stop) - 1 : 64;
                sum += g_wave_sum(hit && lane < L ? E.w[j] : 0);
                if (stop) break;
            }
            for (int base = i + 1; base < hi; base += 64) {
                const int j = base + lane;
                bool cont = j < hi, hit = false;
                if (cont) { const int ea = E.a[j]; cont = ea <= sa + DI && N.pos[ea] <= sq1 + DP; hit = cont && ea < sb && alike(j); }
                const unsigned long long stop = __ballot(!cont);
                const int L = stop ? __ffsll((long long)stop) - 1 : 64;
                sum += g_wave_sum(hit && lane < L ? E.w[j] : 0);
                if (stop) break;
            }
            if (lane == 0) { g_st(&gw[i], sum + E.w[i]); g_st(&seen[i], 1); }
            wave_sync();
        }
      }
    }
}

// FilterbyInterleaving: keep[] = 0 for the groups it flags (:2161-2277)
// the edges FilterbyInterleaving keeps without looking around (:2168-2172): no seed of a sweep (they may still JOIN one: nothing is written for them here)
__global__ void k_filter_interleave_kind(GNodes N, GEdgeView E, int DI, int DP, uint8_t* kind) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E.m) return;
    const int sa = E.a[i], sb = E.b[i];
    int dpos = N.pos[sa] - N.pos[sb]; if (dpos < 0) dpos = -dpos;
    kind[i] = (sb - sa <= DI || (N.chr[sa] == N.chr[sb] && dpos <= DP)) ? 0 : 1;
}
__global__ __launch_bounds__(64) void k_filter_interleave(GNodes N, GEdgeView E, const int32_t* win, const uint8_t* kind, int DI, int DP, uint8_t* keep, int32_t* seen, int32_t* stamp) {
    const int lane = threadIdx.x;
    const int lo = win[blockIdx.x], hi = win[blockIdx.x + 1];
    if (lo >= hi) return;
    for (int sbase = lo; sbase < hi; sbase += 64) {
      unsigned long long todo = __ballot(sbase + lane < hi && kind[sbase + lane] != 0);
      while (todo) {
        const int i = sbase + __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        if (g_ld(&seen[i])) continue;
        const int sa = E.a[i], sb = E.b[i], sq1 = E.q1[i], sq2 = E.q2[i];
        int p1lo = sq1, p1hi = sq1, i1lo = sa, i1hi = sa, p2lo = sq2, p2hi = sq2, i2lo = sb, i2hi = sb;
        bool longgroup = false, stop = false;
        int jmin = i, jmax = i;
        if (lane == 0) g_st(&stamp[i], i + 1);
        // (a window of 64 edges is loaded ONCE: after a join the lanes behind it are looked at again with the group's new bounds -- the
        // reference's edge-by-edge sweep, a memory round trip per window instead of one per joined edge)
        for (int base = i - 1; base >= lo && !stop; base -= 64) {
            const int j = base - lane;
            const bool valid = j >= lo;
            int ea = 0, eb = 0, eq1 = 0, eq2 = 0;
            if (valid) { ea = E.a[j]; eb = E.b[j]; eq1 = E.q1[j]; eq2 = E.q2[j]; }
            unsigned long long pending = ~0ull;  // the lanes the sweep has not passed yet
            bool left = false;
            for (;;) {
                const bool brk = !valid || sa < i1lo - DI || eq1 < p1lo - DP;  // s.a: B14
                const bool join = !brk && eb >= i2lo - DI && sb <= i2hi + DI && eq2 >= p2lo - DP && eq2 <= p2hi + DP;  // s.b: B14
                const unsigned long long ev = __ballot(brk || join) & pending;
                if (!ev) break;  // nothing (more) in this window: on to the next
                const int L = __ffsll((long long)ev) - 1;
                if (__shfl((int)brk, L, 64)) { left = true; break; }
                const int ja = __shfl(ea, L, 64), jb = __shfl(eb, L, 64), j1 = __shfl(eq1, L, 64), j2 = __shfl(eq2, L, 64), jj = base - L;
                if (lane == 0) g_st(&stamp[jj], i + 1);
                jmin = jj;
                i1lo = ja < i1lo ? ja : i1lo; p1lo = j1 < p1lo ? j1 : p1lo;
                i2lo = jb < i2lo ? jb : i2lo; i2hi = jb > i2hi ? jb : i2hi; p2lo = j2 < p2lo ? j2 : p2lo; p2hi = j2 > p2hi ? j2 : p2hi;
                if (i1hi >= i2lo) { longgroup = true; stop = true; break; }
                pending = L == 63 ? 0ull : (~0ull << (L + 1));
            }
            if (left) break;
        }
        stop = false;
        for (int base = i + 1; base < hi && !stop; base += 64) {  // (runs even after the first loop has left with a long group: it then ends at its first join)
            const int j = base + lane;
            const bool valid = j < hi;
            int ea = 0, eb = 0, eq1 = 0, eq2 = 0;
            if (valid) { ea = E.a[j]; eb = E.b[j]; eq1 = E.q1[j]; eq2 = E.q2[j]; }
            unsigned long long pending = ~0ull;
            bool left = false;
            for (;;) {
                const bool brk = !valid || ea > i1hi + DI || eq1 > p1hi + DP;
                const bool join = !brk && eb >= i2lo - DI && eb <= i2hi + DI && eq2 >= p2lo - DP && eq2 <= p2hi + DP;
                const unsigned long long ev = __ballot(brk || join) & pending;
                if (!ev) break;
                const int L = __ffsll((long long)ev) - 1;
                if (__shfl((int)brk, L, 64)) { left = true; break; }
                const int ja = __shfl(ea, L, 64), jb = __shfl(eb, L, 64), j1 = __shfl(eq1, L, 64), j2 = __shfl(eq2, L, 64), jj = base + L;
                if (lane == 0) g_st(&stamp[jj], i + 1);
                jmax = jj;
                i1hi = ja > i1hi ? ja : i1hi; p1hi = j1 > p1hi ? j1 : p1hi;
                i2lo = jb < i2lo ? jb : i2lo; i2hi = jb > i2hi ? jb : i2hi; p2lo = j2 < p2lo ? j2 : p2lo; p2hi = j2 > p2hi ? j2 : p2hi;
                if (i1hi >= i2lo) { longgroup = true; stop = true; break; }
                pending = L == 63 ? 0ull : (~0ull << (L + 1));
            }
            if (left) break;
        }
        wave_sync();
        if (!longgroup) {
            // partner-index extremes per (group end, Head/Tail): four (min, max) pairs; an empty side keeps (0, 0)
            int lo4[4], hi4[4], has4[4];
            for (int w = 0; w < 4; ++w) { lo4[w] = INT_MAX; hi4[w] = INT_MIN; has4[w] = 0; }
            for (int k = jmin + lane; k <= jmax; k += 64)
                if (g_ld(&stamp[k]) == i + 1) {
                    const int ha = E.h[k] & 1, hb = (E.h[k] >> 1) & 1, ka = E.a[k], kb = E.b[k];
                    const int w1 = ha ? 0 : 1, w2 = hb ? 2 : 3;
                    for (int w = 0; w < 4; ++w) {
                        if (w == w1) { lo4[w] = kb < lo4[w] ? kb : lo4[w]; hi4[w] = kb > hi4[w] ? kb : hi4[w]; has4[w] = 1; }
                        if (w == w2) { lo4[w] = ka < lo4[w] ? ka : lo4[w]; hi4[w] = ka > hi4[w] ? ka : hi4[w]; has4[w] = 1; }
                    }
                }
            for (int w = 0; w < 4; ++w)
                for (int d = 32; d >= 1; d >>= 1) {
                    const int ol = __shfl_xor(lo4[w], d, 64), oh = __shfl_xor(hi4[w], d, 64), oa = __shfl_xor(has4[w], d, 64);
                    lo4[w] = ol < lo4[w] ? ol : lo4[w]; hi4[w] = oh > hi4[w] ? oh : hi4[w]; has4[w] |= oa;
                }
            for (int w = 0; w < 4; ++w) if (!has4[w]) { lo4[w] = 0; hi4[w] = 0; }
            const bool ov1 = (hi4[0] < hi4[1] ? hi4[0] : hi4[1]) >= (lo4[0] > lo4[1] ? lo4[0] : lo4[1]);  // unconditional: stray ';' at :2265 (B14)
            const bool ov2 = has4[2] && has4[3] && (hi4[2] < hi4[3] ? hi4[2] : hi4[3]) >= (lo4[2] > lo4[3] ? lo4[2] : lo4[3]);
            if (ov1 && ov2) for (int k = jmin + lane; k <= jmax; k += 64) if (g_ld(&stamp[k]) == i + 1) keep[k] = 0;
        }
        for (int k = jmin + lane; k <= jmax; k += 64) if (g_ld(&stamp[k]) == i + 1) g_st(&seen[k], 1);
        wave_sync();
      }
    }
}

// ---- FilterEdges.  Incidence lists (UpdateNodeLink, :2894-2909) as a CSR over (node, side): side 0 = Head, 1 = Tail.
__global__ void k_fe_count(int m, const int32_t* ea, const int32_t* eb, const uint8_t* eh, int32_t* cnt /* 2n */) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    atomicAdd(&cnt[2 * ea[i] + ((eh[i] & 1) ? 0 : 1)], 1);
    atomicAdd(&cnt[2 * eb[i] + (((eh[i] >> 1) & 1) ? 0 : 1)], 1);
}
__global__ void k_fe_fill(int m, const int32_t* ea, const int32_t* eb, const uint8_t* eh, const int32_t* off, int32_t* cursor, int32_t* inc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int s1 = 2 * ea[i] + ((eh[i] & 1) ? 0 : 1), s2 = 2 * eb[i] + (((eh[i] >> 1) & 1) ? 0 : 1);
    inc[off[s1] + atomicAdd(&cursor[s1], 1)] = i;
    inc[off[s2] + atomicAdd(&cursor[s2], 1)] = i;
}
// one thread per node: weak edges, neighbour groups per side (GroupConnection), degree limit, GroupSelect.  Nothing here depends
// on the order of a node's incidence list (sums, sorted neighbour lists, sets), so the atomic fill order does not matter.
// conn / lab: scratch in the CSR's geometry (an entry per incidence).
__global__ void k_fe_nodes(GNodes N, int m, const int32_t* ea, const int32_t* eb, const int32_t* ew, const int32_t* egw, const int32_t* off, const int32_t* inc, int DP, int MEW,
                           int MAD, int32_t* conn, int32_t* lab, uint8_t* del, uint8_t* bad) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N.n) return;
    const int h0 = off[2 * v], h1 = off[2 * v + 1], t1 = off[2 * v + 2];
    int hw = 0, tw = 0;
    for (int k = h0; k < h1; ++k) hw += ew[inc[k]];
    for (int k = h1; k < t1; ++k) tw += ew[inc[k]];
    const int sw = hw + tw;
    const double thr = 0.01 * sw;
    auto weak = [&](int e) { return egw[e] <= thr && egw[e] <= MEW; };
    for (int k = h0; k < t1; ++k) if (weak(inc[k])) del[inc[k]] = 1;
    auto gap = [&](int x, int y) { return N.pos[y] - N.pos[x] - N.len[x]; };
    int counts[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        const int b = side ? h1 : h0, e = side ? t1 : h1;
        // neighbours over the strong edges, sorted (insertion sort in place)
        int k = 0;
        for (int q = b; q < e; ++q) {
            const int ed = inc[q];
            if (weak(ed)) continue;
            const int u = ea[ed] != v ? ea[ed] : eb[ed];
            int p = b + k;
            while (p > b && conn[p - 1] > u) { conn[p] = conn[p - 1]; --p; }
            conn[p] = u;
            ++k;
        }
        if (!k) continue;
        int32_t* cn = conn + b; int32_t* lb = lab + b;
        for (int i = 0; i < k; ++i) lb[i] = -1;
        int mind = -1, idx = -1;
        for (int i = 0; i < k; ++i) {
            const int u = cn[i];
            int d = v - u; if (d < 0) d = -d;
            if (N.chr[u] == N.chr[v] && gap(u, v) <= DP && gap(v, u) <= DP && (mind == -1 || mind > d)) { mind = d; idx = i; }
        }
        if (idx != -1) {
            lb[idx] = 0;
            for (int i = idx + 1; i < k; ++i) { if (N.chr[cn[i]] == N.chr[v] && gap(cn[i - 1], cn[i]) <= DP) lb[i] = 0; else break; }
            for (int i = idx - 1; i >= 0; --i) { if (N.chr[cn[i]] == N.chr[v] && gap(cn[i], cn[i + 1]) <= DP) lb[i] = 0; else break; }
        }
        int count = lb[0] == -1 ? 1 : 0;
        if (lb[0] == -1) lb[0] = 1;
        for (int i = 1; i < k; ++i) {
            if (lb[i] != -1) continue;
            if (N.chr[cn[i]] != N.chr[cn[i - 1]] || gap(cn[i - 1], cn[i]) > DP) count++;
            lb[i] = count;
        }
        counts[side] = count;
        // the number of strong neighbours of this side is needed again below: keep it in the slot behind the list when there is
        // room, else recount (k <= e - b always; a full list has no weak edge)
    }
    if (counts[0] + counts[1] >= MAD) { bad[v] = 1; return; }
    for (int side = 0; side < 2; ++side) {
        const int b = side ? h1 : h0, e = side ? t1 : h1, sidew = side ? tw : hw, count = counts[side];
        int k = 0;
        for (int q = b; q < e; ++q) if (!weak(inc[q])) ++k;
        const int32_t* cn = conn + b; const int32_t* lb = lab + b;
        auto labof = [&](int ed) { const int u = ea[ed] != v ? ea[ed] : eb[ed]; int p = 0; while (p < k && cn[p] != u) ++p; return lb[p]; };
        if (count > 1) {  // GroupSelect: keep the heaviest neighbour group (and the local group 0)
            int best = 1;
            long long bestw = -1;
            for (int l = 1; l <= count; ++l) {
                long long lw = 0;
                for (int q = b; q < e; ++q) if (!weak(inc[q]) && labof(inc[q]) == l) lw += ew[inc[q]];
                if (lw > bestw) { bestw = lw; best = l; }
            }
            for (int q = b; q < e; ++q) if (!weak(inc[q])) { const int l = labof(inc[q]); if (l != best && l != 0) del[inc[q]] = 1; }
        } else {
            const double sthr = 0.01 * sidew;
            for (int q = b; q < e; ++q) if (!weak(inc[q]) && egw[inc[q]] < sthr) del[inc[q]] = 1;
        }
    }
}
// one thread per edge: the edge-level tests of FilterEdges (:2503-2524).  ndep = depth | depth_lo | depth_hi (3 x n doubles).
__global__ void k_fe_edges(GNodes N, int m, const int32_t* ea, const int32_t* eb, const uint8_t* eh, const int32_t* ew, const int32_t* egw, const double* ndep, int bounds, int DP, int DI,
                           int MEW, const uint8_t* keep_in, const uint8_t* del, const uint8_t* bad, uint8_t* kept, int32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int a = ea[i], b = eb[i], ha = eh[i] & 1, hb = (eh[i] >> 1) & 1, w = ew[i];
    const bool goodends = !bad[a] && !bad[b];
    int d = N.pos[b] - N.pos[a] - N.len[a]; if (d < 0) d = -d;
    const bool nearby = N.chr[a] == N.chr[b] && d <= DP;
    const bool cond1 = (goodends || nearby) && egw[i] > MEW;
    bool cond2 = true;
    if (cond1 && (b - a > DI || ha != 0 || hb != 1)) {
        // x / 0 = inf deletes, 0 / 0 = NaN keeps (IEEE double division, as in the reference :2512-2516)
        auto ratio_of = [](double c1, double c2) { return (c1 > c2) ? c1 / c2 : c2 / c1; };
        auto passes = [&](double ratio) { return !((w <= MEW + 2 && ratio > 3) || (w > MEW + 2 && ratio > 50)); };
        const double da = ndep[a], db = ndep[b];
        cond2 = passes(ratio_of(da, db));
        if (bounds) {
            const double alo = ndep[(size_t)N.n + a], ahi = ndep[2 * (size_t)N.n + a], blo = ndep[(size_t)N.n + b], bhi = ndep[2 * (size_t)N.n + b];
            if (alo != ahi || blo != bhi) {
                // depths known up to the tie order of the reference's ReadsOther sort: the decision must hold over the whole box
                bool stable = !(alo <= 0 && blo <= 0);
                if (stable) {
                    const double r1 = ratio_of(ahi, blo), r2 = ratio_of(alo, bhi);
                    const double sup = (r1 < r2) ? r2 : r1;          // std::max(r1, r2)
                    const bool overlap = !(alo > bhi || blo > ahi);
                    const double r3 = ratio_of(alo, bhi), r4 = ratio_of(ahi, blo);
                    const double inf = overlap ? 1.0 : ((r4 < r3) ? r4 : r3);  // std::min(r3, r4)
                    stable = passes(sup) == passes(inf) && passes(sup) == cond2;
                }
                if (!stable) atomicOr(&flags[0], 1);
            }
        }
    }
    kept[i] = (keep_in[i] && cond1 && cond2 && !del[i]) ? 1 : 0;
}

// ---- CompressNode (:2528-2604): linked flag -> run heads -> new ids (scan) -> one thread per run head sums its run in index order
__global__ void k_cn_mark(int m, const int32_t* ea, const int32_t* eb, uint8_t* linked) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    linked[ea[i]] = 1; linked[eb[i]] = 1;
}
struct FRunHead {  // 1 for a node that starts an output node: every linked node, and the first node of a run of unlinked ones on one chromosome
    const uint8_t* linked; const int32_t* chr;
    __device__ int operator()(int64_t i) const { return (linked[i] || i == 0 || linked[i - 1] || chr[i - 1] != chr[i]) ? 1 : 0; }
};
__global__ void k_cn_gather(GNodes N, const int32_t* sup, const double* dep, const uint8_t* linked, const int32_t* newid /* exclusive scan of the run-head flag */, int32_t* remap,
                            int32_t* o_chr, int32_t* o_pos, int32_t* o_len, int32_t* o_sup, double* o_dep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N.n) return;
    const bool head = linked[i] || i == 0 || linked[i - 1] || N.chr[i - 1] != N.chr[i];
    const int id = head ? newid[i] : newid[i] - 1;  // (exclusive scan: a non-head belongs to the output node of the head before it)
    remap[i] = id;
    if (!head) return;
    if (linked[i]) { o_chr[id] = N.chr[i]; o_pos[id] = N.pos[i]; o_len[id] = N.len[i]; o_sup[id] = sup[i]; o_dep[id] = dep[i]; return; }
    int j = i, s = 0;
    double dsum = 0.0;
    // same summation order as :2552-2556, every operation rounded on its own: the reference's x86-64 build has no fused multiply-add.
    // (__dadd_rn / __dmul_rn are plain + and * in HIP's headers, and clang contracts a * b + c into an FMA by default in device code:
    // rounds 2-4 believed the intrinsics prevented that; the low-support samples of round 5 -- merged runs of hundreds of nodes --
    // showed AvgDepth one ulp off.  The library is built with -ffp-contract=off, and the pragma says it again where it matters.)
    for (; j < N.n && !linked[j] && N.chr[j] == N.chr[i]; ++j) {
#pragma clang fp contract(off)
        s += sup[j]; dsum = __dadd_rn(dsum, __dmul_rn(dep[j], (double)N.len[j]));
    }
    const int len = N.pos[j - 1] + N.len[j - 1] - N.pos[i];
    o_chr[id] = N.chr[i]; o_pos[id] = N.pos[i]; o_len[id] = len; o_sup[id] = s; o_dep[id] = __ddiv_rn(dsum, (double)len);
}
__global__ void k_relabel(int m, int32_t* ea, int32_t* eb, const int32_t* remap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    ea[i] = remap[ea[i]]; eb[i] = remap[eb[i]];
}

// ---- FurtherCompressNode (:2693-2892): MergeNode[] by a left-to-right walk that carries `cur` and `rightmost` through the node
// list.  The reference walks all nodes in one go; nothing but the running id crosses a chromosome boundary -- a concordant
// edge never leaves its chromosome, so `rightmost` is exactly the first node of the next chromosome when the walk gets
// there, and the chromosome-change rule (:2722) makes that node start a fresh id -- so every chromosome is walked by its
// own wave (workgroup b: the nodes seg[b] .. seg[b + 1]) with ids counted from 0, and k_fc_offsets adds the number of ids of
// the chromosomes in front.  Inside a walk the control flow is uniform; the per-node edge collections and the pairwise
// set comparison (`cross`) are spread over the lanes.  Edge lists of a node: its CSR incidences (Head list first, then Tail,
// each in edge order -- `inc` must be sorted per segment here, see k_fc_sort).  CAP edges per collected list; more => flag.
constexpr int FC_CAP = 256;
__global__ void k_fc_sort(int n2, const int32_t* off, int32_t* inc) {  // per (node, side) segment: ascending edge index (= UpdateNodeLink's order)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n2) return;
    for (int i = off[s] + 1; i < off[s + 1]; ++i) { const int x = inc[i]; int p = i; while (p > off[s] && inc[p - 1] > x) { inc[p] = inc[p - 1]; --p; } inc[p] = x; }
}
// per node: does it have a discordant edge, and the farthest node its concordant edges reach (-1: none)
__global__ void k_fc_summary(int n, const int32_t* ea, const int32_t* eb, const uint8_t* disc, const int32_t* off, const int32_t* inc, int32_t* hasdisc, int32_t* maxfar) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int hd = 0, mf = -1;
    for (int k = off[2 * v]; k < off[2 * v + 2]; ++k) {
        const int e = inc[k];
        if (disc[e]) hd = 1;
        else { const int x = ea[e] > eb[e] ? ea[e] : eb[e]; mf = x > mf ? x : mf; }
    }
    hasdisc[v] = hd; maxfar[v] = mf;
}
struct FcList { int32_t a[FC_CAP], b[FC_CAP]; uint8_t h[FC_CAP]; int n; };
__global__ __launch_bounds__(64) void k_further_compress(GNodes N, int m, const int32_t* ea, const int32_t* eb, const uint8_t* eh, const uint8_t* disc, const int32_t* off, const int32_t* inc, int DI,
                                                         const int32_t* hasdisc, const int32_t* maxfar, int32_t* merge, int32_t* flags, const int32_t* seg) {
    __shared__ FcList s_mine, s_nx;
    __shared__ uint8_t s_am[FC_CAP], s_bm[FC_CAP];
    const int lane = threadIdx.x, lo = seg[blockIdx.x], n = seg[blockIdx.x + 1];  // this chromosome's nodes: [lo, n)
    int cur = 0, rightmost = lo;
    // collect the discordant edges of node v (Head list, then Tail list) into L; `track`: concordant ones move `rightmost`
    // (one incidence per lane: the edge index, then the edge's fields -- two memory round trips per node instead of two per incidence, which
    // is what the walk waits for; the discordant ones keep their list order through a ballot and a count of the lanes below)
    auto discordant_of = [&](int v, FcList& L, bool track) {
        int cnt = L.n, rm = rightmost;
        const int k0 = off[2 * v], k1 = off[2 * v + 2];
        for (int base = k0; base < k1; base += 64) {
            const int k = base + lane;
            const bool valid = k < k1;
            int a = 0, b = 0;
            uint8_t h = 0;
            bool d = false;
            if (valid) { const int e = inc[k]; d = disc[e] != 0; a = ea[e]; b = eb[e]; h = eh[e]; }
            const unsigned long long m = __ballot(valid && d);
            if (valid && d) {
                const int at = cnt + __popcll(m & ((1ull << lane) - 1ull));
                if (at < FC_CAP) { L.a[at] = a; L.b[at] = b; L.h[at] = h; }
            }
            cnt += __popcll(m);
            if (track) {
                int x = (valid && !d) ? (a > b ? a : b) : INT_MIN;
                for (int dd = 32; dd >= 1; dd >>= 1) { const int o = __shfl_xor(x, dd, 64); x = o > x ? o : x; }
                rm = x > rm ? x : rm;
            }
        }
        if (cnt > FC_CAP) { if (lane == 0) atomicOr(&flags[0], 2); cnt = FC_CAP; }
        if (lane == 0) L.n = cnt;
        rightmost = rm;
        wave_sync();
    };
    auto sameheads = [](uint8_t x, uint8_t y) { return x == y; };
    // drop an edge when it continues the previous one's group; `anchor` >= 0 additionally demands the same end at that node
    auto squeeze = [&](FcList& V, int anchor, bool needchr) {
        if (lane == 0 && V.n > 0) {
            int t = 1;
            int pa = V.a[0], pb = V.b[0]; uint8_t ph = V.h[0];
            for (int k = 0; k + 1 < V.n; ++k) {
                const int xa = V.a[k], xb = V.b[k], ya = V.a[k + 1], yb = V.b[k + 1];
                const uint8_t xh = V.h[k], yh = V.h[k + 1];
                int d1 = xa - ya; if (d1 < 0) d1 = -d1;
                int d2 = xb - yb; if (d2 < 0) d2 = -d2;
                bool same = d1 <= DI && d2 <= DI && sameheads(xh, yh) && (!needchr || (N.chr[xa] == N.chr[ya] && N.chr[xb] == N.chr[yb]));
                if (anchor >= 0) same = same && ((xa == anchor && ya == anchor) || (xb == anchor && yb == anchor));
                // (in place: entry t is written from entry k + 1 >= t, and the comparison above has already read entries k and k + 1)
                if (!same) { pa = ya; pb = yb; ph = yh; V.a[t] = pa; V.b[t] = pb; V.h[t] = ph; ++t; }
            }
            V.n = t;
        }
        wave_sync();
    };
    auto cross = [&]() -> bool {  // every edge of `mine` has a partner in `nx` and the other way round
        const int na = s_mine.n, nb = s_nx.n;
        for (int k = lane; k < FC_CAP; k += 64) { s_am[k] = 0; s_bm[k] = 0; }
        wave_sync();
        for (int p = lane; p < na * nb; p += 64) {
            const int k = p / nb, l = p % nb;
            const int aa = s_mine.a[k], ab = s_mine.b[k], ba = s_nx.a[l], bb = s_nx.b[l];
            int d1 = aa - ba; if (d1 < 0) d1 = -d1;
            int d2 = ab - bb; if (d2 < 0) d2 = -d2;
            if (ab > ba && bb > aa && N.chr[aa] == N.chr[ba] && N.chr[ab] == N.chr[bb] && d1 <= DI && d2 <= DI && s_mine.h[k] == s_nx.h[l]) { s_am[k] = 1; s_bm[l] = 1; }
        }
        wave_sync();
        bool ok = true;
        for (int k = lane; k < na; k += 64) if (!s_am[k]) ok = false;
        for (int l = lane; l < nb; l += 64) if (!s_bm[l]) ok = false;
        return !__any(!ok);
    };
    // the next node (at most 19 ahead, below `limit`, on this chromosome -- a wave's nodes are one chromosome's) that has a discordant edge:
    // found in the per-node summary (k_fc_summary), one lane per candidate, instead of collecting the (empty) list of every node on the way
    auto next_with = [&](int i, int limit) {
        int end = i + 20;
        end = n < end ? n : end; end = limit < end ? limit : end; end = end < i + 1 ? i + 1 : end;  // where the reference's loop stops without a find
        const int j = i + 1 + lane;
        const unsigned long long found = __ballot(j < end && hasdisc[j] != 0);
        if (!found) return end;
        const int jj = i + 1 + (__ffsll((long long)found) - 1);
        discordant_of(jj, s_nx, false);
        return jj;
    };
    // Nodes without a discordant edge (nearly all) only move `cur` / `rightmost` and take the running id: 64 of them are loaded at
    // once (one per lane) and walked through lane reads, so the walk waits for memory once per 64 nodes instead of at every node.
    // A range assignment merge[i..j] = cur also updates the lanes of the current chunk that hold those nodes.
    int c_hd = 0, c_mf = -1, c_chg = 0, c_mg = -1, c_base = lo - 64;
    int mprev = -1;
    for (int i = lo; i < n; ++i) {
        if (i >= c_base + 64) {
            wave_sync();
            c_base = i;
            const int v = i + lane;
            c_hd = v < n ? hasdisc[v] : 0; c_mf = v < n ? maxfar[v] : -1;
            c_chg = (v < n && v > lo && N.chr[v] != N.chr[v - 1]) ? 1 : 0;  // (never inside one chromosome; kept as the reference has it)
            c_mg = v < n ? g_ld(&merge[v]) : -1;
        }
        const int t = i - c_base;
        if (!__shfl(c_hd, t, 64)) {
            if (__shfl(c_chg, t, 64) && cur == mprev) ++cur;
            const int mf = __shfl(c_mf, t, 64);
            rightmost = mf > rightmost ? mf : rightmost;
            int mi = __shfl(c_mg, t, 64);
            if (mi == -1) {
                // (i <= rightmost always holds here: every node leaves rightmost >= i + 1 behind)
                mi = cur;
                if (lane == 0) g_st(&merge[i], cur);
                if (i == rightmost) { ++cur; ++rightmost; }
                else if (i > rightmost) atomicOr(&flags[0], 8);  // cannot happen (see above); the host version takes over if it does
            }
            mprev = mi;
            continue;
        }
        int limit = i + 20;  // minDisInd2
        if (lane == 0) { s_mine.n = 0; s_nx.n = 0; }
        wave_sync();
        if (i != lo && N.chr[i] != N.chr[i - 1] && cur == mprev) ++cur;
        discordant_of(i, s_mine, true);
        const int nmine0 = s_mine.n;
        if (nmine0) {
            limit = s_mine.a[0] == i ? s_mine.b[0] : i + 20;
            for (int k = 1; k < nmine0; ++k) { const int t = s_mine.a[k] == i ? s_mine.b[k] : i + 20; limit = t < limit ? t : limit; }
            squeeze(s_mine, i, false);
        }
        const int mi = __shfl(c_mg, t, 64);
        if (mi == -1) {
            if (!nmine0 && i < rightmost) { if (lane == 0) g_st(&merge[i], cur); mprev = cur; }
            else if (!nmine0 && i == rightmost) { if (lane == 0) g_st(&merge[i], cur); mprev = cur; ++cur; ++rightmost; }
            else {
                if (i != lo && cur == mprev) ++cur;
                const int j = next_with(i, limit);
                bool eq = s_nx.n != 0;
                if (eq) { squeeze(s_nx, j, true); eq = cross(); }
                if (!eq) { if (lane == 0) g_st(&merge[i], cur); mprev = cur; ++cur; }
                else { for (int k = i + lane; k <= j; k += 64) g_st(&merge[k], cur); { const int v = c_base + lane; if (v >= i && v <= j) c_mg = cur; } mprev = cur; }
                rightmost = i + 1;
            }
        } else if (nmine0) {
            const int j = next_with(i, limit);
            bool eq = s_nx.n != 0;
            mprev = mi;
            if (eq) { squeeze(s_mine, -1, true); squeeze(s_nx, -1, true); eq = cross(); }
            if (!eq) ++cur;
            else { for (int k = i + lane; k <= j; k += 64) g_st(&merge[k], cur); { const int v = c_base + lane; if (v >= i && v <= j) c_mg = cur; } mprev = cur; }
            rightmost = i + 1;
        } else mprev = mi;
        wave_sync();
    }
}
// ids of the chromosomes in front: a chromosome uses the ids 0 .. merge[its last node] (they never decrease along the walk)
__global__ void k_fc_offsets(int nseg, const int32_t* seg, const int32_t* merge, int32_t* segoff) {
    if (blockIdx.x || threadIdx.x) return;
    int run = 0;
    for (int b = 0; b < nseg; ++b) { segoff[b] = run; run += merge[seg[b + 1] - 1] + 1; }
}
__global__ void k_fc_addoff(int n, int nseg, const int32_t* seg, const int32_t* segoff, int32_t* merge) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nseg;  // last b with seg[b] <= i
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg[mid] <= i) lo = mid; else hi = mid; }
    merge[i] += segoff[lo];
}
// ---- the same walk cut at independent windows (sq_compress_windows_on_device; the bodies, the rule and its reasons: sq_compress_stage.inc):
// k_further_compress above runs unchanged with the window table in place of `seg`, one wave per window
__global__ __launch_bounds__(256) void k_fcw_tile_state(fcw::In G, int64_t ntiles, int32_t* state) {
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per tile
    if (tile >= ntiles) return;
    fcw::tile_state(G, tile, state);
}
__global__ __launch_bounds__(64) void k_fcw_tile_prefix(int64_t ntiles, const int32_t* state, int32_t* front) { fcw::tile_prefix(ntiles, state, front); }
__global__ __launch_bounds__(256) void k_fcw_tile_flags(fcw::In G, int64_t ntiles, const int32_t* front, int32_t* flag) {
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    fcw::tile_flags(G, tile, front, flag);
}
__global__ __launch_bounds__(256) void k_fcw_scatter(int32_t n, const int32_t* flag, const int32_t* winc, int32_t* win) { fcw::scatter(n, flag, winc, win, (int64_t)blockIdx.x * blockDim.x + threadIdx.x); }
struct FFcwIds { const int32_t *win, *merge; __device__ int operator()(int64_t w) const { return fcw::window_ids(win, merge, w); } };
__global__ __launch_bounds__(256) void k_fcw_add(int32_t n, const int32_t* winc, const int32_t* off, int32_t* merge) { fcw::add_offsets(n, winc, off, merge, (int64_t)blockIdx.x * blockDim.x + threadIdx.x); }
__global__ __launch_bounds__(256) void k_fcw_longest(int32_t nwin, const int32_t* win, int32_t* longest) {  // (a timer row, nothing else reads it)
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    int x = w < nwin ? win[w + 1] - win[w] : 0;
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(x, d, 64); x = o > x ? o : x; }
    if ((threadIdx.x & 63) == 0 && x > 0) atomicMax(longest, x);
}
// output nodes of FurtherCompressNode: one per run of equal merge ids; Support / AvgDepth reset (ledger B15)
struct FMergeHead { const int32_t* merge; __device__ int operator()(int64_t i) const { return (i == 0 || merge[i] != merge[i - 1]) ? 1 : 0; } };
__global__ void k_fc_gather(GNodes N, const int32_t* merge, const int32_t* newid, int32_t* remap, int32_t* o_chr, int32_t* o_pos, int32_t* o_len, int32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N.n) return;
    if (i + 1 < N.n && !(merge[i] == merge[i + 1] || merge[i] + 1 == merge[i + 1])) atomicOr(&flags[0], 4);  // the reference asserts (:2862)
    const bool head = i == 0 || merge[i] != merge[i - 1];
    const int id = head ? newid[i] : newid[i] - 1;
    remap[i] = id;
    if (!head) return;
    int j = i;
    while (j + 1 < N.n && merge[j + 1] == merge[i]) ++j;
    o_chr[id] = N.chr[i]; o_pos[id] = N.pos[i]; o_len[id] = N.pos[j] + N.len[j] - N.pos[i];
}

// ================================================================================================ host wrappers (K6 / K7)
// The graph (a few thousand nodes and edges) lives in c->nodes / c->edges between stages -- the stage snapshots of
// sq_graph_view and the chimeric-side code read it there -- so every stage uploads what it needs, runs its kernels and brings
// its result back: one packed copy each way.
namespace {
struct GraphUp {  // device copy of c->nodes / c->edges, carved from the three pools of DeviceRecords
    int n = 0, m = 0;
    int32_t *nchr = nullptr, *npos = nullptr, *nlen = nullptr, *nsup = nullptr, *ea = nullptr, *eb = nullptr, *ew = nullptr, *egw = nullptr, *q1 = nullptr, *q2 = nullptr, *chr1 = nullptr;
    int32_t* iscratch = nullptr;  // 6 * max(n, m) + 2 * n + 8 ints behind the fixed arrays
    double* ndep = nullptr;       // depth | lo | hi, then 1 x n scratch
    uint8_t *eh = nullptr, *disc = nullptr, *bscratch = nullptr;  // bscratch: 4 * max(n, m) bytes
    GNodes nodes() const { return GNodes{n, nchr, npos, nlen}; }
    GEdgeView edges() const { return GEdgeView{m, ea, eb, ew, eh, q1, q2, chr1, disc}; }
};
int graph_upload(sq_ctx* c, GraphUp& g, bool derive) {
    DeviceRecords& D = *c->dev;
    hipStream_t s = c->stream;
    const std::vector<Node>& N = c->nodes;
    const std::vector<Edge>& E = c->edges;
    const size_t n = N.size(), m = E.size(), mx = std::max(n, m) + 1;
    g.n = (int)n; g.m = (int)m;
    const size_t ni = 4 * n + 7 * m + 6 * mx + 2 * n + 16, nd = 4 * n + 4, nb = 2 * m + 4 * mx + 16;
    HIPCHK(D.g_i.reserve(ni)); HIPCHK(D.g_d.reserve(nd)); HIPCHK(D.g_b.reserve(nb));
    std::vector<int32_t> hi(4 * n + 4 * m);
    std::vector<double> hd(3 * n);
    std::vector<uint8_t> hb(m);
    for (size_t i = 0; i < n; ++i) { hi[i] = N[i].chr; hi[n + i] = N[i].pos; hi[2 * n + i] = N[i].len; hi[3 * n + i] = N[i].support; hd[i] = N[i].depth; hd[n + i] = N[i].depth_lo; hd[2 * n + i] = N[i].depth_hi; }
    for (size_t i = 0; i < m; ++i) { hi[4 * n + i] = E[i].a; hi[4 * n + m + i] = E[i].b; hi[4 * n + 2 * m + i] = E[i].w; hi[4 * n + 3 * m + i] = E[i].gw; hb[i] = (uint8_t)((E[i].ha ? 1 : 0) | (E[i].hb ? 2 : 0)); }
    if (!hi.empty()) HIPCHK(hipMemcpyAsync(D.g_i.p, hi.data(), hi.size() * 4, hipMemcpyHostToDevice, s));
    if (n) HIPCHK(hipMemcpyAsync(D.g_d.p, hd.data(), hd.size() * 8, hipMemcpyHostToDevice, s));
    if (m) HIPCHK(hipMemcpyAsync(D.g_b.p, hb.data(), m, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (the staging vectors go out of scope)
    int32_t* p = D.g_i.p;
    g.nchr = p; g.npos = p + n; g.nlen = p + 2 * n; g.nsup = p + 3 * n; p += 4 * n;
    g.ea = p; g.eb = p + m; g.ew = p + 2 * m; g.egw = p + 3 * m; p += 4 * m;
    g.q1 = p; g.q2 = p + m; g.chr1 = p + 2 * m; p += 3 * m;
    g.iscratch = p;
    g.ndep = D.g_d.p;
    g.eh = D.g_b.p; g.disc = D.g_b.p + m; g.bscratch = D.g_b.p + 2 * m;
    if (derive && m) hipLaunchKernelGGL(k_edge_derive, grid_for((int64_t)m, 256), dim3(256), 0, s, g.nodes(), (int)m, g.ea, g.eb, g.eh, c->P.concord_dist_pos, c->P.concord_dist_idx, g.q1, g.q2, g.chr1, g.disc);
    return SQ_OK;
}
}  // namespace

// FilterbyWeight (:1968-2123): GroupWeight by k_filter_weight, then the relaxed threshold (:1969,2117-2119)
// Windows of the sorted edge list for the two group filters (FilterbyWeight :1968-2123, FilterbyInterleaving :2161-2277).  Both grow a group
// from a seed by walking the list down and up, and every walk stops at the first edge whose Ind1-side position lies more than
// Concord_Dist_Pos outside the group's box (:2003,2038,2194,2212; the concordant branch of FilterbyWeight: :2092,2099) or on another
// chromosome.  Every such position is the start or the end of the edge's Ind1 node and the nodes ascend with the edges, so where the node
// of an edge starts more than Concord_Dist_Pos behind the END of the node of the edge in front, no walk gets across, from either side: the
// stretches between such gaps are independent problems -- HasInspected, the boxes and the group weights of one never see an edge of
// another -- and each gets a wave.  (Round 4 gave a wave to every chromosome: 25 waves for 425 k edges on the dense config, 130 + 74 ms.)
// `discordant_only` (FilterbyWeight): only a DISCORDANT edge can join a group there (:2004,2019,2039,2054 ask IsDiscordant(j)) and the edges
// in between never stop a walk earlier than the gap itself does, so the gaps are looked for between consecutive discordant edges -- a sample with
// splice edges every few kilobases still falls into thousands of windows.  (FilterbyInterleaving lets any edge join: all edges count there.)
static int edge_windows(sq_ctx* c, int& nwin, bool discordant_only) {
    DeviceRecords& D = *c->dev;
    const std::vector<Edge>& E = c->edges;
    const std::vector<Node>& N = c->nodes;
    const int m = (int)E.size(), dp = c->P.concord_dist_pos;
    std::vector<int32_t> win;
    win.reserve(1024);
    int prev = -1;  // the edge the gap is measured from: the one in front / the last discordant one on this chromosome
    for (int j = 0; j < m; ++j) {
        const Node& q = N[(size_t)E[(size_t)j].a];
        bool start = j == 0 || N[(size_t)E[(size_t)j - 1].a].chr != q.chr;
        if (start) prev = -1;
        const bool counts = !discordant_only || edge_discordant(c, N, E[(size_t)j]);
        if (!start && counts && prev >= 0) {
            const Node& p = N[(size_t)E[(size_t)prev].a];
            start = (long long)q.pos - ((long long)p.pos + p.len) > (long long)dp;
        }
        if (counts) prev = j;
        if (start) win.push_back(j);
    }
    win.push_back(m);
    nwin = (int)win.size() - 1;
    HIPCHK(D.g_win.reserve(win.size()));
    HIPCHK(hipMemcpyAsync(D.g_win.p, win.data(), win.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (`win` is a local)
    return SQ_OK;
}
int dev_filter_by_weight(sq_ctx* c) {
    std::vector<Edge>& E = c->edges;
    const int m = (int)E.size();
    if (!m) return SQ_OK;
    hipStream_t s = c->stream;
    GraphUp g;
    for (Edge& e : E) e.gw = 0;
    int rc = graph_upload(c, g, true);
    if (rc) return rc;
    int32_t *seen = g.iscratch, *stamp = g.iscratch + m, *cw = g.iscratch + 2 * (size_t)m;
    uint8_t* kind = g.bscratch;
    HIPCHK(hipMemsetAsync(seen, 0, 2 * (size_t)m * 4, s));
    int nwin = 0;
    { const int rw = edge_windows(c, nwin, true); if (rw) return rw; }
    { EvTimer t(c, "k_filter_weight", 0);
      hipLaunchKernelGGL(k_filter_weight_conc, grid_for(m, 256), dim3(256), 0, s, g.nodes(), g.edges(), c->P.concord_dist_idx, c->P.concord_dist_pos, cw, g.egw, seen, kind);
      hipLaunchKernelGGL(k_filter_weight, dim3(nwin), dim3(64), 0, s, g.nodes(), g.edges(), c->dev->g_win.p, kind, cw, c->P.concord_dist_idx, c->P.concord_dist_pos, g.egw, seen, stamp); }
    std::vector<int32_t> gw(m);
    HIPCHK(hipMemcpyAsync(gw.data(), g.egw, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int relaxed = c->P.min_edge_weight - 2;
    size_t k = 0;
    for (int i = 0; i < m; ++i) { E[i].gw = gw[i]; if (gw[i] > relaxed) E[k++] = E[i]; }
    E.resize(k);
    return SQ_OK;
}

// FilterbyInterleaving (:2161-2277)
int dev_filter_by_interleaving(sq_ctx* c, std::vector<uint8_t>& keep) {
    const int m = (int)c->edges.size();
    keep.assign(m, 1);
    if (!m) return SQ_OK;
    hipStream_t s = c->stream;
    GraphUp g;
    int rc = graph_upload(c, g, true);
    if (rc) return rc;
    int32_t *seen = g.iscratch, *stamp = g.iscratch + m;
    uint8_t* dkeep = g.bscratch;
    HIPCHK(hipMemsetAsync(seen, 0, 2 * (size_t)m * 4, s));
    HIPCHK(hipMemsetAsync(dkeep, 1, (size_t)m, s));
    int nwin = 0;
    uint8_t* kind = g.bscratch + m;
    { const int rw = edge_windows(c, nwin, false); if (rw) return rw; }
    { EvTimer t(c, "k_filter_interleave", 0);
      hipLaunchKernelGGL(k_filter_interleave_kind, grid_for(m, 256), dim3(256), 0, s, g.nodes(), g.edges(), c->P.concord_dist_idx, c->P.concord_dist_pos, kind);
      hipLaunchKernelGGL(k_filter_interleave, dim3(nwin), dim3(64), 0, s, g.nodes(), g.edges(), c->dev->g_win.p, kind, c->P.concord_dist_idx, c->P.concord_dist_pos, dkeep, seen, stamp); }
    HIPCHK(hipMemcpyAsync(keep.data(), dkeep, (size_t)m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SQ_OK;
}

// incidence CSR of the uploaded graph: off[2n + 1] and inc[2m] inside the int scratch (behind `skip` ints)
static int graph_csr(sq_ctx* c, const GraphUp& g, int32_t* base, int32_t*& off, int32_t*& inc, bool sorted) {
    DeviceRecords& D = *c->dev;
    hipStream_t s = c->stream;
    const int n = g.n, m = g.m;
    int32_t* cnt = base;                 // 2n
    off = base + 2 * (size_t)n;          // 2n + 1
    int32_t* cursor = off + 2 * (size_t)n + 1;  // 2n
    inc = cursor + 2 * (size_t)n;        // 2m
    HIPCHK(hipMemsetAsync(cnt, 0, (size_t)2 * n * 4, s));
    HIPCHK(hipMemsetAsync(cursor, 0, (size_t)2 * n * 4, s));
    if (m) hipLaunchKernelGGL(k_fe_count, grid_for(m, 256), dim3(256), 0, s, m, g.ea, g.eb, g.eh, cnt);
    HIPCHK((device_scan<OpSum, true>(s, 2 * (int64_t)n, FArr{cnt}, off, D.spine, off + 2 * (size_t)n)));
    if (m) hipLaunchKernelGGL(k_fe_fill, grid_for(m, 256), dim3(256), 0, s, m, g.ea, g.eb, g.eh, off, cursor, inc);
    if (sorted) hipLaunchKernelGGL(k_fc_sort, grid_for(2 * (int64_t)n, 256), dim3(256), 0, s, 2 * n, off, inc);
    return SQ_OK;
}

// GroupConnection / GroupSelect / FilterEdges (:2394-2526)
int dev_filter_edges(sq_ctx* c, const std::vector<uint8_t>& keep) {
    std::vector<Edge>& E = c->edges;
    const int m = (int)E.size(), n = (int)c->nodes.size();
    if (!m) return SQ_OK;
    hipStream_t s = c->stream;
    GraphUp g;
    int rc = graph_upload(c, g, false);
    if (rc) return rc;
    // int scratch: conn[2m] | lab[2m] | CSR (6n + 1 + 2m) ; byte scratch: keep_in[m] | del[m] | bad[n] | kept[m]
    const size_t mx = std::max((size_t)n, (size_t)m) + 1;
    DeviceRecords& D = *c->dev;
    HIPCHK(D.g_x.reserve(4 * (size_t)m + 6 * (size_t)n + 2 * (size_t)m + 16));
    int32_t *conn = D.g_x.p, *lab = conn + 2 * (size_t)m, *csr = lab + 2 * (size_t)m, *off = nullptr, *inc = nullptr;
    (void)mx;
    uint8_t *keep_in = g.bscratch, *del = keep_in + m, *bad = del + m, *kept = bad + n;
    HIPCHK(hipMemcpyAsync(keep_in, keep.data(), (size_t)m, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(del, 0, (size_t)m + (size_t)n, s));
    HIPCHK(hipMemsetAsync(D.flags.p, 0, 4, s));
    {
        EvTimer t(c, "k_filter_edges", 0);
        rc = graph_csr(c, g, csr, off, inc, false);
        if (rc) return rc;
        hipLaunchKernelGGL(k_fe_nodes, grid_for(n, 64), dim3(64), 0, s, g.nodes(), m, g.ea, g.eb, g.ew, g.egw, off, inc, c->P.concord_dist_pos, c->P.min_edge_weight, c->P.max_allowed_degree, conn, lab,
                           del, bad);
        hipLaunchKernelGGL(k_fe_edges, grid_for(m, 256), dim3(256), 0, s, g.nodes(), m, g.ea, g.eb, g.eh, g.ew, g.egw, g.ndep, c->depth_bounds ? 1 : 0, c->P.concord_dist_pos,
                           c->P.concord_dist_idx, c->P.min_edge_weight, keep_in, del, bad, kept, D.flags.p);
    }
    std::vector<uint8_t> hk(m);
    int32_t hf = 0;
    HIPCHK(hipMemcpyAsync(hk.data(), kept, (size_t)m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&hf, D.flags.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hf & 1) c->depth_ambiguous = true;
    size_t k = 0;
    for (int i = 0; i < m; ++i) if (hk[i]) E[k++] = E[i];  // (a subset of a key-sorted list stays sorted: the reference's sort at :2520 is a no-op on it)
    E.resize(k);
    return SQ_OK;
}

// CompressNode (:2528-2604)
int dev_compress_nodes(sq_ctx* c) {
    std::vector<Node>& N = c->nodes;
    std::vector<Edge>& E = c->edges;
    const int n = (int)N.size(), m = (int)E.size();
    if (E.empty()) return fail(c, SQ_E_ASSERT, "0 nodes are connected by edges (the reference asserts at SegmentGraph.cpp:2537)");
    hipStream_t s = c->stream;
    DeviceRecords& D = *c->dev;
    GraphUp g;
    int rc = graph_upload(c, g, false);
    if (rc) return rc;
    uint8_t* linked = g.bscratch;
    int32_t *newid = g.iscratch, *remap = newid + n + 1, *o = remap + n;  // o: chr | pos | len | sup (4 x n)
    double* odep = g.ndep + 3 * (size_t)n;
    int32_t* tot = D.flags.p + 8;
    HIPCHK(hipMemsetAsync(linked, 0, (size_t)n, s));
    {
        EvTimer t(c, "k_compress_nodes", 0);
        hipLaunchKernelGGL(k_cn_mark, grid_for(m, 256), dim3(256), 0, s, m, g.ea, g.eb, linked);
        HIPCHK((device_scan<OpSum, true>(s, n, FRunHead{linked, g.nchr}, newid, D.spine, tot)));
        hipLaunchKernelGGL(k_cn_gather, grid_for(n, 256), dim3(256), 0, s, g.nodes(), g.nsup, g.ndep, linked, newid, remap, o, o + n, o + 2 * (size_t)n, o + 3 * (size_t)n, odep);
        hipLaunchKernelGGL(k_relabel, grid_for(m, 256), dim3(256), 0, s, m, g.ea, g.eb, remap);
    }
    int32_t n2 = 0;
    HIPCHK(hipMemcpyAsync(&n2, tot, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<int32_t> ho(4 * (size_t)n), hab(2 * (size_t)m);
    std::vector<double> hd(n);
    HIPCHK(hipMemcpyAsync(ho.data(), o, ho.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hd.data(), odep, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hab.data(), g.ea, hab.size() * 4, hipMemcpyDeviceToHost, s));  // (ea | eb are adjacent)
    HIPCHK(hipStreamSynchronize(s));
    std::vector<Node> out((size_t)n2);
    for (int i = 0; i < n2; ++i) out[i] = Node{ho[i], ho[n + i], ho[2 * (size_t)n + i], ho[3 * (size_t)n + i], hd[i]};
    for (int i = 0; i < m; ++i) { E[i].a = hab[i]; E[i].b = hab[(size_t)m + i]; }
    N.swap(out);
    return SQ_OK;
}

// The window table of sq_compress_windows_on_device for the n nodes whose summary is in hasdisc / maxfar: win[0 .. nwin] and the inclusive
// sum of the flags winc[0 .. n) inside D.fc_seg, with `extra` ints behind them for the caller.  Waits for the stream once: the walk's grid is nwin.
static int fc_cut_windows(sq_ctx* c, const GraphUp& g, const int32_t* hasdisc, const int32_t* maxfar, size_t extra, int& nwin, int32_t*& win, int32_t*& winc, int32_t*& rest) {
    DeviceRecords& D = *c->dev;
    hipStream_t s = c->stream;
    const int n = g.n;
    const int64_t ntiles = ((int64_t)n + fcw::TILE - 1) / fcw::TILE;
    HIPCHK(D.fc_seg.reserve(3 * (size_t)n + 1 + 4 * (size_t)ntiles + extra + 16));
    win = D.fc_seg.p; winc = win + n + 1;
    int32_t *flag = winc + n, *state = flag + n, *front = state + 2 * ntiles;
    rest = front + 2 * ntiles;
    int32_t* tot = D.flags.p + 9;
    const fcw::In G{n, g.nchr, hasdisc, maxfar};
    const dim3 tgrid((unsigned)((ntiles + 3) / 4));
    {
        EvTimer t(c, "k_fc_cuts", 0);
        hipLaunchKernelGGL(k_fcw_tile_state, tgrid, dim3(256), 0, s, G, ntiles, state);
        hipLaunchKernelGGL(k_fcw_tile_prefix, dim3(1), dim3(64), 0, s, ntiles, state, front);
        hipLaunchKernelGGL(k_fcw_tile_flags, tgrid, dim3(256), 0, s, G, ntiles, front, flag);
        HIPCHK((device_scan<OpSum, false>(s, n, FArr{flag}, winc, D.spine, tot)));
        hipLaunchKernelGGL(k_fcw_scatter, grid_for(n, 256), dim3(256), 0, s, n, flag, winc, win);
    }
    int32_t h = 0;
    HIPCHK(hipMemcpyAsync(&h, tot, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h < 1 || h > n) return fail(c, SQ_E_ARG, "internal: the window table of FurtherCompressNode holds " + std::to_string(h) + " windows for " + std::to_string(n) + " nodes");
    nwin = h;
    return SQ_OK;
}

// (tests: sq_debug_fc_windows) c->nodes / c->edges as they enter FurtherCompressNode -> the window table alone
int dev_fc_windows_debug(sq_ctx* c, std::vector<int32_t>& table) {
    table.clear();
    const int n = (int)c->nodes.size(), m = (int)c->edges.size();
    if (!n) return SQ_OK;
    hipStream_t s = c->stream;
    DeviceRecords& D = *c->dev;
    GraphUp g;
    int rc = graph_upload(c, g, true);
    if (rc) return rc;
    HIPCHK(D.g_x.reserve(6 * (size_t)n + 2 * (size_t)m + 16));
    int32_t *off = nullptr, *inc = nullptr;
    rc = graph_csr(c, g, D.g_x.p, off, inc, true);
    if (rc) return rc;
    int32_t *hasdisc = g.iscratch, *maxfar = hasdisc + n;
    hipLaunchKernelGGL(k_fc_summary, grid_for(n, 256), dim3(256), 0, s, n, g.ea, g.eb, g.disc, off, inc, hasdisc, maxfar);
    int nwin = 0;
    int32_t *win = nullptr, *winc = nullptr, *rest = nullptr;
    rc = fc_cut_windows(c, g, hasdisc, maxfar, 0, nwin, win, winc, rest);
    if (rc) return rc;
    table.resize((size_t)nwin + 1);
    HIPCHK(hipMemcpyAsync(table.data(), win, table.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SQ_OK;
}

// FurtherCompressNode (:2693-2892).  Returns 2 when a per-node edge list exceeded the kernel's capacity (caller: host version).
int dev_further_compress(sq_ctx* c) {
    std::vector<Node>& N = c->nodes;
    std::vector<Edge>& E = c->edges;
    const int n = (int)N.size(), m = (int)E.size();
    hipStream_t s = c->stream;
    DeviceRecords& D = *c->dev;
    GraphUp g;
    int rc = graph_upload(c, g, true);
    if (rc) return rc;
    HIPCHK(D.g_x.reserve(6 * (size_t)n + 2 * (size_t)m + 16));
    int32_t *off = nullptr, *inc = nullptr;
    int32_t *merge = g.iscratch, *newid = merge + n, *remap = newid + n + 1, *o = remap + n;  // o: chr | pos | len
    int32_t* tot = D.flags.p + 8;
    HIPCHK(hipMemsetAsync(merge, 0xff, (size_t)n * 4, s));
    HIPCHK(hipMemsetAsync(D.flags.p, 0, 4, s));
    int fc_nwin = 0;  // (sq_compress_windows_on_device: the windows walked; 0: one walk per chromosome)
    {
        EvTimer t(c, "k_further_compress", 0);
        rc = graph_csr(c, g, D.g_x.p, off, inc, true);
        if (rc) return rc;
        int32_t *hasdisc = o, *maxfar = o + n;  // (the output area is written after the walk)
        hipLaunchKernelGGL(k_fc_summary, grid_for(n, 256), dim3(256), 0, s, n, g.ea, g.eb, g.disc, off, inc, hasdisc, maxfar);
        if (c->fc_windows_on() && n) {
            // one walk per independent window: the cut flags, the window table, the same walk over nwin waves, the ids in front of every window
            int32_t *win = nullptr, *winc = nullptr, *woff = nullptr;
            rc = fc_cut_windows(c, g, hasdisc, maxfar, (size_t)n + 1, fc_nwin, win, winc, woff);
            if (rc) return rc;
            HIPCHK(hipMemsetAsync(D.flags.p + 10, 0, 4, s));
            hipLaunchKernelGGL(k_further_compress, dim3(fc_nwin), dim3(64), 0, s, g.nodes(), m, g.ea, g.eb, g.eh, g.disc, off, inc, c->P.concord_dist_idx, hasdisc, maxfar, merge, D.flags.p, win);
            HIPCHK((device_scan<OpSum, true>(s, fc_nwin, FFcwIds{win, merge}, woff, D.spine, (int32_t*)nullptr)));
            hipLaunchKernelGGL(k_fcw_add, grid_for(n, 256), dim3(256), 0, s, n, winc, woff, merge);
            hipLaunchKernelGGL(k_fcw_longest, grid_for(fc_nwin, 256), dim3(256), 0, s, fc_nwin, win, D.flags.p + 10);
        } else {
        // one walk per chromosome (run of equal Chr in the node list)
        std::vector<int32_t> seg;
        for (int i = 0; i < n; ++i) if (i == 0 || N[i].chr != N[i - 1].chr) seg.push_back(i);
        const int nseg = (int)seg.size();
        seg.push_back(n);
        HIPCHK(D.fc_seg.reserve(2 * seg.size()));
        HIPCHK(hipMemcpyAsync(D.fc_seg.p, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, s));
        int32_t* segoff = D.fc_seg.p + seg.size();
        if (nseg) {
            hipLaunchKernelGGL(k_further_compress, dim3(nseg), dim3(64), 0, s, g.nodes(), m, g.ea, g.eb, g.eh, g.disc, off, inc, c->P.concord_dist_idx, hasdisc, maxfar, merge, D.flags.p, D.fc_seg.p);
            hipLaunchKernelGGL(k_fc_offsets, dim3(1), dim3(64), 0, s, nseg, D.fc_seg.p, merge, segoff);
            hipLaunchKernelGGL(k_fc_addoff, grid_for(n, 256), dim3(256), 0, s, n, nseg, D.fc_seg.p, segoff, merge);
        }
        HIPCHK(hipStreamSynchronize(s));  // (`seg` goes out of scope)
        }
        HIPCHK((device_scan<OpSum, true>(s, n, FMergeHead{merge}, newid, D.spine, tot)));
        hipLaunchKernelGGL(k_fc_gather, grid_for(n, 256), dim3(256), 0, s, g.nodes(), merge, newid, remap, o, o + n, o + 2 * (size_t)n, D.flags.p);
    }
    int32_t n2 = 0, hf = 0, fc_longest = 0;
    HIPCHK(hipMemcpyAsync(&n2, tot, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&hf, D.flags.p, 4, hipMemcpyDeviceToHost, s));
    if (fc_nwin) HIPCHK(hipMemcpyAsync(&fc_longest, D.flags.p + 10, 4, hipMemcpyDeviceToHost, s));
    std::vector<int32_t> ho(3 * (size_t)n), hm(n);
    HIPCHK(hipMemcpyAsync(ho.data(), o, ho.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hm.data(), remap, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (fc_nwin) { c->timer.add("fc_windows", 0.0, 0.0, fc_nwin); c->timer.add("fc_longest_window", 0.0, 0.0, fc_longest); }
    if (hf & (2 | 8)) return 2;
    if (hf & 4) return fail(c, SQ_E_ASSERT, "node merge map is not contiguous (the reference asserts at SegmentGraph.cpp:2862)");
    std::vector<Node> out((size_t)n2);
    for (int i = 0; i < n2; ++i) out[i] = Node{ho[i], ho[n + i], ho[2 * (size_t)n + i], 0, 0.0};  // Support / AvgDepth reset (ledger B15)
    // edges between different output nodes, re-keyed, sorted and summed (as BuildEdges does, :2872-2885)
    std::vector<Edge> raw;
    for (const Edge& e : E) if (hm[e.a] != hm[e.b]) raw.push_back(make_edge(hm[e.a], e.ha, hm[e.b], e.hb, e.w));
    std::sort(raw.begin(), raw.end(), edge_key_less);
    E.clear();
    for (const Edge& e : raw) { if (E.empty() || !edge_key_eq(e, E.back())) E.push_back(e); else E.back().w += e.w; }
    N.swap(out);
    return SQ_OK;
}
