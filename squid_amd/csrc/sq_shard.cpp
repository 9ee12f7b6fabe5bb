// Chromosome-sharded runs: what a rank decides from the gathered payloads of an exchange (sq_shard.h has the payloads).  Plain host code
// over small integer tables; tools/shard_emu.cpp drives it without a device.
#include <algorithm>

#include "sq_shard.h"

namespace sq {

// a pass-1 / pass-2 record precedes this shard and its lists are not empty: the nearest earlier rank that has such a record decides
int dedup_mask(const std::vector<XDedup>& p, int me) {
    int mask = 0;
    for (int r = 0; r < me; ++r)
        for (int k = 0; k < 2; ++k) {
            const int32_t has = p[r].last[2 * k], empty = p[r].last[2 * k + 1];
            if (has) { if (empty) mask &= ~(1 << k); else mask |= 1 << k; }
        }
    return mask;
}

void merge_streams(const std::vector<XStream>& p, int me, int64_t own_trigger_last, Shard& sh, std::vector<int32_t>& first_chr) {
    const int W = (int)p.size();
    first_chr.assign(W, -1);
    for (int r = 0; r < W; ++r) if (p[r].kept > 0) first_chr[r] = p[r].first_refid;
    sh.kept_before = 0; sh.kept_total = 0; sh.prior_kept = false; sh.other_seed = INT64_MIN; sh.has_terminal = false;
    for (int r = 0; r < W; ++r) {
        const int64_t K = p[r].kept;
        if (r < me) { sh.kept_before += K; if (K > 0) { sh.prior_kept = true; sh.other_seed = std::max<long long>(sh.other_seed, p[r].other_max); } }
        if (r > me && K > 0 && !sh.has_terminal) { sh.has_terminal = true; sh.term_refid = p[r].first_refid; sh.term_pos = p[r].first_pos; }
        sh.kept_total += K;
    }
    // B12: the consumed prefix ends one record behind the trigger of the globally last cluster
    if (own_trigger_last < 0) sh.n_break_global = std::min<int64_t>(sh.kept_total, 1);  // no discordant cluster at all
    else {
        int64_t T = sh.kept_total, off = 0;
        for (int r = 0; r < W; ++r) { if (p[r].trigger_last >= 0 && p[r].trigger_last < p[r].kept) { T = off + p[r].trigger_last; break; } off += p[r].kept; }
        sh.n_break_global = std::min<int64_t>(sh.kept_total, T + 2);
    }
}

// Seed nodes of all shards, resolved in rank order.  What a shard emits depends on the last node emitted before it: none (A); one on an
// earlier chromosome than the shard's records, then only its existence matters (B); or -- a discordant cluster in front of a
// chromosome's first kept record is processed by the shard before -- one on the shard's own first chromosome, then the shard replays
// again behind exactly that node (C) and everybody exchanges once more.
void resolve_seeds(const std::vector<XSeeds>& p, const std::vector<int32_t>& first_chr, std::vector<Node>& all, int& redo, Node& last) {
    all.clear();
    redo = -1;
    auto append = [&](const std::vector<int32_t>& v, size_t from) { for (size_t i = from; i + 2 < v.size(); i += 3) all.push_back(Node{v[i], v[i + 1], v[i + 2], 0, 0.0}); };
    for (int r = 0; r < (int)p.size(); ++r) {
        const XSeeds& s = p[r];
        if (first_chr[r] < 0) continue;                            // no kept record: nothing replayed, nothing emitted
        if (all.empty() || !s.hasB) { append(s.a, 0); continue; }  // nothing has been emitted before this shard
        last = all.back();
        bool exact_needed = last.chr >= first_chr[r];
        for (int32_t v : s.sens) if (v == last.pos + last.len) exact_needed = true;  // the one comparison without a chromosome test (:623)
        if (!exact_needed) { append(s.b, 0); continue; }
        if (s.hasC && s.seedC[0] == last.chr && s.seedC[1] == last.pos && s.seedC[2] == last.len && s.c.size() >= 3) {
            all.back() = Node{s.c[0], s.c[1], s.c[2], 0, 0.0};  // the shard may have extended the node in front of it
            append(s.c, 3);
            continue;
        }
        redo = r;
        return;
    }
}

// the sum of the per-node accumulators (sup: main support, other support, then |ReadsOther|; sl: main sum, other sum) and the edges
const char* merge_graph(const std::vector<XGraph>& p, int nn, std::vector<int32_t>& sup, std::vector<int64_t>& sl, std::vector<int32_t>& amb_plus, std::vector<int32_t>& amb_minus,
                        bool& tiny, std::vector<Edge>& conc, int64_t& n_raw) {
    static const char* const malformed = "sharded run: malformed graph payload";
    sup.assign(2 * (size_t)nn + 1, 0); sl.assign(2 * (size_t)nn, 0); amb_plus.assign(nn, 0); amb_minus.assign(nn, 0);
    tiny = false; conc.clear();
    int64_t n_other = 0;
    n_raw = 0;
    for (const XGraph& x : p) {
        const int lo = x.lo, hi = x.hi;
        n_other += x.n_other;
        if (x.tiny) tiny = true;
        n_raw += x.n_raw;
        if (lo < 0 || hi > nn || lo > hi || x.keys.size() != x.ws.size()) return malformed;
        for (const auto& v : x.v) if ((int)v.size() != hi - lo) return malformed;
        for (int i = lo; i < hi; ++i) {
            sup[i] += x.v[0][i - lo]; sl[i] += x.v[1][i - lo]; sup[nn + i] += x.v[2][i - lo]; sl[nn + i] += x.v[3][i - lo];
            amb_plus[i] += x.v[4][i - lo]; amb_minus[i] += x.v[5][i - lo];
        }
        for (size_t i = 0; i < x.keys.size(); ++i) {
            const uint64_t k = x.keys[i];
            Edge e;
            e.a = (int32_t)(k >> 32); e.b = (int32_t)((k & 0xffffffffull) >> 2); e.ha = (k >> 1) & 1; e.hb = k & 1; e.w = x.ws[i]; e.gw = 0;
            conc.push_back(e);
        }
    }
    sup[2 * (size_t)nn] = (int32_t)std::min<int64_t>(n_other, INT32_MAX);
    return nullptr;
}

// the cursor (SegmentGraph.cpp:3157) is carried from shard to shard; every shard counted from a guess, this verifies the guesses in rank order
const char* check_cursors(const std::vector<XBpSup>& p, size_t nb, std::vector<int64_t>& total, int& bad, int& truth) {
    total.assign(nb + 1, 0);
    truth = 0; bad = -1;
    for (int r = 0; r < (int)p.size(); ++r) {
        const XBpSup& x = p[r];
        if (x.diff.size() != nb + 1) return "sharded run: malformed breakpoint payload";
        if (!x.has_p3) continue;  // no pass-3 record: the cursor passes through untouched
        // a cursor that arrives `lag` entries behind the assumed position catches up one entry per pass-3 record;
        // every breakpoint it still has to pass lies on an earlier chromosome, so nothing counted here changes as
        // long as it has caught up before the first record that moves it further
        const int64_t lag = (int64_t)x.assumed - truth;
        if (lag < 0 || lag > x.absorb) { bad = r; break; }
        truth = x.has_event ? x.end : (int)std::min<int64_t>(x.assumed, (int64_t)truth + x.n_p3);
        for (size_t i = 0; i <= nb; ++i) total[i] += x.diff[i];
    }
    return nullptr;
}

const char* gather_other(const std::vector<XOther>& p, std::vector<OtherR>& other) {
    other.clear();
    for (const XOther& x : p) {
        if (x.chr.size() != x.pos.size() || x.chr.size() != x.len.size()) return "sharded run: malformed ReadsOther payload";
        for (size_t i = 0; i < x.chr.size(); ++i) other.push_back(OtherR{x.chr[i], x.pos[i], x.len[i]});
    }
    return nullptr;
}

const char* check_tags(const std::vector<std::vector<uint8_t>>& got, int32_t tag) {
    for (const auto& v : got) {
        int32_t t = 0;
        if (v.size() < 4) return "sharded run: short exchange payload";
        std::memcpy(&t, v.data(), 4);
        if (t != tag) return "sharded run: ranks are out of step (payload tag mismatch)";
    }
    return nullptr;
}
int need_exchange(sq_ctx* c) {
    c->x_pending = true; c->x_ready = false;
    return SQ_NEED_EXCHANGE;
}
int take_exchange(sq_ctx* c, int32_t tag) {
    if (!c->x_ready || (int)c->xgot.size() != c->P.world_size) return fail(c, SQ_E_ARG, "sharded run: sq_exchange_unpack has not been called for the pending exchange");
    c->x_ready = false;
    const char* err = check_tags(c->xgot, tag);
    return err ? fail(c, SQ_E_ARG, err) : (int)SQ_OK;
}

void pack_seeds(sq_ctx* c, const GraphBuild& g) {
    auto flat = [](const std::vector<Node>& v) { std::vector<int32_t> f; f.reserve(v.size() * 3); for (const Node& n : v) { f.push_back(n.chr); f.push_back(n.pos); f.push_back(n.len); } return f; };
    XSeeds x;
    x.a = flat(g.seedsA);
    x.hasB = c->shard.prior_kept ? 1 : 0;
    x.b = flat(g.seedsB);
    x.sens = g.sensB;
    x.hasC = g.hasC ? 1 : 0;
    x.seedC[0] = g.seedC.chr; x.seedC[1] = g.seedC.pos; x.seedC[2] = g.seedC.len;
    x.c = flat(g.seedsC);
    x.pack(c->xbuf);
}

}  // namespace sq
