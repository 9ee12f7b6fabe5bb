// The protocol of a chromosome-sharded run (host only, no HIP call): the six payloads the ranks all-gather, each defined once, the
// decisions a rank takes from the gathered payloads as functions of plain tables (also tools/shard_emu.cpp), and the state of
// sq_build_graph / sq_call_sv that survives an exchange.  The pipeline that calls these is sq_build.cpp.
#pragma once
#include "sq_internal.h"

namespace sq {

// ---- the wire: little-endian PODs appended to a byte vector; a vector is an int64 count followed by its elements
struct Packer {
    std::vector<uint8_t>& b;
    explicit Packer(std::vector<uint8_t>& buf) : b(buf) { b.clear(); }
    template <class T> void put(const T& v) { const uint8_t* p = (const uint8_t*)&v; b.insert(b.end(), p, p + sizeof(T)); }
    template <class T> void put_vec(const std::vector<T>& v) { put<int64_t>((int64_t)v.size()); const uint8_t* p = (const uint8_t*)v.data(); b.insert(b.end(), p, p + v.size() * sizeof(T)); }
    template <class T> void operator()(T& v) { put<T>(v); }
    template <class T> void operator()(std::vector<T>& v) { put_vec(v); }
};
struct Unpacker {
    const std::vector<uint8_t>& b; size_t at = 0; bool ok = true;
    explicit Unpacker(const std::vector<uint8_t>& buf) : b(buf) {}
    template <class T> T get() { T v{}; if (!ok || sizeof(T) > b.size() - at) { ok = false; return v; } std::memcpy(&v, b.data() + at, sizeof(T)); at += sizeof(T); return v; }
    template <class T> void get_vec(std::vector<T>& v) {
        const int64_t n = get<int64_t>();
        if (!ok || n < 0 || (uint64_t)n > (b.size() - at) / sizeof(T)) { ok = false; v.clear(); return; }  // (a count, not a product that can wrap)
        v.resize((size_t)n);
        if (n) std::memcpy(v.data(), b.data() + at, (size_t)n * sizeof(T));
        at += (size_t)n * sizeof(T);
    }
    template <class T> void operator()(T& v) { v = get<T>(); }
    template <class T> void operator()(std::vector<T>& v) { get_vec(v); }
};
enum : int32_t { X_DEDUP = 0x51a0, X_STREAM, X_SEEDS, X_GRAPH, X_BPSUP, X_OTHER };  // payload tags (a mismatch means the ranks are out of step)

// A payload lists its fields once (fields), the tag first; pack and unpack walk that list
template <class P, int32_t TAG> struct Payload {
    int32_t tag = TAG;
    void pack(std::vector<uint8_t>& buf) const { Packer pk(buf); const_cast<P*>(static_cast<const P*>(this))->fields(pk); }
    bool unpack(const std::vector<uint8_t>& buf) { Unpacker u(buf); static_cast<P*>(this)->fields(u); return u.ok && tag == TAG; }
};
// exchange 1: what the last passing records of the shard look like to ReadRec_t::Equal -- (has, its lists empty) of pass 1 and of pass 2
struct XDedup : Payload<XDedup, X_DEDUP> {
    int32_t last[4] = {0, 0, 0, 0};
    template <class Ar> void fields(Ar& ar) { ar(tag); for (int32_t& x : last) ar(x); }
};
// exchange 2: size, first record, running other-pair maximum and last-cluster trigger of the local stream
struct XStream : Payload<XStream, X_STREAM> {
    int64_t kept = 0;
    int32_t first_refid = 0, first_pos = 0;
    int64_t other_max = INT64_MIN, trigger_last = 0;
    template <class Ar> void fields(Ar& ar) { ar(tag); ar(kept); ar(first_refid); ar(first_pos); ar(other_max); ar(trigger_last); }
};
// exchange 3: the shard's seed nodes (chr, pos, len each) under the three possible pasts, see resolve_seeds
struct XSeeds : Payload<XSeeds, X_SEEDS> {
    std::vector<int32_t> a;
    int32_t hasB = 0;
    std::vector<int32_t> b, sens;
    int32_t hasC = 0, seedC[3] = {0, 0, 0};
    std::vector<int32_t> c;
    template <class Ar> void fields(Ar& ar) { ar(tag); ar(a); ar(hasB); ar(b); ar(sens); ar(hasC); for (int32_t& x : seedC) ar(x); ar(c); }
};
// exchange 4 (the data exchange): per-node depth accumulators of the own nodes [lo, hi) and the locally reduced edges
struct XGraph : Payload<XGraph, X_GRAPH> {
    int32_t lo = 0, hi = 0;
    int64_t n_other = 0;  // |ReadsOther| of this shard
    int32_t tiny = 0;
    std::vector<int32_t> v[6];  // main support, main sum, other support, other sum, amb_plus, amb_minus
    std::vector<uint64_t> keys;
    std::vector<int32_t> ws;
    int64_t n_raw = 0;
    template <class Ar> void fields(Ar& ar) { ar(tag); ar(lo); ar(hi); ar(n_other); ar(tiny); for (auto& x : v) ar(x); ar(keys); ar(ws); ar(n_raw); }
};
// exchange of sq_call_sv: the shard's difference array and what the next shard needs to know about the breakpoint cursor
struct XBpSup : Payload<XBpSup, X_BPSUP> {
    int32_t assumed = 0, end = 0, has_p3 = 0, has_event = 0;
    int64_t n_p3 = 0, absorb = 0;
    std::vector<int32_t> diff;
    template <class Ar> void fields(Ar& ar) { ar(tag); ar(assumed); ar(end); ar(has_p3); ar(has_event); ar(n_p3); ar(absorb); ar(diff); }
};
// exchange 5 (exact depth sweep only): the shard's ReadsOther list in stream order
struct XOther : Payload<XOther, X_OTHER> {
    std::vector<int32_t> chr, pos, len;
    template <class Ar> void fields(Ar& ar) { ar(tag); ar(chr); ar(pos); ar(len); }
};
template <class P> bool unpack_all(const std::vector<std::vector<uint8_t>>& got, std::vector<P>& out) {
    out.assign(got.size(), P());
    for (size_t r = 0; r < got.size(); ++r) if (!out[r].unpack(got[r])) return false;
    return true;
}

// ---- the decisions: payloads by rank in, a value or an error text (null: none) out
struct OtherR { int32_t chr, pos, len; };  // one ReadsOther block
int dedup_mask(const std::vector<XDedup>& p, int me);
void merge_streams(const std::vector<XStream>& p, int me, int64_t own_trigger_last, Shard& sh, std::vector<int32_t>& first_chr);
// redo (-1: none): the rank that has to replay again behind exactly `last`, the node emitted in front of it; `all` is complete only without one
void resolve_seeds(const std::vector<XSeeds>& p, const std::vector<int32_t>& first_chr, std::vector<Node>& all, int& redo, Node& last);
const char* merge_graph(const std::vector<XGraph>& p, int nn, std::vector<int32_t>& sup, std::vector<int64_t>& sl, std::vector<int32_t>& amb_plus, std::vector<int32_t>& amb_minus,
                        bool& tiny, std::vector<Edge>& conc, int64_t& n_raw);
// bad (-1: none): the rank that started from a wrong cursor and recounts from `truth`; total: the summed difference arrays, nb + 1 entries
const char* check_cursors(const std::vector<XBpSup>& p, size_t nb, std::vector<int64_t>& total, int& bad, int& truth);
const char* gather_other(const std::vector<XOther>& p, std::vector<OtherR>& other);  // the lists in rank order: the unsharded stream order

// ---- the exchange as the pipeline sees it
const char* check_tags(const std::vector<std::vector<uint8_t>>& got, int32_t tag);
int need_exchange(sq_ctx* c);              // c->xbuf is packed: SQ_NEED_EXCHANGE
int take_exchange(sq_ctx* c, int32_t tag);  // the gathered payloads of the exchange that has just completed, or an error when the caller skipped it
// take_exchange + unpack_all; `what` names the payload in the error text
template <class P> int take_payloads(sq_ctx* c, std::vector<P>& out, const char* what) {
    const int rc = take_exchange(c, P().tag);
    if (rc) return rc;
    return unpack_all(c->xgot, out) ? (int)SQ_OK : fail(c, SQ_E_ARG, std::string("sharded run: malformed ") + what + " payload");
}

// locals of build_graph that have to survive an exchange
struct GraphBuild {
    int stage = 0;
    std::shared_ptr<SegPlan> plan;
    std::vector<Blk> disc;
    int64_t n_break = 0;
    int64_t trigger_last = 0;
    std::vector<Node> seeds;
    std::vector<Edge> raw, conc, before;  // before: the edges in front of FilterEdges (the filter is repeated when a depth decision was ambiguous)
    std::vector<uint8_t> keep;          // KeepEdge of FilterbyInterleaving
    std::vector<int32_t> sup, amb_plus, amb_minus;
    std::vector<int64_t> sl;
    bool tiny_boundary = false;
    std::vector<int32_t> first_chr;   // sharded: chromosome of every rank's first kept record (-1: none)
    // sharded seed exchange: this shard's seeds under the three possible pasts (see resolve_seeds)
    std::vector<Node> seedsA, seedsB, seedsC;
    std::vector<int32_t> sensB;
    bool hasC = false;
    Node seedC{0, 0, 0, 0, 0.0};
    std::future<double> clusters;     // segment_clusters running next to the record kernels
    ~GraphBuild() { if (clusters.valid()) clusters.wait(); }  // (a pooled task's future does not wait by itself; the task writes into this object)
};
void pack_seeds(sq_ctx* c, const GraphBuild& g);

// the same for call_sv
struct SvBuild {
    int stage = 0;
    BPMap bpmap;
    // the breakpoint pairs of every edge, once (edge i: entries [eoff[i], eoff[i + 1]); round 4 looked every edge up three times in the map)
    std::vector<int32_t> eoff;
    std::vector<std::pair<std::pair<int, int>, std::pair<int, int>>> ebp;
    std::vector<uint8_t> eexact;
    std::vector<std::pair<int, int>> BPs;
    std::vector<int32_t> diff;  // this shard's difference array
    int cur_prev = 0;
    BpBoundary bb;
};

}  // namespace sq
