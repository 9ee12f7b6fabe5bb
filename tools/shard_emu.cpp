// The protocol of a chromosome-sharded run (squid_amd/csrc/sq_shard.h) without a device and without N ranks: the bytes of the six
// payloads, their round trip and what is refused, and the decisions a rank takes from the gathered payloads on tables given on the
// command line (linked against libsquid_hip.so; tests/test_shard_emu.py has the expected values).  Every decision runs as it does in
// the library: the tables become payloads, the payloads bytes, the bytes of all ranks are unpacked, the decision reads those.
//   shard_emu wire                                   one fixed instance of each payload as hex (the numbers: wire() below and the test)
//   shard_emu fuzz <instances> <seed>                random instances: round trip, every proper prefix, another tag, a vector count of 2^62
//   shard_emu dedup <me> <rank>...                   rank = has1,empty1,has2,empty2
//   shard_emu streams <me> <own_trigger> <rank>...   rank = kept,first_refid,first_pos,other_max,trigger_last
//   shard_emu seeds <first_chr,...> <rank>...        rank = A;hasB;B;sens;hasC;seedC;C          (lists of numbers, nodes as chr,pos,len)
//   shard_emu cursors <nb> <rank>...                 rank = assumed;end;has_p3;has_event;n_p3;absorb;diff
//   shard_emu graph <nn> <rank>...                   rank = lo;hi;n_other;tiny;v0;v1;v2;v3;v4;v5;edges;n_raw   (edges: a:b:ha:hb:w,...)
//   shard_emu other <rank>...                        rank = chr;pos;len
#include "../squid_amd/csrc/sq_shard.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
using namespace sq;
typedef std::vector<uint8_t> Bytes;
#ifdef SHARD_EMU_STANDALONE  // built from this file and sq_shard.cpp alone, without the library (sanitizer builds): the one function sq_shard.cpp takes from it
int sq::fail(sq_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }
#endif

namespace {
std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out(1);
    for (char ch : s) if (ch == sep) out.emplace_back(); else out.back() += ch;
    return out;
}
std::vector<int64_t> nums(const std::string& s, char sep = ',') {
    std::vector<int64_t> v;
    if (!s.empty()) for (const std::string& t : split(s, sep)) v.push_back(std::strtoll(t.c_str(), nullptr, 10));
    return v;
}
std::vector<int32_t> nums32(const std::string& s) { std::vector<int32_t> v; for (int64_t x : nums(s)) v.push_back((int32_t)x); return v; }
std::vector<std::string> fields_of(const char* arg, size_t n) {
    std::vector<std::string> f = split(arg, ';');
    if (f.size() != n) { std::fprintf(stderr, "shard_emu: '%s' has %zu fields, not %zu\n", arg, f.size(), n); std::exit(2); }
    return f;
}
template <class T> void print_list(const char* name, const std::vector<T>& v) {
    std::printf("%s=", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? "," : "", (long long)v[i]);
    std::printf(" ");
}
void print_hex(const char* name, const Bytes& b) {
    std::printf("%s ", name);
    for (uint8_t x : b) std::printf("%02x", x);
    std::printf("\n");
}
// the payloads of all ranks as the exchange delivers them
template <class P> std::vector<P> gathered(const std::vector<P>& ranks) {
    std::vector<Bytes> got(ranks.size());
    for (size_t r = 0; r < ranks.size(); ++r) ranks[r].pack(got[r]);
    std::vector<P> out;
    if (check_tags(got, P().tag) || !unpack_all(got, out)) { std::fprintf(stderr, "shard_emu: a packed payload does not unpack\n"); std::exit(3); }
    return out;
}

int wire() {
    Bytes b;
    XDedup d; d.last[0] = 1; d.last[1] = 0; d.last[2] = 1; d.last[3] = 1;
    d.pack(b); print_hex("X_DEDUP", b);
    XStream s; s.kept = 5000000000ll; s.first_refid = 3; s.first_pos = 123456; s.other_max = (7ll << 32) | 99; s.trigger_last = -1;
    s.pack(b); print_hex("X_STREAM", b);
    XSeeds e; e.a = {0, 100, 50, 0, 400, 30}; e.hasB = 1; e.b = {1, 20, 5}; e.sens = {150, 151, 152, 153}; e.hasC = 1; e.seedC[0] = 0; e.seedC[1] = 100; e.seedC[2] = 50; e.c = {0, 100, 80, 0, 300, 10, 2, 7, 9};
    e.pack(b); print_hex("X_SEEDS", b);
    XGraph g; g.lo = 2; g.hi = 5; g.n_other = 77; g.tiny = 1;
    g.v[0] = {1, 2, 3}; g.v[1] = {100, 200, 300}; g.v[2] = {4, 5, 6}; g.v[3] = {40, 50, 60}; g.v[4] = {0, 1, 0}; g.v[5] = {2, 0, -1};
    for (const Edge& x : {make_edge(2, true, 4, false, 11), make_edge(3, false, 3, true, 7), make_edge(1000000, true, 5, true, 1)}) { g.keys.push_back(edge_pack(x)); g.ws.push_back(x.w); }
    g.n_raw = 123456789012ll;
    g.pack(b); print_hex("X_GRAPH", b);
    XBpSup p; p.assumed = 6; p.end = 9; p.has_p3 = 1; p.has_event = 0; p.n_p3 = 1234567890123ll; p.absorb = 5; p.diff = {1, -1, 0, 2, -2};
    p.pack(b); print_hex("X_BPSUP", b);
    XOther o; o.chr = {0, 0, 3}; o.pos = {10, 20, 30}; o.len = {76, 3, 1};
    o.pack(b); print_hex("X_OTHER", b);
    return 0;
}

// ---- fuzz
typedef std::mt19937_64 Rng;
int32_t r32(Rng& g) { return (int32_t)g(); }
int64_t r64(Rng& g) { return (int64_t)g(); }
std::vector<int32_t> rvec(Rng& g) { std::vector<int32_t> v(g() % 4 == 0 ? 0 : g() % 9); for (int32_t& x : v) x = r32(g); return v; }
void randomize(XDedup& x, Rng& g) { for (int32_t& v : x.last) v = (int32_t)(g() & 1); }
void randomize(XStream& x, Rng& g) { x.kept = r64(g); x.first_refid = r32(g); x.first_pos = r32(g); x.other_max = r64(g); x.trigger_last = r64(g); }
void randomize(XSeeds& x, Rng& g) { x.a = rvec(g); x.hasB = (int32_t)(g() & 1); x.b = rvec(g); x.sens = rvec(g); x.hasC = (int32_t)(g() & 1); for (int32_t& v : x.seedC) v = r32(g); x.c = rvec(g); }
void randomize(XGraph& x, Rng& g) {
    x.lo = r32(g); x.hi = r32(g); x.n_other = r64(g); x.tiny = (int32_t)(g() & 1); x.n_raw = r64(g);
    for (auto& v : x.v) v = rvec(g);
    x.keys.resize(g() % 4 == 0 ? 0 : g() % 9); for (uint64_t& k : x.keys) k = g();
    x.ws = rvec(g);
}
void randomize(XBpSup& x, Rng& g) { x.assumed = r32(g); x.end = r32(g); x.has_p3 = (int32_t)(g() & 1); x.has_event = (int32_t)(g() & 1); x.n_p3 = r64(g); x.absorb = r64(g); x.diff = rvec(g); }
void randomize(XOther& x, Rng& g) { x.chr = rvec(g); x.pos = rvec(g); x.len = rvec(g); }
template <class T, size_t N> bool same(const T (&a)[N], const T (&b)[N]) { for (size_t i = 0; i < N; ++i) if (!(a[i] == b[i])) return false; return true; }
bool equal(const XDedup& a, const XDedup& b) { return a.tag == b.tag && same(a.last, b.last); }
bool equal(const XStream& a, const XStream& b) { return a.tag == b.tag && a.kept == b.kept && a.first_refid == b.first_refid && a.first_pos == b.first_pos && a.other_max == b.other_max && a.trigger_last == b.trigger_last; }
bool equal(const XSeeds& a, const XSeeds& b) { return a.tag == b.tag && a.a == b.a && a.hasB == b.hasB && a.b == b.b && a.sens == b.sens && a.hasC == b.hasC && same(a.seedC, b.seedC) && a.c == b.c; }
bool equal(const XGraph& a, const XGraph& b) { return a.tag == b.tag && a.lo == b.lo && a.hi == b.hi && a.n_other == b.n_other && a.tiny == b.tiny && same(a.v, b.v) && a.keys == b.keys && a.ws == b.ws && a.n_raw == b.n_raw; }
bool equal(const XBpSup& a, const XBpSup& b) { return a.tag == b.tag && a.assumed == b.assumed && a.end == b.end && a.has_p3 == b.has_p3 && a.has_event == b.has_event && a.n_p3 == b.n_p3 && a.absorb == b.absorb && a.diff == b.diff; }
bool equal(const XOther& a, const XOther& b) { return a.tag == b.tag && a.chr == b.chr && a.pos == b.pos && a.len == b.len; }

struct Tally { long instances = 0, bytes = 0, empty_vectors = 0, prefixes = 0, tags = 0, huge = 0, differences = 0; };
// first_count: offset of the payload's first vector count (-1: it has no vector)
template <class P> void fuzz_payload(int n, Rng& g, long first_count, Tally& t) {
    for (int i = 0; i < n; ++i) {
        P x, y;
        randomize(x, g);
        Bytes b;
        x.pack(b);
        ++t.instances; t.bytes += (long)b.size();
        if (!y.unpack(b) || !equal(x, y)) ++t.differences;
        for (size_t k = 0; k < b.size(); ++k) {  // every proper prefix is refused
            P z;
            if (z.unpack(Bytes(b.begin(), b.begin() + (long)k))) ++t.differences;
            ++t.prefixes;
        }
        // take_exchange's rule: the tag every rank sent is the expected one, and at least the tag is there
        const std::vector<Bytes> got = {b, b};
        if (check_tags(got, x.tag) != nullptr) ++t.differences;
        for (int32_t other = X_DEDUP; other <= X_OTHER; ++other) if (other != x.tag) {
            const char* err = check_tags(got, other);
            if (!err || std::string(err) != "sharded run: ranks are out of step (payload tag mismatch)") ++t.differences;
            Bytes w = b; std::memcpy(w.data(), &other, 4);
            P z;
            if (z.unpack(w)) ++t.differences;
            ++t.tags;
        }
        const char* err = check_tags({b, Bytes(b.begin(), b.begin() + 3)}, x.tag);
        if (!err || std::string(err) != "sharded run: short exchange payload") ++t.differences;
        if (first_count >= 0) {  // a count no payload can hold: refused by the count, nothing is allocated
            for (const int64_t huge : {(int64_t)1 << 62, (int64_t)1 << 61, INT64_MAX, (int64_t)-1}) {
                Bytes w = b; std::memcpy(w.data() + first_count, &huge, 8);
                P z;
                if (z.unpack(w)) ++t.differences;
                ++t.huge;
            }
            int64_t cnt; std::memcpy(&cnt, b.data() + first_count, 8);
            t.empty_vectors += cnt == 0;
        }
    }
}
int fuzz(int n, uint64_t seed) {
    Rng g(seed);
    Tally t;
    fuzz_payload<XDedup>(n, g, -1, t); fuzz_payload<XStream>(n, g, -1, t);
    fuzz_payload<XSeeds>(n, g, 4, t); fuzz_payload<XGraph>(n, g, 24, t); fuzz_payload<XBpSup>(n, g, 36, t); fuzz_payload<XOther>(n, g, 4, t);
    std::printf("%ld instances, %ld bytes, empty first vectors %ld, prefixes refused %ld, other tags refused %ld, huge counts refused %ld, %ld differences%s\n", t.instances, t.bytes, t.empty_vectors,
                t.prefixes, t.tags, t.huge, t.differences, t.differences ? "" : ": same");
    return t.differences ? 1 : 0;
}

// ---- decisions
int dedup(int argc, char** argv) {
    std::vector<XDedup> p;
    for (int i = 1; i < argc; ++i) { const std::vector<int64_t> f = nums(argv[i]); XDedup x; for (int k = 0; k < 4; ++k) x.last[k] = (int32_t)f.at(k); p.push_back(x); }
    std::printf("dedup_mask=%d\n", dedup_mask(gathered(p), std::atoi(argv[0])));
    return 0;
}
int streams(int argc, char** argv) {
    std::vector<XStream> p;
    for (int i = 2; i < argc; ++i) {
        const std::vector<int64_t> f = nums(argv[i]);
        XStream x; x.kept = f.at(0); x.first_refid = (int32_t)f.at(1); x.first_pos = (int32_t)f.at(2); x.other_max = f.at(3); x.trigger_last = f.at(4);
        p.push_back(x);
    }
    Shard sh;
    std::vector<int32_t> first_chr;
    merge_streams(gathered(p), std::atoi(argv[0]), std::strtoll(argv[1], nullptr, 10), sh, first_chr);
    std::printf("kept_before=%lld kept_total=%lld prior_kept=%d other_seed=%lld has_terminal=%d term=%d,%d n_break_global=%lld ", (long long)sh.kept_before, (long long)sh.kept_total, (int)sh.prior_kept,
                sh.other_seed, (int)sh.has_terminal, sh.has_terminal ? sh.term_refid : 0, sh.has_terminal ? sh.term_pos : 0, (long long)sh.n_break_global);
    print_list("first_chr", first_chr);
    std::printf("\n");
    return 0;
}
int seeds(int argc, char** argv) {
    const std::vector<int32_t> first_chr = nums32(argv[0]);
    std::vector<XSeeds> p;
    for (int i = 1; i < argc; ++i) {
        const std::vector<std::string> f = fields_of(argv[i], 7);
        XSeeds x; x.a = nums32(f[0]); x.hasB = std::atoi(f[1].c_str()); x.b = nums32(f[2]); x.sens = nums32(f[3]); x.hasC = std::atoi(f[4].c_str());
        const std::vector<int32_t> sc = nums32(f[5]); for (int k = 0; k < 3; ++k) x.seedC[k] = sc.at(k);
        x.c = nums32(f[6]);
        p.push_back(x);
    }
    std::vector<Node> all;
    int redo = -1;
    Node last{0, 0, 0, 0, 0.0};
    resolve_seeds(gathered(p), first_chr, all, redo, last);
    std::vector<int32_t> flat;
    for (const Node& n : all) { flat.push_back(n.chr); flat.push_back(n.pos); flat.push_back(n.len); }
    print_list("all", flat);
    std::printf("redo=%d last=%d,%d,%d\n", redo, redo >= 0 ? last.chr : 0, redo >= 0 ? last.pos : 0, redo >= 0 ? last.len : 0);
    return 0;
}
int cursors(int argc, char** argv) {
    std::vector<XBpSup> p;
    for (int i = 1; i < argc; ++i) {
        const std::vector<std::string> f = fields_of(argv[i], 7);
        XBpSup x; x.assumed = std::atoi(f[0].c_str()); x.end = std::atoi(f[1].c_str()); x.has_p3 = std::atoi(f[2].c_str()); x.has_event = std::atoi(f[3].c_str());
        x.n_p3 = std::strtoll(f[4].c_str(), nullptr, 10); x.absorb = std::strtoll(f[5].c_str(), nullptr, 10); x.diff = nums32(f[6]);
        p.push_back(x);
    }
    std::vector<int64_t> total;
    int bad = -1, truth = 0;
    if (const char* err = check_cursors(gathered(p), (size_t)std::atoll(argv[0]), total, bad, truth)) { std::printf("error=%s\n", err); return 0; }
    std::printf("bad=%d truth=%d ", bad, truth);
    print_list("total", total);
    std::printf("\n");
    return 0;
}
int graph(int argc, char** argv) {
    const int nn = std::atoi(argv[0]);
    std::vector<XGraph> p;
    for (int i = 1; i < argc; ++i) {
        const std::vector<std::string> f = fields_of(argv[i], 12);
        XGraph x; x.lo = std::atoi(f[0].c_str()); x.hi = std::atoi(f[1].c_str()); x.n_other = std::strtoll(f[2].c_str(), nullptr, 10); x.tiny = std::atoi(f[3].c_str());
        for (int k = 0; k < 6; ++k) x.v[k] = nums32(f[4 + (size_t)k]);
        if (!f[10].empty()) for (const std::string& e : split(f[10], ',')) {
            const std::vector<int64_t> q = nums(e, ':');
            const Edge made = make_edge((int)q.at(0), q.at(2) != 0, (int)q.at(1), q.at(3) != 0, (int)q.at(4));
            x.keys.push_back(edge_pack(made)); x.ws.push_back(made.w);
        }
        x.n_raw = std::strtoll(f[11].c_str(), nullptr, 10);
        p.push_back(x);
    }
    std::vector<int32_t> sup, amb_plus, amb_minus;
    std::vector<int64_t> sl;
    std::vector<Edge> conc;
    bool tiny = false;
    int64_t n_raw = 0;
    if (const char* err = merge_graph(gathered(p), nn, sup, sl, amb_plus, amb_minus, tiny, conc, n_raw)) { std::printf("error=%s\n", err); return 0; }
    print_list("sup", sup); print_list("sl", sl); print_list("amb_plus", amb_plus); print_list("amb_minus", amb_minus);
    std::printf("tiny=%d conc=", (int)tiny);
    for (size_t i = 0; i < conc.size(); ++i) std::printf("%s%d:%d:%d:%d:%d:%d", i ? "," : "", conc[i].a, conc[i].b, (int)conc[i].ha, (int)conc[i].hb, conc[i].w, conc[i].gw);
    std::printf(" n_raw=%lld\n", (long long)n_raw);
    return 0;
}
int other(int argc, char** argv) {
    std::vector<XOther> p;
    for (int i = 0; i < argc; ++i) { const std::vector<std::string> f = fields_of(argv[i], 3); XOther x; x.chr = nums32(f[0]); x.pos = nums32(f[1]); x.len = nums32(f[2]); p.push_back(x); }
    std::vector<OtherR> list;
    if (const char* err = gather_other(gathered(p), list)) { std::printf("error=%s\n", err); return 0; }
    std::printf("other=");
    for (size_t i = 0; i < list.size(); ++i) std::printf("%s%d:%d:%d", i ? "," : "", list[i].chr, list[i].pos, list[i].len);
    std::printf("\n");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "wire") return wire();
    if (cmd == "fuzz" && argc == 4) return fuzz(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10));
    if (cmd == "dedup" && argc >= 4) return dedup(argc - 2, argv + 2);
    if (cmd == "streams" && argc >= 5) return streams(argc - 2, argv + 2);
    if (cmd == "seeds" && argc >= 4) return seeds(argc - 2, argv + 2);
    if (cmd == "cursors" && argc >= 4) return cursors(argc - 2, argv + 2);
    if (cmd == "graph" && argc >= 4) return graph(argc - 2, argv + 2);
    if (cmd == "other" && argc >= 3) return other(argc - 2, argv + 2);
    std::fprintf(stderr, "usage: shard_emu wire | fuzz <instances> <seed> | dedup|streams|seeds|cursors|graph|other <tables> (see the head of tools/shard_emu.cpp)\n");
    return 2;
}
