// C-ABI entry points of libsquid_hip.so (include/squid_hip.h): the ingest and debug entry points; the pipelines behind sq_build_graph / sq_call_sv are sq_build.cpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>

#include <sys/stat.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <unistd.h>

#include "sq_internal.h"
#include <malloc.h>

namespace sq {

// sq_ingest_files decodes the chimeric file on a second thread while the calling thread may report its own errors into c->err:
// the helper's messages go to c->chim_err (this thread-local names it) and reach c->err when chim_join collects the result
static thread_local std::string* tl_err_sink = nullptr;
// a helper thread of the library sends its error texts to a string of its own (the thread that owns the context moves it into c->err once
// the helper has been joined): the chimeric decode of sq_ingest_files, the planner thread of the GPU reader
ErrSink::ErrSink(std::string* to) { tl_err_sink = to; }
ErrSink::~ErrSink() { tl_err_sink = nullptr; }
int fail(sq_ctx* c, int code, const std::string& msg) {
    if (tl_err_sink) *tl_err_sink = msg;
    else if (c) c->err = msg;
    return code;
}
int chim_join_names(sq_ctx* c) {
    if (!c->chim_names_future.valid()) return SQ_OK;
    const int rc = c->chim_names_future.get();  // (once: the future is invalid afterwards)
    if (rc) { c->err = c->chim_err; return rc; }
    return SQ_OK;
}
int chim_join(sq_ctx* c) {
    if (!c->chim_future.valid()) return SQ_OK;
    const int rc_names = chim_join_names(c);  // (a concordant file without records never reached the parse)
    const int rc = c->chim_future.get();
    if (rc) { c->err = c->chim_err; return rc; }
    if (rc_names) return rc_names;
    return dev_chim_finalize(c, c->chim_dead);
}

int Timer::slot(const char* name) {
    for (size_t i = 0; i < names.size(); ++i) if (names[i] == name || !std::strcmp(names[i], name)) return (int)i;
    names.push_back(name); ms.push_back(0); bytes.push_back(0); busy.push_back(0); launches.push_back(0);
    return (int)names.size() - 1;
}
void Timer::add(const char* name, double ms_, double bytes_, int64_t n) {
    int s = slot(name);
    ms[s] += ms_; bytes[s] += bytes_; launches[s] += n;
}
void Timer::add_busy(const char* name, double ms_) { busy[slot(name)] += ms_; }
void Timer::clear() { names.clear(); ms.clear(); bytes.clear(); busy.clear(); launches.clear(); }

void GraphSnap::take(const std::vector<Node>& N, const std::vector<Edge>& E, const std::vector<int32_t>* lab) {
    const size_t n = N.size(), m = E.size();
    chr.resize(n); pos.resize(n); len.resize(n); support.resize(n); depth.resize(n); label.assign(n, 0);
    for (size_t i = 0; i < n; ++i) { chr[i] = N[i].chr; pos[i] = N[i].pos; len[i] = N[i].len; support[i] = N[i].support; depth[i] = N[i].depth; }
    if (lab) label = *lab;
    ind1.resize(m); ind2.resize(m); weight.resize(m); gweight.resize(m); h1.resize(m); h2.resize(m);
    for (size_t i = 0; i < m; ++i) { ind1[i] = E[i].a; ind2[i] = E[i].b; weight[i] = E[i].w; gweight[i] = E[i].gw; h1[i] = E[i].ha; h2[i] = E[i].hb; }
}
void GraphSnap::view(sq_graph* g) const {
    g->n_nodes = (int32_t)chr.size(); g->n_edges = (int32_t)ind1.size();
    g->chr = chr.data(); g->pos = pos.data(); g->len = len.data(); g->support = support.data(); g->label = label.data(); g->avgdepth = depth.data();
    g->ind1 = ind1.data(); g->ind2 = ind2.data(); g->weight = weight.data(); g->groupweight = gweight.data(); g->head1 = h1.data(); g->head2 = h2.data();
}

static void drop_early_clusters(sq_ctx* c) { c->plan_early.reset(); c->disc_early.clear(); c->disc_early.shrink_to_fit(); c->clusters_early_ms = -1; }

}  // namespace sq

using namespace sq;

// No exception leaves the library: the host stages allocate (std::bad_alloc from the vectors, the raw scratch blocks and the bodies of
// HostPool::parallel_for, which hands a helper's exception to its caller) -- at the C boundary that becomes SQ_E_CAPACITY with a message.
template <class F> static int abi_guard(sq_ctx* c, const char* what, F f) {
    try { return f(); }
    catch (const std::bad_alloc&) { return c ? sq::fail(c, SQ_E_CAPACITY, std::string(what) + ": out of host memory") : (int)SQ_E_CAPACITY; }
    catch (const std::exception& e) { return c ? sq::fail(c, SQ_E_CAPACITY, std::string(what) + ": " + e.what()) : (int)SQ_E_CAPACITY; }
}

extern "C" {

void sq_default_params(sq_params* p) {
    std::memset(p, 0, sizeof *p);
    p->abi_version = SQ_ABI_VERSION;
    p->device = 0;
    p->phred_type = 1; p->max_lowphred_len = 10; p->min_phred = 4; p->min_mapqual = 1;
    p->concord_dist_pos = 50000; p->concord_dist_idx = 20; p->min_edge_weight = 5; p->discordant_ratio = 8; p->max_allowed_degree = 5;
    p->rank = 0; p->world_size = 1;
}

const char* sq_strerror(int code) {
    switch (code) {
        case SQ_OK: return "ok";
        case SQ_E_ARG: return "bad argument or call order";
        case SQ_E_NODEVICE: return "no usable HIP device";
        case SQ_E_HIP: return "HIP runtime error";
        case SQ_E_IO: return "cannot read BAM";
        case SQ_E_UNSORTED: return "input not coordinate sorted";
        case SQ_E_ASSERT: return "input trips a reference assert";
        case SQ_E_CAPACITY: return "internal capacity exceeded";
        case SQ_E_EMPTYCHIM: return "chimeric input has no usable record";
        default: return "unknown error";
    }
}
const char* sq_last_error(sq_ctx* c) { return c ? c->err.c_str() : ""; }

int sq_create(const sq_params* p, sq_ctx** out) {
    if (!p || !out || p->abi_version != SQ_ABI_VERSION) return SQ_E_ARG;
    sq_ctx* c = new sq_ctx();
    c->P = *p;
    c->pool.reset(new HostPool(host_workers(p->world_size)));
    if (env_set("SQUID_CHIM_STAGES_GPU")) c->chim_dev_env = env_nonzero("SQUID_CHIM_STAGES_GPU") ? 1 : 0;  // forces / forbids the device route of the chimeric graph stages
    if (env_set("SQUID_BWA_STAGES_GPU")) c->bwa_dev_env = env_nonzero("SQUID_BWA_STAGES_GPU") ? 1 : 0;    // the same for node depth / breakpoint support of a --bwa context
    if (env_set("SQUID_BWA_EDGES_GPU")) c->bwa_edges_env = env_nonzero("SQUID_BWA_EDGES_GPU") ? 1 : 0;    // the same for the BAM loop of RawEdges of a --bwa context
    if (env_set("SQUID_SEGMENT_GPU")) c->seg_dev_env = env_nonzero("SQUID_SEGMENT_GPU") ? 1 : 0;          // the same for BuildNode_STAR's segmentation automaton (not --bwa, not sharded)
    if (env_set("SQUID_BWA_NODES_GPU")) c->bwa_nodes_env = env_nonzero("SQUID_BWA_NODES_GPU") ? 1 : 0;    // the same for the record automaton of BuildNode_BWA of a --bwa context
    if (env_set("SQUID_COMPRESS_WINDOWS_GPU")) c->fc_windows_env = env_nonzero("SQUID_COMPRESS_WINDOWS_GPU") ? 1 : 0;  // the same for FurtherCompressNode's walk over windows (every context)
    int rc = dev_create(c);
    if (rc) { std::fprintf(stderr, "libsquid_hip: %s\n", c->err.c_str()); dev_destroy(c); delete c; return rc; }
    *out = c;
    return SQ_OK;
}
void sq_destroy(sq_ctx* c) {
    if (!c) return;
    if (c->bp_future.valid()) (void)c->bp_future.get();
    dev_chim_drop_pending(c);
    exchange_release(c);
    dev_destroy(c);
    delete c;
}
int sq_set_references(sq_ctx* c, int32_t n_ref, const int32_t* ref_len) {
    if (!c || n_ref < 0 || (n_ref && !ref_len)) return SQ_E_ARG;
    c->ref_len.assign(ref_len, ref_len + n_ref);
    drop_early_clusters(c);
    return SQ_OK;
}
// frags0 = frags, side by side (millions of fragments on a dense sample; sq_reset copies the other way)
static void copy_frags(sq_ctx* c, const std::vector<Frag>& src, std::vector<Frag>& dst) {
    dst.resize(src.size());
    HostPool* pool = c->pool.get();
    const int64_t n = (int64_t)src.size();
    const int pieces = (int)std::min<int64_t>(std::max<int64_t>(1, n / 4096), pool ? 4 * (pool->size() + 1) : 1);
    auto piece = [&](int k) { for (int64_t i = n * k / pieces; i < n * (k + 1) / pieces; ++i) dst[(size_t)i] = src[(size_t)i]; };
    if (pieces <= 1 || !pool) { for (int k = 0; k < pieces; ++k) piece(k); }
    else pool->parallel_for(pieces, 1 << 20, piece);
}
static int sq_ingest_chimeric_impl(sq_ctx* c, const sq_aln_batch* b) {
    if (!c || !b) return SQ_E_ARG;
    drop_early_clusters(c);
    int rc = build_fragments(c, b);
    if (rc) return rc;
    copy_frags(c, c->frags, c->frags0);
    return dev_upload_chim_names(c);
}
int sq_ingest_chimeric(sq_ctx* c, const sq_aln_batch* b) { return abi_guard(c, "sq_ingest_chimeric", [&]() { return sq_ingest_chimeric_impl(c, b); }); }
int sq_chim_contains(sq_ctx* c, const char* name, size_t len) {
    if (!c) return SQ_E_ARG;
    return std::binary_search(c->chim_names.begin(), c->chim_names.end(), std::string(name, len)) ? 1 : 0;
}
// does this shard own records of RefID `id`?  (the unplaced records at the end of a sorted BAM go to the last rank)
static inline bool shard_owns(const sq_ctx* c, int32_t id) {
    const Shard& sh = c->shard;
    if (!sh.on) return true;
    if (id < 0) return c->P.rank == c->P.world_size - 1;
    return id >= sh.first_ref && id < sh.end_ref;
}
static int sq_ingest_concordant_impl(sq_ctx* c, const sq_aln_batch* b) {
    if (!c || !b) return SQ_E_ARG;
    if (c->bwa) return fail(c, SQ_E_ARG, "this context holds a --bwa batch (sq_ingest_bwa_file): sq_clear_records before a STAR-mode ingest -- the mode is per context");
    if (!c->shard.on) return dev_append_records(c, b);
    // sharded: keep the runs of records this rank owns (one run per batch on a sorted stream)
    int64_t i = 0;
    while (i < b->n_rec) {
        while (i < b->n_rec && !shard_owns(c, b->refid[i])) ++i;
        int64_t j = i;
        while (j < b->n_rec && shard_owns(c, b->refid[j])) ++j;
        if (j > i) {
            sq_aln_batch v = *b;
            v.n_rec = j - i; v.n_blk = b->blk_off[j] - b->blk_off[i];
            v.refid += i; v.pos += i; v.mate_refid += i; v.mate_pos += i; v.end_pos += i; v.flag += i; v.mapq += i; v.aux += i; v.totlen += i; v.blk_off += i;
            const uint32_t o = b->blk_off[i] - b->blk_off[0];
            v.b_refpos += o; v.b_matchref += o; v.b_readpos += o; v.b_matchread += o;
            int rc = dev_append_records(c, &v);
            if (rc) return rc;
        }
        i = j;
    }
    return SQ_OK;
}
int sq_ingest_concordant(sq_ctx* c, const sq_aln_batch* b) { return abi_guard(c, "sq_ingest_concordant", [&]() { return sq_ingest_concordant_impl(c, b); }); }
static int ingest_raw(sq_ctx* c, const uint8_t* bam, size_t nbytes, const unsigned long long* rec_off, int64_t n_rec) {
    if (!c->shard.on) return dev_parse_append(c, bam, nbytes, rec_off, n_rec);
    // sharded: RefID sits 4 bytes into a record; upload only the byte range of the runs this rank owns
    auto refid_at = [&](int64_t i) { int32_t v; std::memcpy(&v, bam + rec_off[i] + 4, 4); return v; };
    int64_t i = 0;
    std::vector<unsigned long long> off;
    while (i < n_rec) {
        while (i < n_rec && (rec_off[i] + 8 > nbytes || !shard_owns(c, refid_at(i)))) ++i;
        int64_t j = i;
        while (j < n_rec && rec_off[j] + 8 <= nbytes && shard_owns(c, refid_at(j))) ++j;
        if (j > i) {
            const unsigned long long lo = rec_off[i], hi = j < n_rec ? rec_off[j] : (unsigned long long)nbytes;
            off.resize((size_t)(j - i));
            for (int64_t k = i; k < j; ++k) off[(size_t)(k - i)] = rec_off[k] - lo;
            int rc = dev_parse_append(c, bam + lo, (size_t)(hi - lo), off.data(), j - i);
            if (rc) return rc;
        }
        i = j;
    }
    return SQ_OK;
}
int sq_ingest_concordant_bam(sq_ctx* c, const uint8_t* bam, size_t nbytes, const uint64_t* rec_off, int64_t n_rec) {
    if (!c || (n_rec && (!bam || !rec_off))) return SQ_E_ARG;
    if (c->bwa) return fail(c, SQ_E_ARG, "this context holds a --bwa batch (sq_ingest_bwa_file): sq_clear_records before a STAR-mode ingest -- the mode is per context");
    int rc = ingest_raw(c, bam, nbytes, (const unsigned long long*)rec_off, n_rec);
    dev_flush_timers(c);
    return rc;
}
int sq_read_header(const char* path, int32_t* n_ref, int32_t* ref_len, char* names, size_t names_cap) {
    std::vector<std::string> nm;
    std::vector<int32_t> ln;
    std::string err;
    int rc = read_bam_header(path, nm, ln, err);
    if (rc) return rc;
    if (n_ref) {
        int cap = *n_ref;
        *n_ref = (int32_t)nm.size();
        if (ref_len) for (int i = 0; i < (int)nm.size() && i < cap; ++i) ref_len[i] = ln[i];
    }
    if (names && names_cap) {
        size_t o = 0;
        for (const std::string& s : nm) {
            if (o + s.size() + 1 >= names_cap) break;
            std::memcpy(names + o, s.data(), s.size());
            o += s.size();
            names[o++] = '\n';
        }
        names[o < names_cap ? o : names_cap - 1] = 0;
    }
    return SQ_OK;
}
// the whole chimeric BAM as one batch -> fragments (the batch is consumed where the reader hands it over: no copy of it)
// `early` (sq_ingest_files): as soon as the records are decoded, the device gets the table of all their usable QNAMEs and the promise
// the record parse of the concordant BAM waits for is kept -- the pairing goes on meanwhile
static int chimeric_file_to_fragments(sq_ctx* c, const char* path, int nt, std::string& err, bool early = false, const HostBatch* decoded = nullptr) {
    const auto t_chim0 = std::chrono::steady_clock::now();
    static const bool chim_prof = env_set("SQUID_CHIM_PROF");
    auto lap = [&](const char* what) { if (chim_prof) std::fprintf(stderr, "chimeric file: %-28s at %8.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_chim0).count()); };
    drop_early_clusters(c);
    ParseOpts o{c->P.phred_type, c->P.min_phred, c->P.max_lowphred_len, true, nullptr};
    bool got = false, promised = false;
    auto promise = [&](int rc) { if (early && !promised) { promised = true; c->chim_names_promise.set_value(rc); } };
    const std::function<int(const HostBatch&)> take = [&](const HostBatch& hb) {
        sq_aln_batch b;
        hb.view(&b, true);
        got = true;
        if (early && decoded) promise(SQ_OK);  // (chimeric_records_through_the_device has made the table from the names on the device: dev_chim_begin_captured)
        else if (early) {
            // one entry per usable record (mapped, not a duplicate: ReadRec.cpp:344), the name with a trailing /1 or /2 cut off
            // (ReadRec.cpp:62-66), plus the empty name the reference's set always holds (SegmentGraph.cpp:196-201, ledger B9)
            std::vector<uint32_t> off, len;
            off.reserve((size_t)b.n_rec + 1); len.reserve((size_t)b.n_rec + 1);
            for (int64_t i = 0; i < b.n_rec; ++i) {
                if ((b.flag[i] & 0x4) || (b.flag[i] & 0x400)) continue;
                const char* nm = b.name_blob + b.name_off[i];
                size_t L = b.name_off[i + 1] - b.name_off[i];
                if (L >= 2 && nm[L - 2] == '/' && (nm[L - 1] == '1' || nm[L - 1] == '2')) L -= 2;
                off.push_back(b.name_off[i]); len.push_back((uint32_t)L);
            }
            if (!off.empty()) { off.push_back(0); len.push_back(0); }
            lap("records decoded");
            const int rt = off.empty() ? SQ_OK : dev_chim_begin(c, b.name_blob, (size_t)b.name_off[b.n_rec], off.data(), len.data(), off.size());
            promise(rt);
            lap("name table handed to the device");
            if (rt) return rt;
        }
        const int rf = build_fragments(c, &b);
        lap("fragments built");
        return rf;
    };
    // `decoded`: the records came through the GPU reader (chimeric_records_through_the_device); otherwise the host decoder reads the file
    int rc = decoded ? (decoded->refid.empty() ? SQ_OK : take(*decoded)) : parse_bam_file(path, o, (size_t)1 << 40, nt, err, take);
    lap("reader returned");
    if (!rc && !got) rc = fail(c, SQ_E_EMPTYCHIM, "chimeric BAM holds no record");
    promise(rc ? rc : SQ_OK);  // (whatever happened: nobody waits for ever)
    if (rc) return rc;
    if (early && !c->ref_len.empty()) {  // this thread has nothing else to do, the concordant file is still being read
        // (the copy sq_reset restores the fragments from is made next to the cluster table: both only read c->frags)
        std::future<void> copied = std::async(std::launch::async, [c]() { copy_frags(c, c->frags, c->frags0); });
        c->plan_early.reset(); c->disc_early.clear();
        c->clusters_early_ms = segment_clusters(c, c->plan_early, c->disc_early);
        lap("cluster table");
        copied.get();
        lap("fragments copied");
        return SQ_OK;
    }
    copy_frags(c, c->frags, c->frags0);
    lap("fragments copied");
    return SQ_OK;
}
// BuildChimericSBamRecord on a context that has no device side (the junction-sequence utility): c->frags0
}  // extern "C"
int sq::chimeric_fragments_host(sq_ctx* c, const char* path, int threads) { return chimeric_file_to_fragments(c, path, std::max(1, threads), c->err); }
extern "C" {
static int sq_ingest_chimeric_file_impl(sq_ctx* c, const char* path) {
    if (!c || !path) return SQ_E_ARG;
    // (inflate and decode on a few threads: a dense sample has millions of chimeric records; the result does not depend on the count)
    const int nt = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 4));
    int rc = chimeric_file_to_fragments(c, path, nt, c->err);
    return rc ? rc : dev_upload_chim_names(c);
}
int sq_ingest_chimeric_file(sq_ctx* c, const char* path) { return abi_guard(c, "sq_ingest_chimeric_file", [&]() { return sq_ingest_chimeric_file_impl(c, path); }); }
// The chimeric BAM through the GPU reader (K-1 + K0 with sq_ctx::capture_names): BGZF inflate, record boundaries and the record parse on
// the device, the decoded records and their QNAMEs copied back as one batch -- the batch the host decoder (parse_bam_file, keep_names) makes
// of the same file, field for field.  On the dense config the host decoder is 0.6 s of sixteen threads = 9 of the 16 CPU-seconds per second
// a box gives the process; the device does it in the time it takes to get the file there.  Needs an empty record
// store (the records pass through it).  Returns 2 when the route is not taken or gave up: the caller runs the host decoder, whose
// error messages are then the ones the user sees.
static int chimeric_records_through_the_device(sq_ctx* c, const char* path, int n_threads, HostBatch& hb, bool name_table = true) {
    if (!c->dev || c->counts.n_concordant != 0) return 2;
    struct Mode { sq_ctx* c; Mode(sq_ctx* c) : c(c) { c->capture_names = true; } ~Mode() { c->capture_names = false; dev_clear_records(c); c->counts.n_concordant = 0; c->counts.n_blocks = 0; c->ingest_total_bytes = 0; c->ingest_seen_bytes = 0; } } mode(c);
    std::string err;
    c->ingest_total_bytes = 0; c->ingest_seen_bytes = 0;
    std::string saved_err = c->err;
    int rc = scan_bam_file(path, n_threads, err, [&](const uint8_t* bam, size_t nbytes, const unsigned long long* off, int64_t n) { c->ingest_seen_bytes += nbytes; return dev_parse_append(c, bam, nbytes, off, n); },
                           [&](size_t total) { c->ingest_total_bytes = total; }, nullptr,
                           [&](const uint8_t* file, std::vector<BgzfRange>& blocks, size_t b0, size_t b1, size_t begin, bool synced, int nref, const IndexMore& more, size_t file_bytes, GpuFileSrc* src) {
                               return dev_ingest_bgzf(c, file, blocks, b0, b1, begin, synced, nref, more, file_bytes, src); }, false, true, true);
    static const bool prof = env_set("SQUID_CHIM_PROF");
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (prof) std::fprintf(stderr, "chimeric file on the device: %-24s at %8.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); };
    lap("reader returned (since then)");
    if (rc == SQ_OK && name_table) rc = dev_chim_begin_captured(c);
    lap("name table");
    if (rc == SQ_OK) rc = dev_download_records(c, hb);
    if (rc == SQ_OK) rc = dev_download_names(c, hb);
    lap("records and names copied back");
    dev_flush_timers(c);  // (its launches are not the concordant ingest's)
    if (rc != SQ_OK) { c->err = saved_err; hb.clear(); return 2; }
    return SQ_OK;
}
// both input files in one call: the chimeric BAM (1-2 % of the records, decoded on the host: 17 ms at C3) is read on a helper
// thread while the GPU reader starts on the concordant BAM; the record parse -- the first consumer of the chimeric QNAME set --
// waits for it (chim_join).  Same result as sq_ingest_chimeric_file followed by sq_ingest_concordant_file.
static int sq_ingest_files_impl(sq_ctx* c, const char* chim_path, const char* bam_path, int32_t n_threads) {
    if (!c || !chim_path || !bam_path) return SQ_E_ARG;
    if (c->bwa) return fail(c, SQ_E_ARG, "this context holds a --bwa batch (sq_ingest_bwa_file): sq_clear_records before a STAR-mode ingest -- the mode is per context");
    if (env_set("SQUID_HOST_PARSE") || env_set("SQUID_SERIAL_LOAD")) {  // (the host parser consults the name set record by record)
        const int rc = sq_ingest_chimeric_file(c, chim_path);
        return rc ? rc : sq_ingest_concordant_file(c, bam_path, n_threads);
    }
    const std::string chim = chim_path;
    c->chim_err.clear();
    c->chim_names_promise = std::promise<int>();
    c->chim_names_future = c->chim_names_promise.get_future();
    // a chimeric BAM of some size goes through the GPU reader first (SQUID_CHIM_GPU=1 / =0 forces / forbids it): the helper thread then
    // starts from decoded records
    std::shared_ptr<HostBatch> decoded;
    {
        struct stat st;
        const bool want = env_set("SQUID_CHIM_GPU") ? env_nonzero("SQUID_CHIM_GPU") : (::stat(chim_path, &st) == 0 && (size_t)st.st_size >= ((size_t)128 << 20));
        if (want) {
            // (the batch is the context's between calls, like the scratch of a whole-file read on the host: 0.5 GB of pages on the dense
            // config that the next read of a chimeric file finds in place; sq_release_reader_buffers gives them back)
            if (!c->chim_decoded || c->chim_decoded.use_count() > 1) c->chim_decoded = std::make_shared<HostBatch>();
            decoded = c->chim_decoded;
            if (chimeric_records_through_the_device(c, chim_path, n_threads, *decoded) != SQ_OK) decoded.reset();
        }
        c->counts.chimeric_through_gpu_reader = decoded ? 1 : 0;
    }
    c->chim_pairing_running = decoded != nullptr;
    c->chim_future = std::async(std::launch::async, [c, chim, n_threads, decoded]() {
        tl_err_sink = &c->chim_err;
        struct Unsink { sq_ctx* c; ~Unsink() { tl_err_sink = nullptr; c->chim_pairing_running = false; } } unsink{c};
        // (decode threads: the rank's share of the CPUs the process may really use -- eight ranks on one host decode the same file side by side)
        return chimeric_file_to_fragments(c, chim.c_str(), std::max(1, std::min({(int)n_threads, 16, usable_cpus() / std::max(1, c->P.world_size)})), c->chim_err, true, decoded.get());  // (the host decoder of the chimeric BAM: 16 threads 96 ms of decode per 9.6 M records, 64 threads 254 ms)
    });
    const int rc_conc = sq_ingest_concordant_file(c, bam_path, n_threads);
    const int rc_chim = chim_join(c);  // (a concordant file without records never reached the parse)
    return rc_chim ? rc_chim : rc_conc;
}
int sq_ingest_files(sq_ctx* c, const char* chim_path, const char* bam_path, int32_t n_threads) { return abi_guard(c, "sq_ingest_files", [&]() { return sq_ingest_files_impl(c, chim_path, bam_path, n_threads); }); }
int sq_set_source(sq_ctx* c, const char* path) {
    if (!c || !path) return SQ_E_ARG;
    struct stat st;
    if (::stat(path, &st) != 0) return fail(c, SQ_E_IO, std::string("cannot open bamfile ") + path);
    c->source_size = (uint64_t)st.st_size;
    c->source_mtime = (uint64_t)st.st_mtim.tv_sec * 1000000000ull + (uint64_t)st.st_mtim.tv_nsec;
    return SQ_OK;
}
static int sq_ingest_concordant_file_impl(sq_ctx* c, const char* path, int32_t n_threads) {
    if (!c || !path) return SQ_E_ARG;
    if (c->bwa) return fail(c, SQ_E_ARG, "this context holds a --bwa batch (sq_ingest_bwa_file): sq_clear_records before a STAR-mode ingest -- the mode is per context");
    { int r0 = sq_set_source(c, path); if (r0) return r0; }
    if (!env_set("SQUID_HOST_PARSE")) {
        // default: the host only inflates BGZF and finds record boundaries; K0 parses the records on the GPU
        const auto t_file0 = std::chrono::steady_clock::now();
        c->ingest_total_bytes = 0; c->ingest_seen_bytes = 0;
        const RefRange rr{c->shard.first_ref, c->shard.end_ref, c->P.rank == c->P.world_size - 1};
        const bool staged = !c->staged_path.empty() && c->staged_path == path;  // compressed bytes already in HBM (sq_stage_bam)
        struct DfileGuard { sq_ctx* c; ~DfileGuard() { c->ingest_dfile = nullptr; } } dfile_guard{c};
        if (staged) {
            struct stat st;
            if (::stat(path, &st) != 0 || (size_t)st.st_size != c->staged_bytes || (uint64_t)st.st_ino != c->staged_ino) return fail(c, SQ_E_IO, "the file changed since sq_stage_bam");
            if (((uint64_t)st.st_mtim.tv_sec * 1000000000ull + (uint64_t)st.st_mtim.tv_nsec) != c->staged_mtime) return fail(c, SQ_E_IO, "the file changed since sq_stage_bam");
            int r0 = dev_stage_file(c, nullptr, 0, &c->ingest_dfile);
            if (r0) return r0;
        }
        int rc = scan_bam_file(path, n_threads, c->err, [&](const uint8_t* bam, size_t nbytes, const unsigned long long* off, int64_t n) { c->ingest_seen_bytes += nbytes; return ingest_raw(c, bam, nbytes, off, n); },
                               [&](size_t total) { c->ingest_total_bytes = c->shard.on ? 0 : total; }, c->shard.on ? &rr : nullptr,
                               [&](const uint8_t* file, std::vector<BgzfRange>& blocks, size_t b0, size_t b1, size_t begin, bool synced, int nref, const IndexMore& more, size_t file_bytes, GpuFileSrc* src) {
                                   return dev_ingest_bgzf(c, file, blocks, b0, b1, begin, synced, nref, more, file_bytes, src); }, staged, true, !staged);
        c->ingest_total_bytes = 0;
        const double t_scan = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_file0).count();
        dev_flush_timers(c);
        if (env_set("SQUID_INGEST_TIMING")) std::fprintf(stderr, "ingest %s: reader returned after %.1f ms, timers flushed after %.1f ms\n", path, t_scan, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_file0).count());
        return rc;
    }
    if (c->chim_set.size() != c->chim_names.size()) { c->chim_set.clear(); c->chim_set.insert(c->chim_names.begin(), c->chim_names.end()); }
    ParseOpts o{c->P.phred_type, c->P.min_phred, c->P.max_lowphred_len, false, &c->chim_set};
    return parse_bam_file(path, o, (size_t)1 << 21, n_threads, c->err, [&](const HostBatch& hb) {
        sq_aln_batch b;
        hb.view(&b, false);
        return sq_ingest_concordant(c, &b);
    });
}
int sq_ingest_concordant_file(sq_ctx* c, const char* path, int32_t n_threads) { return abi_guard(c, "sq_ingest_concordant_file", [&]() { return sq_ingest_concordant_file_impl(c, path, n_threads); }); }
// `squid --bwa -b <bam>` (src/Config.cpp:98-100; src/main.cpp:33-37 runs without a chimeric file): every record of the one BAM file,
// decoded with its QNAME, is kept on the host; sq_build_graph then takes BuildNode_BWA / RawEdges (sq_bwa.cpp) over that batch.  With
// sq_bwa_on_device the first sq_build_graph also copies the batch into the device record table, where the node depth and the breakpoint
// support are computed; the host batch stays where it is for the two automata
static int sq_ingest_bwa_file_impl(sq_ctx* c, const char* path, int32_t n_threads) {
    if (!c || !path) return SQ_E_ARG;
    if (c->shard.on) return fail(c, SQ_E_ARG, "--bwa input is not chromosome-sharded");
    if (c->ref_len.empty()) return fail(c, SQ_E_ARG, "sq_set_references first");
    { int r0 = sq_set_source(c, path); if (r0) return r0; }
    if (c->bwa_resident) { dev_clear_records(c); c->bwa_resident = false; c->bwa_dev_active = false; }  // (the device table of the batch before)
    std::shared_ptr<HostBatch> all = c->bwa_spare ? std::move(c->bwa_spare) : std::make_shared<HostBatch>();
    c->bwa_spare.reset();
    // (the arrays keep their storage -- and, on the way through the GPU reader, their sizes: every element is overwritten by the copy back)
    {   // a file of 1 GiB and more through the GPU reader (SQUID_BWA_GPU=1 / =0 forces / forbids it): BGZF inflate, record boundaries and the
        // record parse on the device, the QNAMEs kept next to the records (sq_ctx::capture_names, as for a large chimeric BAM), one copy
        // back -- the batch the host decoder below makes, field for field; the two order-dependent loops of the mode then run on it
        struct stat st;
        const bool want = env_set("SQUID_BWA_GPU") ? env_nonzero("SQUID_BWA_GPU") : (::stat(path, &st) == 0 && (size_t)st.st_size >= ((size_t)1 << 30));
        if (want && chimeric_records_through_the_device(c, path, n_threads, *all, false) == SQ_OK) {
            c->bwa = all;
            c->counts.n_concordant = (int64_t)all->size();
            c->counts.n_blocks = (int64_t)all->b_refpos.size();
            c->counts.chimeric_through_gpu_reader = 1;
            return SQ_OK;
        }
        all->clear();
        c->counts.chimeric_through_gpu_reader = 0;
    }
    ParseOpts o{c->P.phred_type, c->P.min_phred, c->P.max_lowphred_len, true, nullptr};
    const int rc = parse_bam_file(path, o, (size_t)1 << 21, std::max(1, (int)n_threads), c->err, [&](const HostBatch& hb) {
        if (all->names.size() + hb.names.size() >= 0xffffffffull || all->b_refpos.size() + hb.b_refpos.size() >= 0xffffffffull) return fail(c, SQ_E_CAPACITY, "--bwa input beyond 4 GB of read names or 2^32 aligned blocks");
        all->append(hb);
        return (int)SQ_OK;
    });
    if (rc) return rc;
    c->bwa = all;
    c->counts.n_concordant = (int64_t)all->size();
    c->counts.n_blocks = (int64_t)all->b_refpos.size();
    return SQ_OK;
}
int sq_ingest_bwa_file(sq_ctx* c, const char* path, int32_t n_threads) { return abi_guard(c, "sq_ingest_bwa_file", [&]() { return sq_ingest_bwa_file_impl(c, path, n_threads); }); }
// utils/JunctionSequence.cpp as a library call: host work only (no context, no device)
int sq_junction_sequences(const char* bedpe_path, const char* chim_bam_path, const char* fasta_path, const char* out_prefix, char* errbuf, size_t errcap) {
    if (!bedpe_path || !chim_bam_path || !fasta_path || !out_prefix) return SQ_E_ARG;
    sq_ctx local;  // (never sees a device: only the host pool and the parse parameters -- the utility's own defaults, :520-524)
    sq_default_params(&local.P);
    local.pool.reset(new HostPool((int)std::min(15u, std::max(1u, std::thread::hardware_concurrency()) - 1)));
    std::vector<std::string> names;
    std::vector<int32_t> lens;
    int rc = read_bam_header(chim_bam_path, names, lens, local.err);
    if (!rc) { local.ref_len = lens; rc = chimeric_fragments_host(&local, chim_bam_path, 8); }
    if (!rc) rc = junction_sequences(&local, names, bedpe_path, fasta_path, out_prefix);
    if (rc && errbuf && errcap) { std::strncpy(errbuf, local.err.c_str(), errcap - 1); errbuf[errcap - 1] = 0; }
    return rc;
}
int sq_stage_bam(sq_ctx* c, const char* path) {
    if (!c || !path) return SQ_E_ARG;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(c, SQ_E_IO, std::string("cannot open bamfile ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) { ::close(fd); return fail(c, SQ_E_IO, std::string("cannot read ") + path); }
    const size_t n = (size_t)st.st_size;
    void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);  // (straight from the page cache: no second host copy of the file)
    ::close(fd);
    if (m == MAP_FAILED) return fail(c, SQ_E_IO, std::string("cannot map ") + path);
    c->staged_path.clear(); c->staged_bytes = 0;
    const uint8_t* d = nullptr;
    int rc = dev_stage_file(c, (const uint8_t*)m, n, &d);
    munmap(m, n);
    if (rc) return rc;
    c->staged_path = path; c->staged_bytes = n;
    c->staged_ino = (uint64_t)st.st_ino;
    c->staged_mtime = (uint64_t)st.st_mtim.tv_sec * 1000000000ull + (uint64_t)st.st_mtim.tv_nsec;
    return SQ_OK;
}
int sq_clear_records(sq_ctx* c) {
    if (!c) return SQ_E_ARG;
    int rc = sq_reset(c);
    if (rc) return rc;
    dev_clear_records(c);
    c->bwa_resident = false; c->bwa_dev_active = false;
    // (a --bwa batch is gigabytes in fourteen arrays: the context keeps its storage for the next --bwa ingest -- unmapping it and faulting
    // fresh pages in again was 0.25 s per sample at C3 --; sq_release_reader_buffers gives it back)
    if (c->bwa && c->bwa.use_count() == 1) c->bwa_spare = std::move(c->bwa);
    c->bwa.reset();
    const int64_t side_by_side = c->counts.token_passes_side_by_side;  // (a property of the process, not of the records)
    c->counts = sq_counts{};
    c->counts.token_passes_side_by_side = side_by_side;
    c->counts.n_chimeric_records = c->n_chim_records; c->counts.n_chim_fragments = (int64_t)c->frags.size(); c->counts.read_len = c->read_len;
    return SQ_OK;
}
// ---- record cache (include/squid_hip.h): header, then the arrays of DeviceRecords / sq_aln_batch, each 64-byte aligned
namespace {
struct CacheHeader {
    char magic[8];  // "SQSOA1\0\0"
    int64_t n_rec, n_blk;
    int32_t phred_type, min_phred, max_lowphred_len, n_ref;
    uint64_t chim_hash;
    uint64_t reserved[3];
};
uint64_t chim_set_hash(const sq_ctx* c) {  // order-independent
    uint64_t sum = 0x9e3779b97f4a7c15ull * (c->chim_names.size() + 1);
    for (const std::string& nm : c->chim_names) {
        uint64_t h = 1469598103934665603ull;
        for (unsigned char ch : nm) { h ^= ch; h *= 1099511628211ull; }
        h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
        sum += h;
    }
    return sum;
}
CacheHeader cache_header(const sq_ctx* c, int64_t n_rec, int64_t n_blk) {
    CacheHeader h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, "SQSOA1", 6);
    h.n_rec = n_rec; h.n_blk = n_blk;
    h.phred_type = c->P.phred_type; h.min_phred = c->P.min_phred; h.max_lowphred_len = c->P.max_lowphred_len; h.n_ref = (int32_t)c->ref_len.size();
    h.chim_hash = chim_set_hash(c);
    h.reserved[0] = c->source_size; h.reserved[1] = c->source_mtime;  // (0,0: written from host batches, no file to bind to)
    return h;
}
size_t pad64(size_t n) { return (n + 63) & ~(size_t)63; }
}  // namespace
int sq_save_records(sq_ctx* c, const char* path) {
    if (!c || !path) return SQ_E_ARG;
    if (c->bwa_resident) return fail(c, SQ_E_ARG, "the record cache is a STAR-mode file: the resident table of this context is a --bwa batch (sq_bwa_on_device)");
    HostBatch hb;
    int rc = dev_download_records(c, hb);
    if (rc) return rc;
    const size_t n = hb.refid.size(), nb = hb.b_refpos.size();
    if (hb.blk_off.size() != n + 1) hb.blk_off.assign(n + 1, 0);  // (no record: the offsets array is just {0})
    const CacheHeader h = cache_header(c, (int64_t)n, (int64_t)nb);
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(c, SQ_E_IO, std::string("cannot write ") + path);
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
    static const char zeros[64] = {0};
    auto put = [&](const void* p, size_t bytes) {
        if (bytes) ok = ok && std::fwrite(p, 1, bytes, f) == bytes;
        if (pad64(bytes) > bytes) ok = ok && std::fwrite(zeros, 1, pad64(bytes) - bytes, f) == pad64(bytes) - bytes;
    };
    put(hb.refid.data(), n * 4); put(hb.pos.data(), n * 4); put(hb.mrefid.data(), n * 4); put(hb.mpos.data(), n * 4); put(hb.endpos.data(), n * 4);
    put(hb.flag.data(), n * 2); put(hb.totlen.data(), n * 2); put(hb.mapq.data(), n); put(hb.aux.data(), n); put(hb.blk_off.data(), (n + 1) * 4);
    put(hb.b_refpos.data(), nb * 4); put(hb.b_matchref.data(), nb * 4); put(hb.b_readpos.data(), nb * 2); put(hb.b_matchread.data(), nb * 2);
    ok = std::fclose(f) == 0 && ok;
    if (!ok) return fail(c, SQ_E_IO, std::string("short write to ") + path);
    return SQ_OK;
}
static int sq_load_records_impl(sq_ctx* c, const char* path) {
    if (!c || !path) return SQ_E_ARG;
    if (c->ref_len.empty()) return fail(c, SQ_E_ARG, "sq_set_references first");
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(c, SQ_E_IO, std::string("cannot open ") + path);
    CacheHeader h;
    if (std::fread(&h, sizeof h, 1, f) != 1 || std::memcmp(h.magic, "SQSOA1\0", 8) != 0 || h.n_rec < 0 || h.n_blk < 0) { std::fclose(f); return fail(c, SQ_E_IO, std::string(path) + " is not a record cache"); }
    if (c->counts.n_concordant != 0) { std::fclose(f); return fail(c, SQ_E_ARG, "sq_load_records on a context that already holds concordant records"); }
    const CacheHeader want = cache_header(c, h.n_rec, h.n_blk);
    if ((h.reserved[0] || h.reserved[1]) && (want.reserved[0] || want.reserved[1]) && (h.reserved[0] != want.reserved[0] || h.reserved[1] != want.reserved[1])) {
        std::fclose(f);
        return fail(c, SQ_E_ARG, "record cache was written from another concordant BAM (size or modification time differ)");
    }
    if (h.phred_type != want.phred_type || h.min_phred != want.min_phred || h.max_lowphred_len != want.max_lowphred_len || h.n_ref != want.n_ref || h.chim_hash != want.chim_hash) {
        std::fclose(f);
        return fail(c, SQ_E_ARG, "record cache was written with other -pt/-pl/-pm, another reference list or another chimeric BAM");
    }
    // in pieces of 16 M records: bounded host memory whatever the size of the cache
    const size_t n = (size_t)h.n_rec, nb = (size_t)h.n_blk;
    size_t at = sizeof h;
    const size_t o_refid = at; at += pad64(n * 4);
    const size_t o_pos = at; at += pad64(n * 4);
    const size_t o_mrefid = at; at += pad64(n * 4);
    const size_t o_mpos = at; at += pad64(n * 4);
    const size_t o_endpos = at; at += pad64(n * 4);
    const size_t o_flag = at; at += pad64(n * 2);
    const size_t o_totlen = at; at += pad64(n * 2);
    const size_t o_mapq = at; at += pad64(n);
    const size_t o_aux = at; at += pad64(n);
    const size_t o_blkoff = at; at += pad64((n + 1) * 4);
    const size_t o_brefpos = at; at += pad64(nb * 4);
    const size_t o_bmatchref = at; at += pad64(nb * 4);
    const size_t o_breadpos = at; at += pad64(nb * 2);
    const size_t o_bmatchread = at;
    bool ok = true;
    auto get = [&](void* dst, size_t off, size_t bytes) { if (bytes) ok = ok && fseeko(f, (off_t)off, SEEK_SET) == 0 && std::fread(dst, 1, bytes, f) == bytes; };
    const size_t piece = (size_t)1 << 24;
    HostBatch hb;
    int rc = SQ_OK;
    for (size_t r0 = 0; r0 < n && ok && rc == SQ_OK; r0 += piece) {
        const size_t r1 = std::min(n, r0 + piece), k = r1 - r0;
        hb.clear();
        hb.refid.resize(k); hb.pos.resize(k); hb.mrefid.resize(k); hb.mpos.resize(k); hb.endpos.resize(k); hb.flag.resize(k); hb.totlen.resize(k); hb.mapq.resize(k); hb.aux.resize(k); hb.blk_off.resize(k + 1);
        get(hb.refid.data(), o_refid + r0 * 4, k * 4); get(hb.pos.data(), o_pos + r0 * 4, k * 4); get(hb.mrefid.data(), o_mrefid + r0 * 4, k * 4); get(hb.mpos.data(), o_mpos + r0 * 4, k * 4);
        get(hb.endpos.data(), o_endpos + r0 * 4, k * 4); get(hb.flag.data(), o_flag + r0 * 2, k * 2); get(hb.totlen.data(), o_totlen + r0 * 2, k * 2); get(hb.mapq.data(), o_mapq + r0, k);
        get(hb.aux.data(), o_aux + r0, k); get(hb.blk_off.data(), o_blkoff + r0 * 4, (k + 1) * 4);
        if (!ok) break;
        const uint32_t bo0 = hb.blk_off[0], bo1 = hb.blk_off[k];
        if (bo1 < bo0 || bo1 > nb) { ok = false; break; }
        const size_t kb = bo1 - bo0;
        hb.b_refpos.resize(kb); hb.b_matchref.resize(kb); hb.b_readpos.resize(kb); hb.b_matchread.resize(kb);
        get(hb.b_refpos.data(), o_brefpos + (size_t)bo0 * 4, kb * 4); get(hb.b_matchref.data(), o_bmatchref + (size_t)bo0 * 4, kb * 4);
        get(hb.b_readpos.data(), o_breadpos + (size_t)bo0 * 2, kb * 2); get(hb.b_matchread.data(), o_bmatchread + (size_t)bo0 * 2, kb * 2);
        if (!ok) break;
        for (uint32_t& o : hb.blk_off) o -= bo0;
        sq_aln_batch b;
        hb.view(&b, false);
        rc = sq_ingest_concordant(c, &b);
    }
    std::fclose(f);
    if (!ok) return fail(c, SQ_E_IO, std::string("truncated or corrupt record cache ") + path);
    return rc;
}
int sq_load_records(sq_ctx* c, const char* path) { return abi_guard(c, "sq_load_records", [&]() { return sq_load_records_impl(c, path); }); }
static int sq_build_graph_impl(sq_ctx* c) {
    if (!c) return SQ_E_ARG;
    if (c->ref_len.empty()) return fail(c, SQ_E_ARG, "sq_set_references first");
    if (c->read_len <= 0 && !c->bwa) return fail(c, SQ_E_ARG, "sq_ingest_chimeric first (ReadLen comes from the chimeric BAM)");
    if (c->shard.on != (c->P.world_size > 1)) return fail(c, SQ_E_ARG, "world_size > 1 needs sq_set_shard (and the other way round)");
    if (c->bp_future.valid()) (void)c->bp_future.get();
    if (!c->gb) { dev_chim_drop_pending(c); c->chim_s2_pending = false; }
    if (!c->gb && !c->timer_keep) c->timer.clear();
    if (!c->gb) c->ablated = false;
    c->stage_view = false;
    int rc = c->bwa ? build_graph_bwa(c) : build_graph(c);
    dev_flush_timers(c);
    if (rc <= 0 && c->ablated) {  // (the timers of the run stay readable; its graph does not exist -- whatever the mutilated pass ran into)
        if (c->bp_future.valid()) (void)c->bp_future.get();
        c->graph_built = false;
        rc = fail(c, SQ_E_ARG, "a timing-only switch (SQUID_P1_ABLATE / SQUID_EDGES_ABLATE) is set: the graph of this run is wrong and is not handed out");
    }
    if (rc < 0) { c->gb.reset(); c->x_pending = false; }
    return rc;
}
int sq_build_graph(sq_ctx* c) { return abi_guard(c, "sq_build_graph", [&]() { return sq_build_graph_impl(c); }); }
int sq_graph_view(sq_ctx* c, int32_t stage, sq_graph* g) {
    if (!c || !g || stage < 0 || stage > 5 || (!c->graph_built && !c->stage_view)) return SQ_E_ARG;
    if (stage != 0 && !c->keep_stages && !c->stage_view) return fail(c, SQ_E_ARG, "the intermediate graphs were not kept (sq_keep_stage_graphs(ctx, 0) before sq_build_graph)");
    c->snap[stage].view(g);
    return SQ_OK;
}
static int sq_order_impl(sq_ctx* c, sq_orders* o) {
    if (!c || !c->graph_built) return SQ_E_ARG;
    if (!c->ordered) { int rc = order_components(c); dev_flush_timers(c); if (rc) return rc; }
    if (o) { o->n_components = (int32_t)c->ord_off.size() - 1; o->comp_off = c->ord_off.data(); o->nodes = c->ord_nodes.data(); }
    return SQ_OK;
}
int sq_order(sq_ctx* c, sq_orders* o) { return abi_guard(c, "sq_order", [&]() { return sq_order_impl(c, o); }); }
static int sq_total_order_impl(sq_ctx* c, sq_orders* o) {
    if (!c || !o || !c->graph_built) return SQ_E_ARG;
    if (!c->ordered) { int rc = order_components(c); dev_flush_timers(c); if (rc) return rc; }
    const int rc = total_order(c);
    if (rc) return rc;
    o->n_components = (int32_t)c->tot_off.size() - 1; o->comp_off = c->tot_off.data(); o->nodes = c->tot_nodes.data();
    return SQ_OK;
}
int sq_total_order(sq_ctx* c, sq_orders* o) { return abi_guard(c, "sq_total_order", [&]() { return sq_total_order_impl(c, o); }); }
static int sq_call_sv_impl(sq_ctx* c, sq_sv_table* t) {
    if (!c || !c->graph_built) return SQ_E_ARG;
    int rc = call_sv(c);
    dev_flush_timers(c);
    if (rc < 0) { c->svb.reset(); c->x_pending = false; }
    if (rc) return rc;
    if (t) {
        t->n_rows = (int32_t)c->sv_cols[0].size();
        t->chr1 = c->sv_cols[0].data(); t->start1 = c->sv_cols[1].data(); t->end1 = c->sv_cols[2].data();
        t->chr2 = c->sv_cols[3].data(); t->start2 = c->sv_cols[4].data(); t->end2 = c->sv_cols[5].data();
        t->score = c->sv_cols[6].data(); t->sup1 = c->sv_cols[7].data(); t->sup2 = c->sv_cols[8].data();
        t->strand1_minus = c->sv_s1.data(); t->strand2_minus = c->sv_s2.data();
    }
    return SQ_OK;
}
int sq_call_sv(sq_ctx* c, sq_sv_table* t) { return abi_guard(c, "sq_call_sv", [&]() { return sq_call_sv_impl(c, t); }); }
static int sq_breakpoints_impl(sq_ctx* c, sq_bp_table* t) {
    if (!c || !t || c->bp_off.empty()) return SQ_E_ARG;
    t->n_edges = (int32_t)c->bp_off.size() - 1;
    t->bp_off = c->bp_off.data(); t->bp1 = c->bp1.data(); t->bp2 = c->bp2.data(); t->sup1 = c->bsup1.data(); t->sup2 = c->bsup2.data();
    return SQ_OK;
}
int sq_breakpoints(sq_ctx* c, sq_bp_table* t) { return abi_guard(c, "sq_breakpoints", [&]() { return sq_breakpoints_impl(c, t); }); }
int sq_debug_token_bench(sq_ctx* c, const char* path, int32_t variant, int32_t max_blocks, int32_t reps, int32_t check, double* out7) {
    if (!c || !path || !out7 || max_blocks <= 0 || reps <= 0) return SQ_E_ARG;
    return abi_guard(c, "sq_debug_token_bench", [&]() { return dev_token_bench(c, path, variant, max_blocks, reps, check, out7); });
}
int sq_get_timing(sq_ctx* c, sq_timing* t) {
    if (!c || !t) return SQ_E_ARG;
    t->n = (int32_t)c->timer.names.size();
    t->names = c->timer.names.data(); t->ms = c->timer.ms.data(); t->launches = c->timer.launches.data(); t->bytes = c->timer.bytes.data(); t->busy_ms = c->timer.busy.data();
    return SQ_OK;
}
int sq_drop_file_cache(void) { drop_file_cache(); return SQ_OK; }
int sq_release_reader_buffers(sq_ctx* c) {
    if (!c) return SQ_E_ARG;
    c->staged_path.clear(); c->staged_bytes = 0;
    drop_whole_file_scratch();
    if (!c->chim_future.valid()) c->chim_decoded.reset();  // (a pairing still running reads it)
    c->bwa_spare.reset();
    return dev_release_reader(c);
}
int sq_keep_stage_graphs(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->keep_stages = on != 0;
    return SQ_OK;
}
int sq_keep_host_memory(void) {
    // (mallopt takes ints: the thresholds stop at 2 GiB - 1; thread arenas -- where the context's host threads allocate -- are kept
    // whole by the top pad: an arena heap is only unmapped when more than the pad would stay free in the one before it)
    const int ok = mallopt(M_TRIM_THRESHOLD, INT32_MAX) & mallopt(M_TOP_PAD, INT32_MAX & ~4095) & mallopt(M_MMAP_THRESHOLD, 32 << 20);
    return ok ? SQ_OK : SQ_E_ARG;
}
int sq_timing_accumulate(sq_ctx* c, int32_t keep) {
    if (!c) return SQ_E_ARG;
    c->timer_keep = keep != 0;
    if (keep) c->timer.clear();
    return SQ_OK;
}
int sq_reset(sq_ctx* c) {
    if (!c) return SQ_E_ARG;
    if (c->bp_future.valid()) (void)c->bp_future.get();
    dev_chim_drop_pending(c);
    c->chim_s2_pending = false; c->chim_s1_device = false;
    c->bwa_dev_active = false;  // (the table stays resident: bwa_resident)
    copy_frags(c, c->frags0, c->frags);  // the graph stages trim the chimeric blocks in place, like the reference does
    c->nodes.clear(); c->edges.clear(); c->label.clear();
    c->graph_built = false; c->ordered = false; c->stage_view = false;
    c->bp_off.clear();
    c->gb.reset(); c->svb.reset(); c->x_pending = false; c->x_ready = false;
    return SQ_OK;
}
int sq_get_counts(sq_ctx* c, sq_counts* k) {
    if (!c || !k) return SQ_E_ARG;
    *k = c->counts;
    k->replay_candidates_checked = c->replay_checked.load(); k->replay_count_mismatches = c->replay_mismatch.load();
    return SQ_OK;
}
int sq_debug_download(sq_ctx* c, sq_aln_batch* b) {
    if (!c || !b) return SQ_E_ARG;
    static thread_local HostBatch hb;
    int rc = dev_download_records(c, hb);
    if (rc) return rc;
    hb.view(b, false);
    return SQ_OK;
}
int sq_debug_bp_support(sq_ctx* c, int32_t n_bp, const int32_t* chr, const int32_t* pos, int32_t* coverage, int32_t host_walk) {
    if (!c || n_bp < 0 || (n_bp && (!chr || !pos || !coverage))) return SQ_E_ARG;
    if (!c->graph_built) return fail(c, SQ_E_ARG, "sq_debug_bp_support before sq_build_graph");
    std::vector<std::pair<int, int>> bps(n_bp);
    for (int i = 0; i < n_bp; ++i) bps[i] = {chr[i], pos[i]};
    if (!std::is_sorted(bps.begin(), bps.end())) return fail(c, SQ_E_ARG, "breakpoints must be sorted by (chr, pos)");
    std::vector<int32_t> cov;
    int rc;
    if (c->bwa && c->bwa_dev_active) rc = host_walk ? bwa_breakpoint_support(c, bps, cov, false) : bwa_breakpoint_support_device(c, bps, cov, false);  // (sq_bwa_on_device: the host loop / the kernels over the same batch)
    else rc = host_walk ? dev_breakpoint_support_exact(c, bps, cov) : dev_breakpoint_support(c, bps, cov);
    dev_flush_timers(c);
    if (rc) return rc;
    std::copy(cov.begin(), cov.end(), coverage);
    return SQ_OK;
}
int sq_chimeric_on_device(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->chim_dev_asked = on != 0;  // (a --bwa context keeps the host route: chim_dev_on)
    return SQ_OK;
}
int sq_bwa_on_device(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->bwa_dev_asked = on != 0;  // (only a --bwa context looks at it: bwa_dev_on)
    return SQ_OK;
}
int sq_bwa_edges_on_device(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->bwa_edges_asked = on != 0;  // (only a --bwa context looks at it: bwa_edges_on)
    return SQ_OK;
}
int sq_segment_on_device(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->seg_dev_asked = on != 0;  // (a --bwa context and a sharded one keep their host routes: seg_dev_on)
    return SQ_OK;
}
int sq_compress_windows_on_device(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->fc_windows_asked = on != 0;  // (every context looks at it: fc_windows_on)
    return SQ_OK;
}
static int segment_debug_view(sq_ctx* c, SegPlan& plan, int read_len, int32_t route, sq_segment_debug* out) {
    static thread_local SegSeedsDebug R;
    std::memset(out, 0, sizeof *out);
    const int rc = segment_seeds_debug(c, plan, read_len, route, nullptr, R);
    dev_flush_timers(c);
    if (rc) return rc;
    out->n_seeds = (int64_t)R.seeds3.size() / 3; out->seeds3 = R.seeds3.data();
    out->stretches = R.walk.stretches; out->again = R.walk.again; out->longest = R.walk.longest; out->sens = R.walk.sens; out->extended = R.walk.extended;
    out->kept_with_nodes = R.walk.kept_with_nodes; out->flagged = R.walk.flagged; out->fallback = R.fallback ? 1 : 0;
    return SQ_OK;
}
int sq_debug_segment_seeds(sq_ctx* c, int32_t route, sq_segment_debug* out) {
    if (!c || !out || (route != 0 && route != 1)) return SQ_E_ARG;
    return abi_guard(c, "sq_debug_segment_seeds", [&]() -> int {
        if (c->bwa) return fail(c, SQ_E_ARG, "sq_debug_segment_seeds needs a STAR context");
        std::shared_ptr<SegPlan> plan;
        const int rc = segment_plan_of_context(c, plan);
        if (rc) return rc;
        return segment_debug_view(c, *plan, 0, route, out);
    });
}
int sq_debug_segment_seeds_tables(sq_ctx* c, int32_t route, int32_t read_len, int64_t n_recs, const int32_t* recs6, int32_t n_disc, const int32_t* disc4, int32_t n_part, const int32_t* part2,
                                  int32_t n_clusters, const int32_t* rest_off, const int32_t* rest_pos, const int32_t* rest_len, const int32_t* trigger, int32_t n_zero, const int32_t* zero3,
                                  sq_segment_debug* out) {
    if (!c || !out || (route != 0 && route != 1) || read_len <= 0 || n_recs < 0 || n_disc < 0 || n_part < 0 || n_clusters < 0 || n_zero < 0 || (n_recs && !recs6) || (n_disc && !disc4) || (n_part && !part2) || !rest_off ||
        (n_clusters && !trigger) || (n_zero && !zero3))
        return SQ_E_ARG;
    return abi_guard(c, "sq_debug_segment_seeds_tables", [&]() -> int {
        std::vector<int32_t> cl4;
        segment_clusters_of_tables(read_len, n_disc, disc4, cl4);
        if ((int64_t)cl4.size() != 4 * (int64_t)n_clusters) return fail(c, SQ_E_ARG, "sq_debug_segment_seeds_tables: the blocks make " + std::to_string(cl4.size() / 4) + " clusters, not n_clusters");
        if (rest_off[n_clusters] && (!rest_pos || !rest_len)) return SQ_E_ARG;
        std::vector<StreamRec> recs((size_t)n_recs);
        for (int64_t i = 0; i < n_recs; ++i) {
            const int32_t* q = recs6 + 6 * i;
            StreamRec r{};
            r.refid = q[0]; r.pos = q[1]; r.fb_refpos = q[2]; r.fb_matchref = q[3]; r.fb_readpos = (uint16_t)q[4]; r.flags = (uint8_t)q[5];
            recs[(size_t)i] = r;
        }
        SegTablesIn in;
        in.read_len = read_len; in.n_recs = n_recs; in.recs = recs.data(); in.n_disc = n_disc; in.disc4 = disc4; in.n_part = n_part; in.part2 = part2;
        in.rest_off = rest_off; in.rest_pos = rest_pos; in.rest_len = rest_len; in.trigger = trigger; in.n_zero = n_zero; in.zero3 = zero3;
        std::shared_ptr<SegPlan> plan;
        const int rc = segment_plan_from_tables(c, in, plan);
        if (rc) return rc;
        return segment_debug_view(c, *plan, read_len, route, out);
    });
}
int sq_bwa_nodes_on_device(sq_ctx* c, int32_t on) {
    if (!c) return SQ_E_ARG;
    c->bwa_nodes_asked = on != 0;  // (only a --bwa context looks at it: bwa_nodes_on)
    return SQ_OK;
}
// the record tables of the debug entries as a batch of the library's own layout
static int batch_from_tables(sq_ctx* c, const char* who, int64_t n_rec, const int32_t* rec8, const uint32_t* blk_off, const int32_t* blk4, HostBatch& hb) {
    if (blk_off[0] != 0) return fail(c, SQ_E_ARG, std::string(who) + ": blk_off must start at 0");
    for (int64_t r = 0; r < n_rec; ++r) if (blk_off[r + 1] < blk_off[r]) return fail(c, SQ_E_ARG, std::string(who) + ": blk_off must not go down");
    const size_t nb = blk_off[n_rec];
    if (nb && !blk4) return SQ_E_ARG;
    for (int64_t r = 0; r < n_rec; ++r) {
        const int32_t* q = rec8 + 8 * r;
        hb.refid.push_back(q[0]); hb.pos.push_back(q[1]); hb.mrefid.push_back(q[2]); hb.mpos.push_back(q[3]); hb.endpos.push_back(q[1]);
        hb.flag.push_back((uint16_t)q[4]); hb.totlen.push_back((uint16_t)q[5]); hb.mapq.push_back((uint8_t)q[6]); hb.aux.push_back((uint8_t)q[7]);
    }
    hb.blk_off.assign(blk_off, blk_off + n_rec + 1);
    hb.name_off.assign((size_t)n_rec + 1, 0);
    for (size_t b = 0; b < nb; ++b) { hb.b_refpos.push_back(blk4[4 * b]); hb.b_matchref.push_back(blk4[4 * b + 1]); hb.b_readpos.push_back((uint16_t)blk4[4 * b + 2]); hb.b_matchread.push_back((uint16_t)blk4[4 * b + 3]); }
    return SQ_OK;
}
static int bwa_nodes_debug_view(sq_ctx* c, const HostBatch* tables, int32_t route, sq_bwa_nodes_debug* out) {
    static thread_local BwaNodesDebug R;
    std::memset(out, 0, sizeof *out);
    const int rc = bwa_seed_nodes_debug(c, tables, route, R);
    dev_flush_timers(c);
    if (rc) return rc;
    out->n_seeds = (int64_t)R.seeds3.size() / 3; out->seeds3 = R.seeds3.data();
    out->n_reads_records = R.n_reads_records; out->stretches = R.stretches; out->again = R.again; out->single = R.single; out->longest = R.longest;
    out->flush_nodes = R.flush_nodes; out->marks_closed = R.marks_closed; out->read_len = R.read_len; out->fallback = R.fallback ? 1 : 0;
    return SQ_OK;
}
int sq_debug_bwa_seed_nodes(sq_ctx* c, int32_t route, sq_bwa_nodes_debug* out) {
    if (!c || !out || (route != 0 && route != 1)) return SQ_E_ARG;
    return abi_guard(c, "sq_debug_bwa_seed_nodes", [&]() -> int {
        if (!c->bwa) return fail(c, SQ_E_ARG, "sq_debug_bwa_seed_nodes needs a --bwa context behind sq_ingest_bwa_file");
        return bwa_nodes_debug_view(c, nullptr, route, out);
    });
}
int sq_debug_bwa_seed_nodes_tables(sq_ctx* c, int32_t route, int32_t read_len, int64_t n_rec, const int32_t* rec8, const uint32_t* blk_off, const int32_t* blk4, sq_bwa_nodes_debug* out) {
    if (!c || !out || (route != 0 && route != 1) || read_len < 0 || n_rec < 0 || !blk_off || (n_rec && !rec8)) return SQ_E_ARG;
    return abi_guard(c, "sq_debug_bwa_seed_nodes_tables", [&]() -> int {
        HostBatch hb;
        const int rc = batch_from_tables(c, "sq_debug_bwa_seed_nodes_tables", n_rec, rec8, blk_off, blk4, hb);
        if (rc) return rc;
        const int kept = c->read_len;  // (the loop starts from the caller's value; the context keeps its own)
        c->read_len = read_len;
        const int rc2 = bwa_nodes_debug_view(c, &hb, route, out);
        c->read_len = kept;
        return rc2;
    });
}
static int bwa_edges_debug_view(sq_ctx* c, const HostBatch* tables, const std::vector<Node>& N, int32_t route, sq_bwa_edges_debug* out) {
    static thread_local BwaEdgesDebug R;
    std::memset(out, 0, sizeof *out);
    const int rc = bwa_raw_edges_debug(c, tables, N, route, R);
    dev_flush_timers(c);
    if (rc) return rc;
    out->n_edges = (int64_t)R.keys.size(); out->keys = (const uint64_t*)R.keys.data(); out->weights = R.weights.data();
    out->n_part = (int64_t)R.part.size(); out->n_first_dis = (int64_t)R.first_dis.size(); out->n_second = (int64_t)R.second.size();
    out->part = R.part.data(); out->first_dis = R.first_dis.data(); out->second = R.second.data(); out->second_keys = (const uint64_t*)R.second_keys.data();
    out->n_emitted = R.n_emitted; out->n_soft = R.n_soft; out->final_pos = R.final_pos; out->fallback = R.fallback ? 1 : 0;
    return SQ_OK;
}
int sq_debug_bwa_raw_edges(sq_ctx* c, int32_t route, sq_bwa_edges_debug* out) {
    if (!c || !out || (route != 0 && route != 1)) return SQ_E_ARG;
    return abi_guard(c, "sq_debug_bwa_raw_edges", [&]() -> int {
        if (!c->bwa || !c->graph_built) return fail(c, SQ_E_ARG, "sq_debug_bwa_raw_edges needs a --bwa context behind sq_build_graph");
        const GraphSnap& g = c->snap[1];
        if (g.chr.empty()) return fail(c, SQ_E_ARG, "sq_debug_bwa_raw_edges needs the stage graphs (sq_keep_stage_graphs)");
        std::vector<Node> N(g.chr.size());
        for (size_t i = 0; i < N.size(); ++i) N[i] = Node{g.chr[i], g.pos[i], g.len[i], 0, 0.0};
        return bwa_edges_debug_view(c, nullptr, N, route, out);
    });
}
int sq_debug_bwa_raw_edges_tables(sq_ctx* c, int32_t route, int32_t n_nodes, const int32_t* nodes3, int64_t n_rec, const int32_t* rec8, const uint32_t* blk_off, const int32_t* blk4,
                                  sq_bwa_edges_debug* out) {
    if (!c || !out || (route != 0 && route != 1) || n_nodes < 0 || n_rec < 0 || (n_nodes && !nodes3) || !blk_off || (n_rec && !rec8)) return SQ_E_ARG;
    return abi_guard(c, "sq_debug_bwa_raw_edges_tables", [&]() -> int {
        std::vector<Node> N((size_t)n_nodes);
        for (int32_t i = 0; i < n_nodes; ++i) {
            N[(size_t)i] = Node{nodes3[3 * i], nodes3[3 * i + 1], nodes3[3 * i + 2], 0, 0.0};
            if (N[(size_t)i].chr < 0 || (i && N[(size_t)i].chr < N[(size_t)i - 1].chr)) return fail(c, SQ_E_ARG, "sq_debug_bwa_raw_edges_tables: node chromosomes must be non-negative and sorted");
        }
        HostBatch hb;
        const int rc = batch_from_tables(c, "sq_debug_bwa_raw_edges_tables", n_rec, rec8, blk_off, blk4, hb);
        if (rc) return rc;
        if (n_nodes == 0 && n_rec != 0) return fail(c, SQ_E_ARG, "sq_debug_bwa_raw_edges_tables: records need a node table");
        return bwa_edges_debug_view(c, &hb, N, route, out);
    });
}
static int sq_debug_bwa_depth_impl(sq_ctx* c, int32_t route, int32_t n_nodes, const int32_t* nodes3, int64_t n_reads, const int32_t* reads3, int32_t* support, int32_t* sums, int64_t* out2) {
    if (n_nodes < 0 || n_reads < 0 || (n_nodes && (!nodes3 || !support || !sums)) || (n_reads && !reads3) || !out2 || (route != 0 && route != 1) || (route == 1 && !c)) return SQ_E_ARG;
    std::vector<int32_t> cnts, sm;
    int64_t held = 0;
    bool fallback = false;
    if (route == 0) bwa_node_depth_flat(n_nodes, nodes3, n_reads, reads3, cnts, sm);  // (the loop itself: no cursor restated, nothing held to count)
    else {
        const int rc = dev_bwa_node_depth_flat(c, n_nodes, nodes3, n_reads, reads3, cnts, sm, held, fallback);
        dev_flush_timers(c);
        if (rc) return rc;
    }
    for (int32_t i = 0; i < n_nodes; ++i) { support[i] = cnts[(size_t)i]; sums[i] = sm[(size_t)i]; }
    out2[0] = held; out2[1] = fallback ? 1 : 0;
    return SQ_OK;
}
int sq_debug_bwa_depth(sq_ctx* c, int32_t route, int32_t n_nodes, const int32_t* nodes3, int64_t n_reads, const int32_t* reads3, int32_t* support, int32_t* sums, int64_t* out2) {
    return abi_guard(c, "sq_debug_bwa_depth", [&]() { return sq_debug_bwa_depth_impl(c, route, n_nodes, nodes3, n_reads, reads3, support, sums, out2); });
}
static int sq_debug_chim_stages_impl(sq_ctx* c, int32_t n1, const int32_t* nodes1, int32_t n2, const int32_t* nodes2, int32_t n_frag, const int32_t* frag_off, const int32_t* frag_na,
                                     const int32_t* frag_tot, const int32_t* blocks6, int32_t n_edges, const int32_t* edges4, int64_t* out8) {
    if (!c || n1 <= 0 || n2 <= 0 || n_frag < 0 || n_edges < 0 || !nodes1 || !nodes2 || !frag_off || !frag_na || !frag_tot || !blocks6 || (n_edges && !edges4) || !out8) return SQ_E_ARG;
    if (c->bp_future.valid()) (void)c->bp_future.get();
    dev_chim_drop_pending(c);
    c->chim_s2_pending = false; c->chim_s1_device = false; c->graph_built = false; c->stage_view = false;
    std::vector<Frag> F0((size_t)n_frag);
    for (int32_t q = 0; q < n_frag; ++q) {
        const int32_t o = frag_off[q], e = frag_off[q + 1], na = frag_na[q];
        if (o < 0 || e < o || na < 0 || na > e - o) return fail(c, SQ_E_ARG, "sq_debug_chim_stages: malformed fragment table");
        Frag& f = F0[(size_t)q];
        f.atot = frag_tot[2 * q]; f.btot = frag_tot[2 * q + 1];
        for (int32_t k = o; k < e; ++k) {
            const int32_t* b = blocks6 + 6 * (size_t)k;
            (k < o + na ? f.a : f.b).push_back(Blk{b[0], b[1], b[2], b[3], b[4], b[5] != 0, k < o + na});
        }
    }
    auto nodes_of = [](int32_t n, const int32_t* v) { std::vector<Node> N((size_t)n); for (int32_t i = 0; i < n; ++i) N[(size_t)i] = Node{v[3 * i], v[3 * i + 1], v[3 * i + 2], 0, 0.0}; return N; };
    const std::vector<Node> N1 = nodes_of(n1, nodes1), N2 = nodes_of(n2, nodes2);
    std::vector<Edge> E((size_t)n_edges);
    for (int32_t i = 0; i < n_edges; ++i) {
        const int32_t* e = edges4 + 4 * (size_t)i;
        if (e[0] < 0 || e[1] < e[0] || e[1] >= n2) return fail(c, SQ_E_ARG, "sq_debug_chim_stages: edge outside the node table");
        E[(size_t)i] = make_edge(e[0], e[2] != 0, e[1], e[3] != 0);
    }
    auto same_blocks = [](const std::vector<Frag>& x, const std::vector<Frag>& y) {
        int64_t bad = 0;
        for (size_t q = 0; q < x.size(); ++q)
            for (int mate = 0; mate < 2; ++mate) {
                const BlkList &p = mate ? x[q].b : x[q].a, &r = mate ? y[q].b : y[q].a;
                for (size_t k = 0; k < p.size(); ++k) if (p[k].refpos != r[k].refpos || p[k].readpos != r[k].readpos || p[k].matchref != r[k].matchref || p[k].matchread != r[k].matchread) ++bad;
            }
        return bad;
    };
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    // host route
    c->frags = F0; c->frags0 = F0; ++c->frags_version;
    c->nodes = N1;
    out8[1] = chim_stage_soft_count(c, N1, 1);
    std::vector<Edge> raw_h, red_h, raw_d, red_d;
    BPMap bp_h, bp_d;
    std::vector<Frag> h1, h2;
    int rc_h = chimeric_edges(c, raw_h);
    if (!rc_h) {
        reduce_edges(raw_h, red_h);
        h1 = c->frags;
        c->nodes = N2; c->edges = E;
        out8[2] = chim_stage_soft_count(c, N2, 2);
        rc_h = exact_breakpoints(c, bp_h);
        h2 = c->frags;
    }
    out8[5] = rc_h;
    c->err.clear();
    // device route
    auto soft_seen = [&]() { for (size_t t = 0; t < c->timer.names.size(); ++t) if (!std::strcmp(c->timer.names[t], "chim_soft_fragments")) return c->timer.launches[t]; return (int64_t)0; };
    c->timer.clear();
    c->frags = F0;
    c->nodes = N1;
    bool fb = false;
    int rc_d = dev_chimeric_edges(c, raw_d, fb);
    if (!rc_d && fb) return fail(c, SQ_E_CAPACITY, "sq_debug_chim_stages: the device route handed stage 1 back to the host");
    out8[3] = soft_seen();
    if (!rc_d) {
        reduce_edges(raw_d, red_d);
        if ((rc_d = dev_chim_download_trimmed(c))) return rc_d;
        if (!rc_h) out8[0] += same_blocks(h1, c->frags);
        c->frags = F0;
        c->nodes = N2; c->edges = E;
        rc_d = dev_exact_breakpoints_start(c, fb);
        if (!rc_d && fb) return fail(c, SQ_E_CAPACITY, "sq_debug_chim_stages: the device route handed stage 2 back to the host");
        if (!rc_d) rc_d = dev_exact_breakpoints_collect(c, bp_d);
        out8[4] = soft_seen() - out8[3];
        if (!rc_d) { const int r3 = dev_chim_download_trimmed(c); if (r3) return r3; if (!rc_h) out8[0] += same_blocks(h2, c->frags); }
    }
    dev_flush_timers(c);
    out8[6] = rc_d;
    c->err.clear();
    if (rc_h != rc_d) out8[0] += 1;
    if (!rc_h && !rc_d) {
        if (red_h.size() != red_d.size()) out8[0] += 1;
        for (size_t i = 0; i < std::min(red_h.size(), red_d.size()); ++i) if (!edge_key_eq(red_h[i], red_d[i]) || red_h[i].w != red_d[i].w) out8[0] += 1;
        for (const Edge& e : E) {  // (call_sv only ever looks up the keys of final edges)
            const BPMap::const_iterator a = bp_h.find(edge_pack(e)), b = bp_d.find(edge_pack(e));
            const bool ha = a != bp_h.end(), hb = b != bp_d.end();
            if (ha != hb || (ha && a->second != b->second)) out8[0] += 1;
        }
    }
    c->frags.clear(); c->frags0.clear(); c->nodes.clear(); c->edges.clear(); ++c->frags_version;
    return SQ_OK;
}
int sq_debug_chim_stages(sq_ctx* c, int32_t n1, const int32_t* nodes1, int32_t n2, const int32_t* nodes2, int32_t n_frag, const int32_t* frag_off, const int32_t* frag_na,
                         const int32_t* frag_tot, const int32_t* blocks6, int32_t n_edges, const int32_t* edges4, int64_t* out8) {
    return abi_guard(c, "sq_debug_chim_stages", [&]() { return sq_debug_chim_stages_impl(c, n1, nodes1, n2, nodes2, n_frag, frag_off, frag_na, frag_tot, blocks6, n_edges, edges4, out8); });
}
// (tests) one caller-supplied graph through the small-graph stages, by the calls build_graph / finish_graph make
static int sq_debug_graph_stages_impl(sq_ctx* c, int32_t n_nodes, const int32_t* nodes4, const double* depth3, int32_t n_edges, const int32_t* edges6, const uint8_t* keep_in,
                                      int32_t bounds, int32_t route, int32_t first, int32_t last, const sq_params* params, sq_graph_stages_debug* out) {
    if (!c || !out || n_nodes <= 0 || n_edges < 0 || !nodes4 || !depth3 || (n_edges && !edges6) || route < 0 || route > 1 || first < 0 || last > 4 || first > last) return SQ_E_ARG;
    if (c->bp_future.valid()) (void)c->bp_future.get();
    dev_chim_drop_pending(c);
    c->chim_s2_pending = false; c->chim_s1_device = false; c->graph_built = false; c->ordered = false; c->stage_view = false;
    c->gb.reset();
    std::vector<Node> N((size_t)n_nodes);
    for (int32_t i = 0; i < n_nodes; ++i) {
        const int32_t* v = nodes4 + 4 * (size_t)i;
        const double* d = depth3 + 3 * (size_t)i;
        if (v[2] <= 0 || (i > 0 && (v[0] < nodes4[4 * (size_t)(i - 1)]))) return fail(c, SQ_E_ARG, "sq_debug_graph_stages: node table is not sorted, or holds an empty node");
        N[(size_t)i] = Node{v[0], v[1], v[2], v[3], d[0], d[1], d[2]};
    }
    std::vector<Edge> E((size_t)n_edges);
    for (int32_t i = 0; i < n_edges; ++i) {
        const int32_t* e = edges6 + 6 * (size_t)i;
        if (e[0] < 0 || e[2] < e[0] || e[2] >= n_nodes) return fail(c, SQ_E_ARG, "sq_debug_graph_stages: edge outside the node table");
        Edge& x = E[(size_t)i];
        x.a = e[0]; x.ha = e[1] != 0; x.b = e[2]; x.hb = e[3] != 0; x.w = e[4]; x.gw = e[5];
        if (i > 0 && edge_key_less(x, E[(size_t)i - 1])) return fail(c, SQ_E_ARG, "sq_debug_graph_stages: edges are not sorted by key");
    }
    c->nodes.swap(N); c->edges.swap(E); c->label.clear();
    const sq_params saved = c->P;
    if (params) {  // the five parameters the stages read, for this call only
        c->P.concord_dist_pos = params->concord_dist_pos; c->P.concord_dist_idx = params->concord_dist_idx; c->P.min_edge_weight = params->min_edge_weight;
        c->P.discordant_ratio = params->discordant_ratio; c->P.max_allowed_degree = params->max_allowed_degree;
    }
    c->depth_bounds = bounds != 0; c->depth_ambiguous = false;
    const bool host = route == 0;
    static thread_local std::vector<uint8_t> keep;
    keep.assign((size_t)n_edges, 1);
    if (keep_in) keep.assign(keep_in, keep_in + n_edges);
    *out = sq_graph_stages_debug{0, nullptr, 0, 0, 0};
    auto runs = [&](int k) { return first <= k && k <= last; };
    int rc = SQ_OK;
    bool labelled = false;
    do {
        if (runs(0)) {
            if (host) filter_by_weight(c); else if ((rc = dev_filter_by_weight(c))) break;
            c->snap[3].take(c->nodes, c->edges, nullptr);
        }
        if (runs(1)) { if (host) filter_by_interleaving(c, keep); else if ((rc = dev_filter_by_interleaving(c, keep))) break; }
        if (runs(2)) {
            if (keep.size() != c->edges.size()) { rc = fail(c, SQ_E_ARG, "sq_debug_graph_stages: no KeepEdge column for the edges in front of FilterEdges"); break; }
            if (host) filter_edges(c, keep); else if ((rc = dev_filter_edges(c, keep))) break;
            c->snap[4].take(c->nodes, c->edges, nullptr);
        }
        if (runs(3)) {
            if ((rc = host ? compress_nodes(c) : dev_compress_nodes(c))) break;
            c->snap[5].take(c->nodes, c->edges, nullptr);
        }
        if (runs(4)) {  // (as finish_graph)
            rc = host ? further_compress(c) : dev_further_compress(c);
            if (rc == 2) { out->fallback = 1; rc = further_compress(c); }
            if (rc) break;
            if ((rc = dev_connected_components(c, (int)c->nodes.size(), c->edges, c->label))) break;
            multiply_discordant(c, false);
            labelled = true;
        }
    } while (false);
    dev_flush_timers(c);
    c->P = saved;
    out->n_keep = (int32_t)keep.size(); out->keep = keep.data();
    out->depth_ambiguous = c->depth_ambiguous ? 1 : 0;
    c->depth_bounds = false; c->depth_ambiguous = false;
    if (rc && rc != SQ_E_ASSERT) return rc;
    out->rc = rc;
    c->err.clear();
    c->snap[0].take(c->nodes, c->edges, labelled ? &c->label : nullptr);
    c->nodes.clear(); c->edges.clear(); c->label.clear();
    c->stage_view = true;
    return SQ_OK;
}
int sq_debug_graph_stages(sq_ctx* c, int32_t n_nodes, const int32_t* nodes4, const double* depth3, int32_t n_edges, const int32_t* edges6, const uint8_t* keep_in, int32_t bounds,
                          int32_t route, int32_t first, int32_t last, const sq_params* params, sq_graph_stages_debug* out) {
    return abi_guard(c, "sq_debug_graph_stages", [&]() { return sq_debug_graph_stages_impl(c, n_nodes, nodes4, depth3, n_edges, edges6, keep_in, bounds, route, first, last, params, out); });
}
// (tests) the window table of sq_compress_windows_on_device for one caller-supplied graph as it enters FurtherCompressNode
static int sq_debug_fc_windows_impl(sq_ctx* c, int32_t n_nodes, const int32_t* nodes4, int32_t n_edges, const int32_t* edges6, const sq_params* params, int32_t* n_windows, const int32_t** windows) {
    if (!c || n_nodes <= 0 || n_edges < 0 || !nodes4 || (n_edges && !edges6) || !n_windows || !windows) return SQ_E_ARG;
    if (c->bp_future.valid()) (void)c->bp_future.get();
    dev_chim_drop_pending(c);
    c->chim_s2_pending = false; c->chim_s1_device = false; c->graph_built = false; c->ordered = false; c->stage_view = false;
    c->gb.reset();
    std::vector<Node> N((size_t)n_nodes);
    for (int32_t i = 0; i < n_nodes; ++i) {
        const int32_t* v = nodes4 + 4 * (size_t)i;
        if (v[2] <= 0 || (i > 0 && (v[0] < nodes4[4 * (size_t)(i - 1)]))) return fail(c, SQ_E_ARG, "sq_debug_fc_windows: node table is not sorted, or holds an empty node");
        N[(size_t)i] = Node{v[0], v[1], v[2], v[3], 0.0, 0.0, 0.0};
    }
    std::vector<Edge> E((size_t)n_edges);
    for (int32_t i = 0; i < n_edges; ++i) {
        const int32_t* e = edges6 + 6 * (size_t)i;
        if (e[0] < 0 || e[2] < e[0] || e[2] >= n_nodes) return fail(c, SQ_E_ARG, "sq_debug_fc_windows: edge outside the node table");
        Edge& x = E[(size_t)i];
        x.a = e[0]; x.ha = e[1] != 0; x.b = e[2]; x.hb = e[3] != 0; x.w = e[4]; x.gw = e[5];
        if (i > 0 && edge_key_less(x, E[(size_t)i - 1])) return fail(c, SQ_E_ARG, "sq_debug_fc_windows: edges are not sorted by key");
    }
    c->nodes.swap(N); c->edges.swap(E); c->label.clear();
    const sq_params saved = c->P;
    if (params) { c->P.concord_dist_pos = params->concord_dist_pos; c->P.concord_dist_idx = params->concord_dist_idx; }  // (what IsDiscordant reads, for this call only)
    static thread_local std::vector<int32_t> table;
    const int rc = dev_fc_windows_debug(c, table);
    dev_flush_timers(c);
    c->P = saved;
    c->nodes.clear(); c->edges.clear();
    if (rc) return rc;
    *n_windows = (int32_t)table.size() - 1; *windows = table.data();
    return SQ_OK;
}
int sq_debug_fc_windows(sq_ctx* c, int32_t n_nodes, const int32_t* nodes4, int32_t n_edges, const int32_t* edges6, const sq_params* params, int32_t* n_windows, const int32_t** windows) {
    return abi_guard(c, "sq_debug_fc_windows", [&]() { return sq_debug_fc_windows_impl(c, n_nodes, nodes4, n_edges, edges6, params, n_windows, windows); });
}
int sq_debug_order(sq_ctx* c, int32_t n, int32_t n_edges, const int32_t* edges5, int32_t use_gpu, int32_t* mask, int32_t* order, int64_t* value) {
    if (!c || n_edges < 0 || (n_edges && !edges5) || !mask || !order || !value) return SQ_E_ARG;
    std::vector<int32_t> e(edges5, edges5 + 5 * (size_t)n_edges), o;
    int32_t m = 0; int64_t v = 0;
    int rc = order_problem_debug(c, n, e, use_gpu != 0, m, o, v);
    dev_flush_timers(c);
    if (rc) return rc;
    *mask = m; *value = v;
    std::copy(o.begin(), o.end(), order);
    return SQ_OK;
}
int sq_debug_blocks(int32_t n, const int32_t* f, uint8_t* rel5, int32_t* perm_pos, int32_t* perm_readpos) {
    if (n < 0 || (n && (!f || !rel5 || !perm_pos || !perm_readpos))) return SQ_E_ARG;
    std::vector<Blk> v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = Blk{f[7 * i], f[7 * i + 1], f[7 * i + 2], f[7 * i + 3], f[7 * i + 4], f[7 * i + 5] != 0, f[7 * i + 6] != 0};
    const size_t nn = (size_t)n * (size_t)n;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const size_t at = (size_t)i * (size_t)n + (size_t)j;
            rel5[at] = blk_less_pos(v[i], v[j]); rel5[nn + at] = blk_greater_pos(v[i], v[j]); rel5[2 * nn + at] = blk_eq_pos(v[i], v[j]);
            rel5[3 * nn + at] = blk_same(v[i], v[j]); rel5[4 * nn + at] = blk_less_readpos(v[i], v[j]);
        }
    // the library sorts the blocks themselves (sq_segment.cpp: bamdiscordant; sq_chimeric.cpp: SortbyReadPos); the input
    // index rides along in a parallel array by sorting (block, index) pairs with the same comparator
    std::vector<std::pair<Blk, int32_t>> s((size_t)n);
    for (int i = 0; i < n; ++i) s[(size_t)i] = {v[(size_t)i], i};
    std::sort(s.begin(), s.end(), [](const std::pair<Blk, int32_t>& x, const std::pair<Blk, int32_t>& y) { return blk_less_pos(x.first, y.first); });
    for (int i = 0; i < n; ++i) perm_pos[i] = s[(size_t)i].second;
    for (int i = 0; i < n; ++i) s[(size_t)i] = {v[(size_t)i], i};
    std::sort(s.begin(), s.end(), [](const std::pair<Blk, int32_t>& x, const std::pair<Blk, int32_t>& y) { return blk_less_readpos(x.first, y.first); });
    for (int i = 0; i < n; ++i) perm_readpos[i] = s[(size_t)i].second;
    return SQ_OK;
}
int sq_set_shard(sq_ctx* c, int32_t first_ref, int32_t end_ref) {
    if (!c) return SQ_E_ARG;
    if (c->P.world_size <= 1) return fail(c, SQ_E_ARG, "sq_set_shard needs sq_params.world_size > 1");
    if (c->P.rank < 0 || c->P.rank >= c->P.world_size) return fail(c, SQ_E_ARG, "sq_params.rank out of range");
    if (c->ref_len.empty()) return fail(c, SQ_E_ARG, "sq_set_references first");
    if (first_ref < 0 || end_ref < first_ref || end_ref > (int32_t)c->ref_len.size()) return fail(c, SQ_E_ARG, "bad RefID range");
    if (c->counts.n_concordant) return fail(c, SQ_E_ARG, "sq_set_shard after concordant records were ingested");
    c->shard = Shard();
    c->shard.on = true; c->shard.first_ref = first_ref; c->shard.end_ref = end_ref;
    return SQ_OK;
}
int sq_exchange_pack(sq_ctx* c, const void** buf, int64_t* nbytes) {
    if (!c || !buf || !nbytes) return SQ_E_ARG;
    if (!c->x_pending) return fail(c, SQ_E_ARG, "no exchange is pending (sq_build_graph / sq_call_sv return SQ_NEED_EXCHANGE first)");
    *buf = c->xbuf.data(); *nbytes = (int64_t)c->xbuf.size();
    return SQ_OK;
}
static int sq_exchange_unpack_impl(sq_ctx* c, const void* gathered, const int64_t* nbytes_per_rank, int32_t world_size) {
    if (!c || !nbytes_per_rank || world_size != c->P.world_size) return SQ_E_ARG;
    if (!c->x_pending) return fail(c, SQ_E_ARG, "no exchange is pending");
    c->xgot.assign(world_size, {});
    const uint8_t* p = (const uint8_t*)gathered;
    for (int r = 0; r < world_size; ++r) {
        if (nbytes_per_rank[r] < 0 || (nbytes_per_rank[r] && !p)) return SQ_E_ARG;
        c->xgot[r].assign(p, p + nbytes_per_rank[r]);
        p += nbytes_per_rank[r];
    }
    if (c->xgot[c->P.rank] != c->xbuf) return fail(c, SQ_E_ARG, "sq_exchange_unpack: this rank's slot does not hold what sq_exchange_pack returned");
    c->x_pending = false; c->x_ready = true;
    return SQ_OK;
}
int sq_exchange_unpack(sq_ctx* c, const void* gathered, const int64_t* nbytes_per_rank, int32_t world_size) { return abi_guard(c, "sq_exchange_unpack", [&]() { return sq_exchange_unpack_impl(c, gathered, nbytes_per_rank, world_size); }); }

}  // extern "C"
