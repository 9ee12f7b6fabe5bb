// The cut kernels of sq_compress_windows_on_device (squid_amd/csrc/sq_compress_stage.inc: where a wave of FurtherCompressNode's walk may
// start from the state of a chromosome start) on the CPU: the kernel source itself (sq_wave.h with SQ_WAVE_EMU: every tile's wave runs as 64
// coroutines), host only, nothing linked.
//   fc_windows_emu [-dp <Concord_Dist_Pos>] [-di <Concord_Dist_Idx>] < graphs > tables
// stdin: one graph after the other, each as it enters FurtherCompressNode, in the format of tests/graphs.oracle_text ("n m", n node rows
// "chr pos len support depth", m edge rows "ind1 head1 ind2 head2 weight groupweight").  stdout: one line per graph, the window table: the
// first node of every window, then n.
// The per-node summary comes from k_fc_summary in production; here it is made from the edges by its definition (IsDiscordant,
// SegmentGraph.cpp:159-168).  The two sums the library takes with its device scan are plain loops here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../squid_amd/csrc/sq_compress_stage.inc"

namespace {
struct TileArg { const fcw::In* G; int64_t tile, ntiles; int32_t *state, *front, *flag; };
void w_state(void* p) { const TileArg& a = *(const TileArg*)p; fcw::tile_state(*a.G, a.tile, a.state); }
void w_prefix(void* p) { const TileArg& a = *(const TileArg*)p; fcw::tile_prefix(a.ntiles, a.state, a.front); }
void w_flags(void* p) { const TileArg& a = *(const TileArg*)p; fcw::tile_flags(*a.G, a.tile, a.front, a.flag); }

// dev_further_compress's cut stage, wave by wave
std::vector<int32_t> window_table(const std::vector<int32_t>& chr, const std::vector<int32_t>& hasdisc, const std::vector<int32_t>& maxfar) {
    const int32_t n = (int32_t)chr.size();
    const int64_t ntiles = ((int64_t)n + fcw::TILE - 1) / fcw::TILE;
    const fcw::In G{n, chr.data(), hasdisc.data(), maxfar.data()};
    std::vector<int32_t> state(2 * (size_t)ntiles, INT32_MIN), front(2 * (size_t)ntiles, INT32_MIN), flag((size_t)n, -7), winc((size_t)n);
    TileArg a{&G, 0, ntiles, state.data(), front.data(), flag.data()};
    for (a.tile = ntiles - 1; a.tile >= 0; --a.tile) wv::run_wave(w_state, &a);  // (the tiles from the last to the first: no tile may lean on another)
    wv::run_wave(w_prefix, &a);
    for (a.tile = ntiles - 1; a.tile >= 0; --a.tile) wv::run_wave(w_flags, &a);
    int32_t run = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (flag[i] != 0 && flag[i] != 1) { std::fprintf(stderr, "fc_windows_emu: node %d has no flag\n", i); std::exit(1); }
        winc[i] = run += flag[i];
    }
    std::vector<int32_t> win((size_t)run + 1, -1);
    for (int64_t i = n - 1; i >= 0; --i) fcw::scatter(n, flag.data(), winc.data(), win.data(), i);
    return win;
}
}  // namespace

int main(int argc, char** argv) {
    long dp = 50000, di = 20;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "-dp")) dp = std::atol(argv[i + 1]);
        else if (!std::strcmp(argv[i], "-di")) di = std::atol(argv[i + 1]);
        else { std::fprintf(stderr, "usage: fc_windows_emu [-dp <pos>] [-di <idx>] < graphs\n"); return 2; }
    }
    long n, m;
    while (std::scanf("%ld %ld", &n, &m) == 2) {
        if (n <= 0 || m < 0) { std::fprintf(stderr, "fc_windows_emu: bad graph header\n"); return 2; }
        std::vector<int32_t> chr((size_t)n), pos((size_t)n), len((size_t)n), hasdisc((size_t)n, 0), maxfar((size_t)n, -1);
        for (long i = 0; i < n; ++i) {
            long c, p, l, s;
            char depth[64];
            if (std::scanf("%ld %ld %ld %ld %63s", &c, &p, &l, &s, depth) != 5) { std::fprintf(stderr, "fc_windows_emu: bad node row %ld\n", i); return 2; }
            chr[(size_t)i] = (int32_t)c; pos[(size_t)i] = (int32_t)p; len[(size_t)i] = (int32_t)l;
        }
        for (long k = 0; k < m; ++k) {
            long a, ha, b, hb, w, gw;
            if (std::scanf("%ld %ld %ld %ld %ld %ld", &a, &ha, &b, &hb, &w, &gw) != 6 || a < 0 || b < a || b >= n) { std::fprintf(stderr, "fc_windows_emu: bad edge row %ld\n", k); return 2; }
            const bool disc = chr[(size_t)a] != chr[(size_t)b] || ((long)pos[(size_t)b] - pos[(size_t)a] - len[(size_t)a] > dp && b - a > di) || ha != 0 || hb != 1;
            if (disc) hasdisc[(size_t)a] = hasdisc[(size_t)b] = 1;
            else { if (b > maxfar[(size_t)a]) maxfar[(size_t)a] = (int32_t)b; if (b > maxfar[(size_t)b]) maxfar[(size_t)b] = (int32_t)b; }
        }
        const std::vector<int32_t> win = window_table(chr, hasdisc, maxfar);
        for (size_t k = 0; k < win.size(); ++k) std::printf(k ? " %d" : "%d", win[k]);
        std::printf("\n");
    }
    return 0;
}
