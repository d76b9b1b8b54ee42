// GPU-free check of the host's plan of a pass over resident posterior samples (dynetlsm_amd/csrc/pass_plan.hpp):
// the tiles of a time step, the grid that walks them and the byte accounting of a pass's buffer list.
// Tiles, for every N, tile height and model: every dyad (i < j, directed: i != j) lies in exactly one listed tile,
// an undirected list holds no tile without a dyad, a directed list holds every tile, and the list is in
// row-block-major order.  Grid, for n_tiles around multiples of the cap: G L >= n_tiles, (G - 1) L < n_tiles,
// G <= cap, L no larger than the cap asks for, no tiles give G = 0, and the values are those of the formulas the
// drivers used to spell out.  Buffers: the budget is the sum of the declared bytes, fixed and per-sample apart; an
// absent optional output adds nothing and has a NULL pointer; the outputs come back in the order of declaration.
// Test infrastructure (tests/test_pass_plan_cpu.py builds and runs it, under ASan / UBSan).
#include <cstdio>
#include <map>
#include <utility>
#include <vector>
#include "../../dynetlsm_amd/csrc/pass_plan.hpp"

using namespace dlsm;

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int check_tiles(int N, int TI, bool directed) {
    const std::vector<PassTile> tiles = ic_tiles(N, TI, directed);
    const int nbi = (N + TI - 1) / TI, nbj = (N + PASS_TJ - 1) / PASS_TJ;
    std::map<std::pair<int, int>, long> dyads;          // listed tile -> dyads found in it
    for (size_t k = 0; k < tiles.size(); ++k) {
        const PassTile t = tiles[k];
        CHECK(t.bi >= 0 && t.bi < nbi && t.bj >= 0 && t.bj < nbj, "N %d TI %d: tile (%d, %d) outside", N, TI, t.bi, t.bj);
        if (k) {
            const PassTile p = tiles[k - 1];
            CHECK(p.bi < t.bi || (p.bi == t.bi && p.bj < t.bj), "N %d TI %d dir %d: tile %zu out of order", N, TI,
                  (int)directed, k);
        }
        dyads[std::make_pair(t.bi, t.bj)] = 0;
    }
    CHECK(dyads.size() == tiles.size(), "N %d TI %d: a tile is listed twice", N, TI);     // (implied by the order)
    for (int i = 0; i < N; ++i)
        for (int j = directed ? 0 : i + 1; j < N; ++j) {
            if (i == j) continue;
            const auto it = dyads.find(std::make_pair(i / TI, j / PASS_TJ));
            CHECK(it != dyads.end(), "N %d TI %d dir %d: dyad (%d, %d) in no listed tile", N, TI, (int)directed, i, j);
            ++it->second;
        }
    if (directed) CHECK((long)tiles.size() == (long)nbi * nbj, "N %d TI %d: a directed tile is missing", N, TI);
    else
        for (const auto &kv : dyads)
            CHECK(kv.second > 0, "N %d TI %d: tile (%d, %d) holds no dyad", N, TI, kv.first.first, kv.first.second);
    return 0;
}

static int check_grid(long long n_tiles, size_t cap) {
    if (n_tiles < 0 || n_tiles > 0x7FFFFFFF) return 0;
    const int n = (int)n_tiles;
    const PassGrid g = pass_grid(n, cap);
    if (!n) { CHECK(g.G == 0 && g.L == 0, "cap %zu: no tiles give L %d G %d", cap, g.L, g.G); return 0; }
    CHECK(g.L >= 1 && g.G >= 1, "n %d cap %zu: L %d G %d", n, cap, g.L, g.G);
    CHECK((long long)g.G * g.L >= n, "n %d cap %zu: G L < n", n, cap);
    CHECK((long long)(g.G - 1) * g.L < n, "n %d cap %zu: a workgroup without a tile", n, cap);
    CHECK((size_t)g.G <= cap, "n %d cap %zu: G %d over the cap", n, cap, g.G);
    CHECK((unsigned long long)(g.L - 1) * cap < (unsigned long long)n, "n %d cap %zu: L %d larger than needed", n, cap, g.L);
    // as the drivers spelled it: in int for a cap that is an int, in size_t for the cap of the information criteria
    const int L_sz = (int)(((size_t)n + cap - 1) / cap);
    CHECK(g.L == L_sz && g.G == (n + L_sz - 1) / L_sz, "n %d cap %zu: not the size_t formula", n, cap);
    if (cap <= (1u << 16)) {
        const int c = (int)cap, L = (n + c - 1) / c, G = L ? (n + L - 1) / L : 0;
        CHECK(g.L == L && g.G == G, "n %d cap %zu: not the int formula", n, cap);
    }
    return 0;
}

static int check_buffers(bool want_pointwise) {
    const size_t S = 7, T = 3, N = 70;
    double edges[16] = {0}, totals[1], sample[1], pw[1];
    unsigned long long hist[1];
    PassBufs p;
    const int iE = p.add(sizeof(double), 16, 0, edges);
    const int iPart = p.add(sizeof(double), T * 5);
    const int iPS = p.add(sizeof(double), T * 4, PASS_PER_SAMPLE);
    const int iTot = p.output(sizeof(double), T * 5, totals);
    const int iH = p.output(sizeof(unsigned long long), T * 9, hist, PASS_ZERO);
    const int iPW = p.output(sizeof(double), T * N * N * 2, want_pointwise ? pw : nullptr, PASS_ZERO | PASS_OPTIONAL);
    const int iSL = p.output(sizeof(double), T, sample, PASS_PER_SAMPLE);
    CHECK(iE == 0 && iPart == 1 && iPS == 2 && iTot == 3 && iH == 4, "ids are not the positions in the list");
    CHECK(iPW == (want_pointwise ? 5 : -1) && iSL == (want_pointwise ? 6 : 5), "the optional output's id");
    CHECK(p.list.size() == (want_pointwise ? 7u : 6u), "an absent output was listed");
    size_t fixed = 1, per_sample = 1;
    p.bytes(fixed, per_sample);
    const size_t pw_bytes = want_pointwise ? T * N * N * 2 * sizeof(double) : 0;
    CHECK(fixed == (16 + T * 5 + T * 5) * sizeof(double) + T * 9 * 8 + pw_bytes, "fixed bytes %zu", fixed);
    CHECK(per_sample == (T * 4 + T) * sizeof(double), "per-sample bytes %zu", per_sample);
    size_t sum = 0;                                     // the budget is what the driver allocates
    for (const PassBuf &b : p.list) sum += b.total(S);
    CHECK(sum == fixed + S * per_sample, "the buffers' totals %zu are not the budget", sum);
    CHECK(p.list[(size_t)iPS].total(S) == S * T * 4 * sizeof(double) && p.list[(size_t)iE].total(S) == sizeof(edges),
          "total()");
    CHECK(p.list[(size_t)iE].fill == edges && !p.list[(size_t)iE].dest && !(p.list[(size_t)iE].flags & PASS_ZERO), "fill");
    int dummy[7];
    for (size_t k = 0; k < p.list.size(); ++k) {
        CHECK(p.list[k].dev == nullptr, "a buffer is born allocated");
        p.list[k].dev = &dummy[k];
    }
    CHECK(p.dev(-1) == nullptr && p.dev(iTot) == &dummy[3] && p.dev(iSL) == &dummy[want_pointwise ? 6 : 5], "dev()");
    if (!want_pointwise) CHECK(p.dev(iPW) == nullptr, "an absent output has a pointer");
    const std::vector<const PassBuf *> out = p.outputs();
    std::vector<const void *> dests = {totals, hist};
    if (want_pointwise) dests.push_back(pw);
    dests.push_back(sample);
    CHECK(out.size() == dests.size(), "%zu outputs, %zu declared", out.size(), dests.size());
    for (size_t k = 0; k < out.size(); ++k) CHECK(out[k]->dest == dests[k], "output %zu out of order", k);
    return 0;
}

int main() {
    const int Ns[] = {2, 3, 31, 32, 33, 63, 64, 65, 96, 129, 200}, TIs[] = {1, 2, 4, 16, 32};
    for (int N : Ns)
        for (int TI : TIs)
            for (int directed = 0; directed < 2; ++directed)
                if (check_tiles(N, TI, directed != 0)) return 1;
    // the caps of the passes: PASS_G_MAX, small ones, and one the size of the information criteria's (bytes / (T S 8))
    const size_t caps[] = {1, 2, 7, (size_t)PASS_G_MAX, ((size_t)256 << 20) / (3 * 8 * sizeof(double))};
    for (size_t cap : caps) {
        const long long c = (long long)cap, ns[] = {0, 1, c - 1, c, c + 1, 3 * c + 2};
        for (long long n : ns)
            if (check_grid(n, cap)) return 1;
    }
    if (check_buffers(false) || check_buffers(true)) return 1;
    printf("check_pass_plan ok\n");
    return 0;
}
