// GPU-free check of the packed workspaces' layouts (dynetlsm_amd/csrc/workspace.hpp): the allocations that hold
// several arrays of the sweeps, the HDP-LPCM loop and the case-control pass.  For every layout and shape: the sizing
// run (a Carve over a null base) gives the closed-form total the launchers used to spell out - restated here as the
// independent expectation; every region starts at or behind the end of the one before it and is aligned to its
// element type, and to 16 bytes where a kernel reads it as double2; the last region ends at the total; and the
// carving run over a host allocation of exactly that total stays inside it - the first and last element of every
// region are written under ASan.
// Test infrastructure (tests/test_workspace_cpu.py builds and runs it, under ASan / UBSan).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../dynetlsm_amd/csrc/workspace.hpp"

using namespace dlsm;

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// the kernels' constants, as the headers next to them state them
constexpr size_t SP_BMAX = 128, SP_SMAX = 4;                        // kernels_spec_sweep.hpp
constexpr size_t PP_B = 128, PP_ACC = PP_B + 8, PP_H_SLICE = 2 * PP_B * PP_B;   // kernels_spec_pipe.hpp
constexpr size_t CP_B = 512, CP_WAVES = 16;                         // kernels_ccpipe.hpp
constexpr size_t HS_COUNT = 16;                                     // kernels_hdploop.hpp
static size_t cp_record_width(size_t D) { return D + 1 <= 4 ? 4 : (D + 1 <= 8 ? 8 : 12); }
static size_t llcc_record_width(size_t D) { return D + 2 <= 4 ? 4 : (D + 2 <= 8 ? 8 : 12); }
static size_t even2(size_t n) { return (n + 1) / 2 * 2; }

// the regions' fields of the kernels' argument structs (SpecBuf, PipeBuf, CcPipeBuf, HdpLoopBuf)
struct SpecLayout { double *full0, *prop, *Ht, *consts; };
struct PipeLayout { double *prop, *full0, *H; int32_t *acc; double *consts, *xprod; };
struct CcPipeLayout {
    double *prop, *tot, *xval, *oval, *cur, *snap, *xsum;
    int32_t *xidx, *oidx, *cnt;
    unsigned long long *accmask;
};
struct HdpLoopLayout { double *beta, *mbar, *S, *Q, *L, *LP, *LPD, *scr; int32_t *m, *wover; };

struct Region { const char *name; char *p; size_t bytes, elem, align; };
template <typename T>
static Region region(const char *name, T *p, size_t n, size_t align = alignof(T)) {
    return Region{name, (char *)p, n * sizeof(T), sizeof(T), align};
}

// `sized`: the sizing run's total; `want`: the closed form; `regs`: the carving run's regions over `base`
static int check_regions(const char *what, size_t sized, size_t want, size_t carved, char *base,
                         const std::vector<Region> &regs) {
    CHECK(sized == want, "%s: the sizing run gives %zu bytes, the closed form %zu", what, sized, want);
    CHECK(carved == sized, "%s: the carving run ends at %zu, the sizing run at %zu", what, carved, sized);
    size_t end = 0;
    for (const Region &r : regs) {
        const size_t off = (size_t)(r.p - base);
        CHECK(off >= end, "%s: %s starts at %zu, inside the region before it (ends at %zu)", what, r.name, off, end);
        CHECK(off % r.elem == 0 && off % r.align == 0, "%s: %s at %zu is not aligned to %zu", what, r.name, off, r.align);
        end = off + r.bytes;
        CHECK(end <= sized, "%s: %s ends at %zu, beyond the total %zu", what, r.name, end, sized);
        if (r.bytes) {          // first and last element (ASan: inside the allocation)
            for (size_t b = 0; b < r.elem; ++b) { r.p[b] = 1; r.p[r.bytes - r.elem + b] = 2; }
        }
    }
    return 0;
}
// the layouts end on their last region, but for the HDP-LPCM loop's two spare doubles
static int check_end(const char *what, const Region &last, char *base, size_t sized, size_t spare = 0) {
    CHECK((size_t)(last.p - base) + last.bytes + spare == sized, "%s: %s does not end at the total", what, last.name);
    return 0;
}

static int check_spec(size_t T, size_t N, size_t D, size_t S, bool cc) {
    // (launch_sweep_spec's batch and parts)
    const size_t nsl = (T + 1) / 2, B = std::min(S * SP_BMAX, (N + 1) / 2 * 2);
    size_t parts = std::max<size_t>(1, std::min<size_t>((1024 + nsl * SP_BMAX - 1) / (nsl * SP_BMAX), 8));
    if (cc) parts = 1;
    const size_t want = (even2(nsl * B * parts) + even2(nsl * N * (D + 2)) + nsl * B * B + 2) * sizeof(double);
    SpecLayout l;
    Carve size; spec_layout(size, l, nsl, N, D, B, parts);
    char *base = (char *)malloc(size.bytes());
    Carve at(base); spec_layout(at, l, nsl, N, D, B, parts);
    const std::vector<Region> regs = {region("full0", l.full0, nsl * B * parts, 16), region("prop", l.prop, nsl * N * (D + 2), 16),
                                      region("Ht", l.Ht, nsl * B * B, 16), region("consts", l.consts, 2)};
    int bad = check_regions("spec", size.bytes(), want, at.bytes(), base, regs) || check_end("spec", regs.back(), base, size.bytes());
    free(base);
    CHECK(!bad, "  at T %zu N %zu D %zu S %zu cc %d", T, N, D, S, (int)cc);
    return 0;
}

static int check_pipe(size_t T, size_t N, size_t D, size_t parts) {
    const size_t n_h = 2 * T * PP_H_SLICE;                            // pipe_h_doubles(T)
    const size_t want = (even2(T * N * (2 * D + 2)) + 2 * T * PP_B * parts * 2 + n_h + even2((T * 2 * PP_ACC + 1) / 2) + 2 +
                         T * PP_B) * sizeof(double);
    PipeLayout l;
    Carve size; pipe_layout(size, l, T, N, D, PP_B, parts, n_h, PP_ACC);
    char *base = (char *)malloc(size.bytes());
    Carve at(base); pipe_layout(at, l, T, N, D, PP_B, parts, n_h, PP_ACC);
    const std::vector<Region> regs = {region("prop", l.prop, T * N * (2 * D + 2), 16), region("full0", l.full0, 2 * T * PP_B * parts * 2, 16),
                                      region("H", l.H, n_h, 16), region("acc", l.acc, T * 2 * PP_ACC, 8),
                                      region("consts", l.consts, 2, 16), region("xprod", l.xprod, T * PP_B, 16)};
    int bad = check_regions("pipe", size.bytes(), want, at.bytes(), base, regs) || check_end("pipe", regs.back(), base, size.bytes());
    free(base);
    CHECK(!bad, "  at T %zu N %zu D %zu parts %zu", T, N, D, parts);
    return 0;
}

static int check_ccpipe(size_t T, size_t N, size_t D, size_t terms) {
    const size_t cap = std::max<size_t>(1, terms);                    // (launch_sweep_ccpipe: Din + Dout + 2 C)
    const size_t n_prop = even2(T * N * (2 * D + 2)), n_tot = 2 * T * CP_B, n_ent = 2 * T * cap * CP_B, n_cnt = 2 * T * CP_B * 2;
    const size_t n_rec = T * N * cp_record_width(D), n_xsum = T * CP_B;
    const size_t want = (n_prop + n_tot + 2 * n_ent + 2 + 2 * n_rec + n_xsum) * sizeof(double) +
                        even2(2 * n_ent + n_cnt) * sizeof(int32_t) + T * CP_WAVES * sizeof(unsigned long long);
    CcPipeLayout l;
    Carve size; ccpipe_layout(size, l, T, N, D, CP_B, cap, cp_record_width(D), CP_WAVES);
    char *base = (char *)malloc(size.bytes());
    Carve at(base);
    double *consts = ccpipe_layout(at, l, T, N, D, CP_B, cap, cp_record_width(D), CP_WAVES);
    const std::vector<Region> regs = {
        region("prop", l.prop, T * N * (2 * D + 2), 16), region("tot", l.tot, n_tot, 16), region("xval", l.xval, n_ent),
        region("oval", l.oval, n_ent), region("consts", consts, 2), region("cur", l.cur, n_rec, 16),
        region("snap", l.snap, n_rec, 16), region("xsum", l.xsum, n_xsum), region("xidx", l.xidx, n_ent),
        region("oidx", l.oidx, n_ent), region("cnt", l.cnt, n_cnt), region("accmask", l.accmask, T * CP_WAVES)};
    int bad = check_regions("ccpipe", size.bytes(), want, at.bytes(), base, regs) ||
              check_end("ccpipe", regs.back(), base, size.bytes());
    free(base);
    CHECK(!bad, "  at T %zu N %zu D %zu terms %zu", T, N, D, terms);
    return 0;
}

static int check_hdp_loop(size_t T, size_t K, size_t D) {
    const size_t want = (2 * K + T * K * D + 5 * T * K + HS_COUNT + (T * K * K + T * K + 1) / 2 + 2) * sizeof(double);
    HdpLoopLayout l;
    Carve size; hdp_loop_layout(size, l, T, K, D, HS_COUNT);
    char *base = (char *)malloc(size.bytes());
    Carve at(base); hdp_loop_layout(at, l, T, K, D, HS_COUNT);
    const std::vector<Region> regs = {
        region("beta", l.beta, K), region("mbar", l.mbar, K), region("S", l.S, T * K * D), region("Q", l.Q, T * K),
        region("L", l.L, 2 * T * K), region("LP", l.LP, T * K), region("LPD", l.LPD, T * K), region("scr", l.scr, HS_COUNT),
        region("m", l.m, T * K * K), region("wover", l.wover, T * K)};
    // (behind the counts: their padding to a whole double and the two spare doubles)
    const size_t counts = (T * K * K + T * K) * sizeof(int32_t), pad = (8 - counts % 8) % 8;
    int bad = check_regions("hdp_loop", size.bytes(), want, at.bytes(), base, regs) ||
              check_end("hdp_loop", regs.back(), base, size.bytes(), pad + 2 * sizeof(double));
    free(base);
    CHECK(!bad, "  at T %zu K %zu D %zu", T, K, D);
    return 0;
}

static int check_xr(size_t T, size_t N, size_t D) {
    const size_t want = T * N * llcc_record_width(D) * sizeof(double);
    Carve size;
    xr_layout(size, T, N, llcc_record_width(D));
    char *base = (char *)malloc(size.bytes());
    Carve at(base);
    double *xr = xr_layout(at, T, N, llcc_record_width(D));
    const std::vector<Region> regs = {region("xr", xr, T * N * llcc_record_width(D), 16)};
    int bad = check_regions("xr", size.bytes(), want, at.bytes(), base, regs) || check_end("xr", regs.back(), base, size.bytes());
    free(base);
    CHECK(!bad, "  at T %zu N %zu D %zu", T, N, D);
    return 0;
}

int main() {
    const size_t Ts[] = {1, 2, 3}, Ns[] = {2, 3, 127, 128, 129, 513}, Ds[] = {1, 3, 8}, Ks[] = {1, 5}, terms[] = {0, 1, 7};
    long n = 0;
    for (size_t T : Ts)
        for (size_t D : Ds) {
            for (size_t N : Ns) {
                for (size_t S : {(size_t)1, (size_t)2, SP_SMAX}) {
                    if (check_spec(T, N, D, S, false)) return 1;
                    ++n;
                }
                if (check_spec(T, N, D, 1, true)) return 1;
                for (size_t parts : {1, 3, 4, 8}) {
                    if (check_pipe(T, N, D, parts)) return 1;
                    ++n;
                }
                for (size_t t : terms) {
                    if (check_ccpipe(T, N, D, t)) return 1;
                    ++n;
                }
                if (check_xr(T, N, D)) return 1;
                n += 2;
            }
            for (size_t K : Ks) {
                if (check_hdp_loop(T, K, D)) return 1;
                ++n;
            }
        }
    printf("check_workspace ok (%ld layouts)\n", n);
    return 0;
}
