// GPU-free check of the pipelined sweep's deal (dynetlsm_amd/csrc/pipe_plan.hpp): which (active slice, part, node)
// a wavefront of an evaluator workgroup takes in launch l, at 16 or at 8 nodes per workgroup.  For every series
// length, network size, CU count and launch: every item of the launch is owned by exactly one (workgroup,
// wavefront) under the kernel's decode (pipe_eval_lds: pipe_deal, pipe_deal_part and the slice / node arithmetic
// restated below), the workgroups fit the launch's grid, the nodes of a workgroup share a window (one side of the
// batch's 64-node halves), and a launch whose resolvers have a batch to resolve keeps 16 nodes per workgroup.
// Test infrastructure (tests/test_pipe_deal_cpu.py builds and runs it, under ASan / UBSan).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../dynetlsm_amd/csrc/pipe_plan.hpp"

using namespace dlsm;

int main() {
    long launches = 0, spread = 0;
    const int Ns[] = {512, 520, 640, 2000, 2100};
    for (int T = 1; T <= 12; ++T)
        for (int N : Ns)
            for (int n_cu = 64; n_cu <= 304; n_cu += 8) {
                const int nbat = (N + PL_B - 1) / PL_B;
                const int ne_wg = pipe_eval_workgroups(n_cu, T);
                const int P = pipe_parts_undirected(ne_wg, T);
                if (P < 1 || P > 8) { printf("parts %d: T %d n_cu %d\n", P, T, n_cu); return 1; }
                // (the LDS evaluators run only when one round of workgroups covers the items: capi.hip)
                if ((long)P * T * PL_B > (long)ne_wg * PL_WAVES) continue;
                const int last = T > 1 ? nbat : nbat - 1;
                for (int l = -1; l <= last; ++l) {
                    const bool any_eval = (l + 1 < nbat) || (T > 1 && l >= 0 && l < nbat);
                    if (!any_eval) continue;
                    for (int on = 0; on < 2; ++on) {
                        const int qs = pipe_launch_qshift(T, nbat, P, ne_wg, l, on != 0);
                        if (qs != 3 && qs != 4) { printf("qshift %d\n", qs); return 1; }
                        if (!on && qs != 4) { printf("spread without its switch\n"); return 1; }
                        // resolvers with work: even slices resolve batch l, odd slices batch l - 1
                        bool resolves = false;
                        for (int t = 0; t < T; ++t) { const int b = l - (t & 1); resolves |= b >= 0 && b < nbat; }
                        if (resolves != pipe_launch_resolves(T, nbat, l)) { printf("resolves: T %d nbat %d l %d\n", T, nbat, l); return 1; }
                        if (resolves && qs != 4) { printf("spread beside a resolver: T %d N %d l %d\n", T, N, l); return 1; }
                        // the launch's fields as the host fills them
                        const int beE = l + 1, beO = l, nE = (T + 1) / 2, nO = T / 2;
                        const int nbE = (beE >= 0 && beE < nbat) ? std::min(PL_B, N - beE * PL_B) : 0;
                        const int nbO = (beO >= 0 && beO < nbat) ? std::min(PL_B, N - beO * PL_B) : 0;
                        const int nslE = nbE > 0 ? nE : 0, nslO = nbO > 0 ? nO : 0, nsl = nslE + nslO;
                        if (nsl != pipe_launch_slices(T, nbat, l)) { printf("slices: T %d nbat %d l %d\n", T, nbat, l); return 1; }
                        const uint32_t magic = pipe_deal_magic(nsl);
                        // owners[(t P + p) PL_B + k]
                        std::vector<int> owners((size_t)T * P * PL_B, 0);
                        for (int e = 0; e < ne_wg; ++e) {
                            const PipeDeal d = pipe_deal(e, qs);
                            const int p = pipe_deal_part(d.r, magic);
                            if (p != d.r / nsl) { printf("quotient: r %d nsl %d\n", d.r, nsl); return 1; }
                            const int si = d.r - p * nsl;
                            const bool odd = si >= nslE;
                            const int nb = p < P ? (odd ? nbO : nbE) : 0;
                            if (d.k0 >= nb) continue;                       // (workgroup without items)
                            const int t = odd ? 2 * (si - nslE) + 1 : 2 * si;
                            if (t < 0 || t >= T) { printf("slice %d: T %d\n", t, T); return 1; }
                            int klast = d.k0;
                            for (int wave = 0; wave < PL_WAVES; ++wave) {
                                const int k = d.k0 + wave;
                                if (!(k < nb && wave < d.nlive)) continue;
                                ++owners[((size_t)t * P + p) * PL_B + k];
                                klast = k;
                            }
                            if (d.k0 / 64 != klast / 64) { printf("a workgroup across the halves: k0 %d\n", d.k0); return 1; }
                        }
                        for (int t = 0; t < T; ++t) {
                            const int nb = (t & 1) ? nbO : nbE;
                            for (int p = 0; p < P; ++p)
                                for (int k = 0; k < PL_B; ++k) {
                                    const int want = k < nb ? 1 : 0;
                                    if (owners[((size_t)t * P + p) * PL_B + k] != want) {
                                        printf("owners: T %d N %d n_cu %d l %d q %d: item (t %d, p %d, k %d) owned %d times, not %d\n",
                                               T, N, n_cu, l, 1 << qs, t, p, k, owners[((size_t)t * P + p) * PL_B + k], want);
                                        return 1;
                                    }
                                }
                        }
                        ++launches;
                        if (qs == 3) ++spread;
                    }
                }
            }
    // the benchmark's head launch is one of the spread ones: T = 10, N = 2000 on 256 CUs
    {
        const int ne_wg = pipe_eval_workgroups(256, 10), P = pipe_parts_undirected(ne_wg, 10);
        if (pipe_launch_qshift(10, 16, P, ne_wg, -1, true) != 3) { printf("the benchmark's head is not spread\n"); return 1; }
        if (pipe_launch_qshift(10, 16, P, ne_wg, 0, true) != 4) { printf("launch 0 is spread\n"); return 1; }
    }
    if (spread == 0) { printf("no launch was spread\n"); return 1; }
    printf("check_pipe_deal ok: %ld launches, %ld of them at 8 nodes per workgroup\n", launches, spread);
    return 0;
}
