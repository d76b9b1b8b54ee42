// Host check of csrc/psis_tail.hpp (tests/test_loo_cpu.py): reads sorted tails, prints the fit and the smoothed tail.
//
//     check_psis_tail FILE
//
// FILE: the number of tails, then per tail M and the M + 1 smallest log-likelihoods in ascending order (anything
// strtod reads: hexadecimal floats keep every bit).  Per tail one line: fitted (0 / 1), k, sigma, lw_(1) .. lw_(M)
// as hexadecimal floats (an unfitted tail: the raw lr_(m) = l(0) - l(M - m)).  `check_psis_tail --tail-length S`
// prints psis_tail_length(S).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "psis_tail.hpp"

struct VectorTail {
    const std::vector<double> &v;
    double operator()(int i) const { return v.at((size_t)i); }       // at(): an index beyond the tail throws
};

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "--tail-length") {
        printf("%d\n", dlsm::psis_tail_length(atoll(argv[2])));
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: %s FILE | --tail-length S\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int n = 0;
    if (fscanf(f, "%d", &n) != 1 || n < 0) { fprintf(stderr, "bad count\n"); return 2; }
    char word[128];
    for (int q = 0; q < n; ++q) {
        int M = 0;
        if (fscanf(f, "%d", &M) != 1 || M < 0) { fprintf(stderr, "bad M of tail %d\n", q); return 2; }
        std::vector<double> v((size_t)M + 1);
        for (int i = 0; i <= M; ++i) {
            if (fscanf(f, "%127s", word) != 1) { fprintf(stderr, "tail %d is short\n", q); return 2; }
            v[(size_t)i] = strtod(word, nullptr);
        }
        const VectorTail tail = {v};
        const dlsm::PsisFit fit = dlsm::psis_fit(tail, M);
        printf("%d %a %a", fit.fitted ? 1 : 0, fit.k, fit.sigma);
        for (int m = 1; m <= M; ++m)
            printf(" %a", fit.fitted ? dlsm::psis_smoothed(fit, m, M) : tail(0) - tail(M - m));
        printf("\n");
    }
    fclose(f);
    return 0;
}
