// The host's plan of a pass over resident posterior samples (capi_samples.hpp): the tiles of a time step, the grid
// that walks them and the list of the pass's device buffers with its byte accounting.  Plain C++: capi_samples.hpp
// adds the HIP calls, tests/native/check_pass_plan.cpp compiles this header with g++.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <vector>

namespace dlsm {

constexpr int PASS_TJ = 64;                 // = IC_TJ (kernels_dyad_pass.hpp): columns of a tile
constexpr int PASS_G_MAX = 1 << 16;         // workgroups of one time step, unless a pass has a cap of its own

struct PassTile { int bi, bj; };            // (row block, column block): the device reads it as an int2

// tiles of one time step, row block by row block: (row block of TI rows, column block of PASS_TJ columns);
// undirected: those that hold a dyad i < j
inline std::vector<PassTile> ic_tiles(int N, int TI, bool directed) {
    std::vector<PassTile> tiles;
    const int nbi = (N + TI - 1) / TI, nbj = (N + PASS_TJ - 1) / PASS_TJ;
    for (int bi = 0; bi < nbi; ++bi)
        for (int bj = 0; bj < nbj; ++bj)
            if (directed || bi * TI < std::min(N, (bj + 1) * PASS_TJ) - 1) tiles.push_back(PassTile{bi, bj});
    return tiles;
}

// L tiles per workgroup, as few as keep the G workgroups of a time step within g_cap (no tiles: L = G = 0)
struct PassGrid { int L, G; };
inline PassGrid pass_grid(int n_tiles, size_t g_cap) {
    const int L = (int)(((size_t)n_tiles + g_cap - 1) / g_cap);
    return PassGrid{L, L ? (n_tiles + L - 1) / L : 0};
}

enum : unsigned { PASS_ZERO = 1, PASS_OPTIONAL = 2, PASS_PER_SAMPLE = 4 };

// One device buffer of a pass: `bytes` in all or, with PASS_PER_SAMPLE, for each sample.  It starts from the host
// array `fill` if there is one, zeroed with PASS_ZERO, else untouched; an output is copied back to `dest`.
struct PassBuf {
    size_t bytes;
    unsigned flags;
    const void *fill;
    void *dest;
    void *dev;              // the allocation (the driver's)
    size_t total(size_t S) const { return flags & PASS_PER_SAMPLE ? S * bytes : bytes; }
};

// The buffers of a pass, each declared once; an id is the position in the list, -1 an absent buffer.
struct PassBufs {
    std::vector<PassBuf> list;

    int add(size_t elem, size_t n, unsigned flags = 0, const void *fill = nullptr, void *dest = nullptr) {
        list.push_back(PassBuf{elem * n, flags, fill, dest, nullptr});
        return (int)list.size() - 1;
    }
    // an output; one with PASS_OPTIONAL and no dest is absent
    int output(size_t elem, size_t n, void *dest, unsigned flags = 0, const void *fill = nullptr) {
        return !dest && (flags & PASS_OPTIONAL) ? -1 : add(elem, n, flags, fill, dest);
    }
    void *dev(int id) const { return id < 0 ? nullptr : list[(size_t)id].dev; }
    // what the list allocates: `fixed` + S `per_sample` bytes
    void bytes(size_t &fixed, size_t &per_sample) const {
        fixed = per_sample = 0;
        for (const PassBuf &b : list) (b.flags & PASS_PER_SAMPLE ? per_sample : fixed) += b.bytes;
    }
    std::vector<const PassBuf *> outputs() const {      // in the order of their declaration
        std::vector<const PassBuf *> out;
        for (const PassBuf &b : list) if (b.dest) out.push_back(&b);
        return out;
    }
};

}  // namespace dlsm
