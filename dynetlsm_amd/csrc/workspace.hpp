// The packed workspaces of the sweeps, the HDP-LPCM loop and the case-control pass: each is ONE device allocation
// holding several arrays, and each layout is stated once, as a function that takes its regions from a Carve in order
// and files them in the kernels' argument struct.  Run over a null base it sizes the allocation (Carve::bytes), run
// over the allocation it yields the pointers - the two cannot disagree.  Plain C++ (the struct is a template
// parameter, the kernels' constants are arguments), shared with tests/test_workspace_cpu.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dlsm {

// a cursor over one allocation
class Carve {
    char *base_;
    size_t off_ = 0;

public:
    explicit Carve(void *base = nullptr) : base_((char *)base) {}
    // the next region: n elements of T, its start rounded up to `align` bytes from the base (16 where a kernel
    // reads the region as double2 - the allocation itself is aligned far beyond that)
    template <typename T>
    T *take(size_t n, size_t align = alignof(T)) {
        off_ = (off_ + align - 1) / align * align;
        T *p = base_ ? (T *)(base_ + off_) : nullptr;
        off_ += n * sizeof(T);
        return p;
    }
    size_t bytes() const { return off_; }
};

// algo 2 / 3 (SpecBuf): nsl slices of a parity, batches of B nodes in `parts` parts
template <typename Buf>
void spec_layout(Carve &c, Buf &s, size_t nsl, size_t N, size_t D, size_t B, size_t parts) {
    s.full0 = c.take<double>(nsl * B * parts, 16);
    s.prop = c.take<double>(nsl * N * (D + 2), 16);
    s.Ht = c.take<double>(nsl * B * B, 16);
    s.consts = c.take<double>(2);
}

// algo 4 (PipeBuf): batches of B nodes, two batch slots of everything produced per batch; h_doubles =
// pipe_h_doubles(T), acc_words = PP_ACC
template <typename Buf>
void pipe_layout(Carve &c, Buf &p, size_t T, size_t N, size_t D, size_t B, size_t parts, size_t h_doubles,
                 size_t acc_words) {
    p.prop = c.take<double>(T * N * (2 * D + 2), 16);
    p.full0 = c.take<double>(2 * T * B * parts * 2, 16);
    p.H = c.take<double>(h_doubles);
    p.acc = c.take<int32_t>(T * 2 * acc_words);
    p.consts = c.take<double>(2, 16);
    p.xprod = c.take<double>(T * B);
}

// algo 5 (CcPipeBuf): batches of B nodes, correction lists of `cap` entries per node, records of rec_width doubles,
// an accept mask per wavefront of a resolver's `waves`; returns the proposal pass's two constants
template <typename Buf>
double *ccpipe_layout(Carve &c, Buf &p, size_t T, size_t N, size_t D, size_t B, size_t cap, size_t rec_width,
                      size_t waves) {
    const size_t n_ent = 2 * T * cap * B, n_rec = T * N * rec_width;
    p.prop = c.take<double>(T * N * (2 * D + 2), 16);
    p.tot = c.take<double>(2 * T * B, 16);
    p.xval = c.take<double>(n_ent); p.oval = c.take<double>(n_ent);
    double *consts = c.take<double>(2);
    p.cur = c.take<double>(n_rec); p.snap = c.take<double>(n_rec);
    p.xsum = c.take<double>(T * B);
    p.xidx = c.take<int32_t>(n_ent); p.oidx = c.take<int32_t>(n_ent);
    p.cnt = c.take<int32_t>(2 * T * B * 2);
    p.accmask = c.take<unsigned long long>(T * waves);
    return consts;
}

// the HDP-LPCM loop's auxiliary buffers (HdpLoopBuf); scr_doubles = HS_COUNT
template <typename Buf>
void hdp_loop_layout(Carve &c, Buf &b, size_t T, size_t K, size_t D, size_t scr_doubles) {
    b.beta = c.take<double>(K); b.mbar = c.take<double>(K);
    b.S = c.take<double>(T * K * D);
    b.Q = c.take<double>(T * K);
    b.L = c.take<double>(2 * T * K);
    b.LP = c.take<double>(T * K); b.LPD = c.take<double>(T * K);
    b.scr = c.take<double>(scr_doubles);
    b.m = c.take<int32_t>(T * K * K); b.wover = c.take<int32_t>(T * K);
    c.take<double>(2);          // (two spare doubles behind the counts, as the buffer has always had)
}

// the case-control pass's gather records (k_pack_xr): rec_width = llcc_record_width(D)
inline double *xr_layout(Carve &c, size_t T, size_t N, size_t rec_width) { return c.take<double>(T * N * rec_width); }

}  // namespace dlsm
