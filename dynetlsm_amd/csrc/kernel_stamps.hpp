// In-kernel phase stamps: the one place that knows whether they exist.
//
// A build with -DDLSM_PIPE_TIMING records the 100 MHz constant clock at phase boundaries of the hot kernels into the
// device arrays below; capi.hip's dlsm_debug_read_stamps copies an array out by name and profiles/stamps.py is its
// reader (-DDLSM_PIPE_TIMING=2 also turns on pipe_eval_lds's prologue probe).  In a product build every type here is
// empty and every function does nothing, so the kernels take and pass their stamp records unconditionally.
//
// To add a stamp: pick a free slot of the kernel's record and write DLSM_STAMP(st, slot, value) behind the instruction
// to be timed, `value` being something that instruction produced (the clock is read once `value` is there).  To stamp
// another kernel: declare its array here, name it in StampArray and stamp_array(), and add it to capi.hip's table.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace dlsm {

// the destinations of a stamp record, one per device array
enum StampArray { PIPE_ITEM_T, PIPE_RES_T, CC_RES_T, CC_ITEM_T, LAB_T, LL_T };

#ifdef DLSM_PIPE_TIMING
constexpr bool STAMP_PROLOGUE_PROBE = DLSM_PIPE_TIMING == 2;

// [launch of the sweep][row][slot]; the slots' meanings are with the kernels and in the profiles/ readers
constexpr int PIPE_T_LAUNCHES = 24, PIPE_ITEM_T_ROWS = 4096, PIPE_RES_T_ROWS = 32;
constexpr int CC_T_LAUNCHES = 32, CC_RES_T_ROWS = 16, CC_ITEM_T_ROWS = 4096;
constexpr int LAB_T_ROWS = 4096, LL_T_ROWS = 8192;
constexpr int HDP_T_KERNELS = 6, HDP_T_ROWS = 512, HDP_PHASES = 16;
__device__ unsigned long long g_pipe_item_t[PIPE_T_LAUNCHES][PIPE_ITEM_T_ROWS][6];  // per evaluator wavefront
__device__ unsigned long long g_pipe_res_t[PIPE_T_LAUNCHES][PIPE_RES_T_ROWS][5];    // per resolver workgroup (slice)
__device__ unsigned long long g_cc_res_t[CC_T_LAUNCHES][CC_RES_T_ROWS][8];          // resolver and helper of a slice
__device__ unsigned long long g_cc_item_t[CC_T_LAUNCHES][CC_ITEM_T_ROWS][2];        // per evaluator wavefront: entry, exit
__device__ unsigned long long g_lab_t[LAB_T_ROWS][6];                               // per wavefront of the label kernels
__device__ unsigned long long g_ll_t[LL_T_ROWS][3];                                 // per wavefront: entry, exit, HW_ID | XCC_ID << 32
__device__ unsigned long long g_hdp_t[HDP_T_KERNELS][HDP_T_ROWS][2];                // per workgroup: entry, exit
__device__ unsigned long long g_hdp_phase[HDP_PHASES][2];                           // phases of the globals' workgroup

// The clock, read once `dep` (a vector register) holds its value: the operand pins the read behind what it times.
template <class T>
__device__ __forceinline__ unsigned long long device_clock(T dep) {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep));
    return t;
}
// where the wavefront runs: HW_ID | XCC_ID << 32
__device__ __forceinline__ unsigned long long device_place() {
    unsigned int hwid, xccid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hwid), "=s"(xccid));
    return (unsigned long long)hwid | ((unsigned long long)xccid << 32);
}

template <StampArray A>
__device__ __forceinline__ auto &stamp_array() {
    if constexpr (A == PIPE_ITEM_T) return g_pipe_item_t;
    else if constexpr (A == PIPE_RES_T) return g_pipe_res_t;
    else if constexpr (A == CC_RES_T) return g_cc_res_t;
    else if constexpr (A == CC_ITEM_T) return g_cc_item_t;
    else if constexpr (A == LAB_T) return g_lab_t;
    else return g_ll_t;
}
// the row of an array, null outside its extents
template <int L, int R, int S>
__device__ __forceinline__ unsigned long long *stamp_row(unsigned long long (&a)[L][R][S], int launch, int row) {
    return launch >= 0 && launch < L && row >= 0 && row < R ? a[launch][row] : nullptr;
}
template <int R, int S>
__device__ __forceinline__ unsigned long long *stamp_row(unsigned long long (&a)[R][S], int, int row) {
    return row >= 0 && row < R ? a[row] : nullptr;
}

// The stamps of one row of array A, in registers until flush() stores them.
template <StampArray A>
struct Stamps {
    using Array = std::remove_reference_t<decltype(stamp_array<A>())>;
    static constexpr int N = std::extent<Array, std::rank<Array>::value - 1>::value;
    unsigned long long t[N] = {};
    int launch, row;            // (launch: unused by the arrays without that axis)
    bool armed_ = false;
    __device__ Stamps(int launch_ = -1, int row_ = -1) : launch(launch_), row(row_) {}     // (default: no destination)
    template <class T>
    __device__ __forceinline__ void mark(int i, T dep) { t[i] = device_clock(dep); }
    __device__ void mark_place(int i) { t[i] = device_place(); }
    __device__ unsigned long long get(int i) const { return t[i]; }
    __device__ void set(int i, unsigned long long v) { t[i] = v; }
    // a stamp inside a function that runs many times: `if (st.armed()) DLSM_STAMP(..)` takes the armed call's only
    __device__ void arm(bool on) { armed_ = on; }
    __device__ bool armed() const { return armed_; }
    // the slots named by the mask to the array's row (the caller picks the thread)
    __device__ __forceinline__ void flush(unsigned slots = ~0u) const {
        unsigned long long *dst = stamp_row(stamp_array<A>(), launch, row);
        if (dst) {
#pragma unroll
            for (int i = 0; i < N; ++i) if ((slots >> i) & 1u) dst[i] = t[i];
        }
    }
};
#define DLSM_STAMP(ST_, I_, DEP_) (ST_).mark(I_, DEP_);

// The workgroup-level forms of the HDP tail (profiles/hdp_tail_timing.py).  A phase of the globals' workgroup: every
// thread has arrived, thread 0 stamps.
__device__ __forceinline__ void stamp_workgroup_phase(int i) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = device_clock((int)threadIdx.x);
        g_hdp_phase[i][0] = t; g_hdp_phase[i][1] = t;
    }
}
// entry / exit of every workgroup of launch `kid`: from the declaration to the end of its scope
struct WorkgroupSpan {
    int kid, blk;
    __device__ WorkgroupSpan(int kid_) : kid(kid_), blk((int)(blockIdx.x + gridDim.x * blockIdx.y)) {
        if (threadIdx.x == 0 && blk < HDP_T_ROWS) g_hdp_t[kid][blk][0] = device_clock((int)threadIdx.x);
    }
    __device__ ~WorkgroupSpan() {
        if (threadIdx.x == 0 && blk < HDP_T_ROWS) g_hdp_t[kid][blk][1] = device_clock((int)threadIdx.x);
    }
};

#else   // the product build: nothing is stamped

constexpr bool STAMP_PROLOGUE_PROBE = false;
template <StampArray A>
struct Stamps {
    __device__ Stamps(int = -1, int = -1) {}
    __device__ void mark_place(int) const {}
    __device__ unsigned long long get(int) const { return 0ull; }
    __device__ void set(int, unsigned long long) const {}
    __device__ void arm(bool) const {}
    __device__ static constexpr bool armed() { return false; }
    __device__ void flush(unsigned = ~0u) const {}
};
// (a macro, so that the value a stamp waits for is not evaluated here)
#define DLSM_STAMP(ST_, I_, DEP_)
__device__ __forceinline__ void stamp_workgroup_phase(int) {}
struct WorkgroupSpan {
    __device__ WorkgroupSpan(int) {}
};

#endif

}  // namespace dlsm
