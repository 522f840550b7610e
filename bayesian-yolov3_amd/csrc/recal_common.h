// recal_common.h -- what the kernels of var_recal.hip and score_recal.hip share: the fixed sum and the segment bounds of the fits, the
// out-of-place prologue of the applies.  A header: the code is compiled under the including file's flags (build.py _EXACT_F32).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace byk {

__device__ __forceinline__ double recal_nan() { return __longlong_as_double(0x7ff8000000000000ll); }      // the quiet NaN of an empty fit

// The fixed sum of up to five quantities at once: lane t hands in its partial sums, lane q < nq adds the 256 partials of quantity q
// in ascending t, from 0.0 (tests/_var_recal_ref.py fixed_sum: the order is the contract).  Every lane returns with the totals in
// s_tot; a caller that reads them passes a barrier of its own before the next sum may write them.
__device__ __forceinline__ void recal_totals(double (*s_part)[256], double* s_tot, int nq, double p0, double p1, double p2, double p3, double p4) {
    const int tid = threadIdx.x;
    s_part[0][tid] = p0; s_part[1][tid] = p1; s_part[2][tid] = p2; s_part[3][tid] = p3; s_part[4][tid] = p4;
    __syncthreads();
    if (tid < nq) {
        double acc = 0.0;
        for (int t = 0; t < 256; ++t) acc += s_part[tid][t];
        s_tot[tid] = acc;
    }
    __syncthreads();
}

// The segment [lo, hi) of workgroup `s` of a fit: nothing is read outside [0, n_total) whatever the offsets say
__device__ __forceinline__ void recal_segment(const int64_t* seg, unsigned s, int64_t n_total, int64_t& lo, int64_t& hi) {
    lo = seg[s]; hi = seg[s + 1];
    lo = lo < 0 ? 0 : (lo > n_total ? n_total : lo);
    hi = hi < lo ? lo : (hi > n_total ? n_total : hi);
}

// The prologue of an apply that works out of place (P: VarRecalParams or ScoreRecalParams, n its row count): the workgroup copies
// its 256 rows from row0 on, every column, with consecutive lanes, and waits.  p is uniform over the workgroup, so is the branch.
template <class P>
__device__ __forceinline__ void recal_copy_rows(const P& p, int64_t row0, int64_t n) {
    if (p.out != p.in) {
        const int64_t rows = n - row0 < 256 ? n - row0 : 256;
        const int64_t e0 = row0 * p.D, cnt = rows * p.D;
        for (int64_t e = threadIdx.x; e < cnt; e += 256) p.out[e0 + e] = p.in[e0 + e];
        __syncthreads();
    }
}

}  // namespace byk
