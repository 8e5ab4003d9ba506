// k_matrix.hip -- products with the resident constraint matrix A (blu_matrix.inc: blu_hip_tableau_row, blu_hip_price).
//
//   k_scatter_lhs   the compressed solution a sparse solve left on the device (W.ilhs, W.xval, the count in W.out[0])
//                   into a dense vector y of m doubles that the host has cleared
//   k_at_dot        out[j] = column j of A dotted with y, for every column, in the summation order of the contract
//                   ("Resident constraint matrix"):
//                     n <= 64   s = +0.0, then s = s + a_x[q] * y[a_i[q]] in storage order
//                     n >  64   64 partial sums p[l] over q - a_p[j] = l, l + 64, ..., then p[l] = p[l] + p[l + w] for
//                               w = 32, 16, 8, 4, 2, 1; the result is p[0]
//                   Every product is rounded once (no fma: the build has -ffp-contract=off) and no term is left out.
//
// A wave takes a run of 64 consecutive columns, lane l column base + l.  Short columns are summed by their lane straight
// from global memory: the columns of a run lie one behind the other in a_i / a_x, so the 64 lanes walk one contiguous
// piece of a few KB that stays in the vector L1 between the steps of the walk, and every line of it comes from L2 once.
// Then the wave takes the long columns of its run one after the other, all 64 lanes on one column (coalesced), and hands
// the sum to the lane that owns the column.  Which wave and which lane a column falls on does not enter its sum.
// Row indices are below m (blu_hip_set_matrix refuses others), so y is gathered without a bound test.  skip[j] != 0:
// out[j] = +0.0 and the column is not read.
#include "blu_dev.h"

#define ATD_THREADS 256

struct MatA {
    const long long *ap; // ncol + 1 offsets, ap[0] = 0
    const int *ai;
    const double *ax;
};

__global__ __launch_bounds__(256) void k_scatter_lhs(const long long *__restrict__ cnt, const int *__restrict__ ilhs,
                                                     const double *__restrict__ xval, int m, double *__restrict__ y)
{
    const long long nz = min(cnt[0], (long long)m); // (a solve leaves 0 .. m entries, each row once)
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < nz; n += (long long)gridDim.x * blockDim.x) {
        const int i = ilhs[n];
        if ((unsigned)i < (unsigned)m) y[i] = xval[n];
    }
}

__global__ __launch_bounds__(ATD_THREADS) void k_at_dot(MatA A, const double *__restrict__ y, const unsigned char *__restrict__ skip,
                                                        int ncol, double *__restrict__ out)
{
    const int lane = (int)(threadIdx.x & 63);
    const long long base = ((long long)blockIdx.x * (ATD_THREADS / 64) + (long long)(threadIdx.x >> 6)) * 64;
    if (base >= ncol) return; // (the whole wave)
    const long long j = base + lane;
    const bool live = j < ncol && !(skip && skip[j]);
    long long b = 0;
    int n = 0;
    if (live) {
        b = A.ap[j];
        n = (int)(A.ap[j + 1] - b);
    }
    double s = 0.0;
    if (n <= 64)
        for (int q = 0; q < n; q++) s = s + A.ax[b + q] * y[A.ai[b + q]];
    unsigned long long longs = __ballot(n > 64);
    while (longs) { // (wave-uniform)
        const int l = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const long long lb = A.ap[base + l];
        const int ln = (int)(A.ap[base + l + 1] - lb);
        double p = 0.0;
        for (int q = lane; q < ln; q += 64) p = p + A.ax[lb + q] * y[A.ai[lb + q]];
        // p[l] + p[l + w] for l < w (what the lanes from w on compute is not read afterwards); the result is lane 0's
        for (int w = 32; w > 0; w >>= 1) p = p + __shfl_xor(p, w);
        p = __shfl(p, 0);
        if (lane == l) s = p;
    }
    if (j < ncol) out[j] = s;
}
