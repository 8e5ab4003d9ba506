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

// by_kind (a constant at both call sites): the bytes are the kind[] of the resident duals (k_ratio.hip), and it is
// kind[j] == 0 that skips column j
static __device__ __forceinline__ void at_dot_body(MatA A, const double *__restrict__ y, const unsigned char *__restrict__ skip, const bool by_kind,
                                                   int ncol, double *__restrict__ out)
{
    const int lane = (int)(threadIdx.x & 63);
    const long long base = ((long long)blockIdx.x * (ATD_THREADS / 64) + (long long)(threadIdx.x >> 6)) * 64;
    if (base >= ncol) return; // (the whole wave)
    const long long j = base + lane;
    const bool live = j < ncol && !(skip && (by_kind ? skip[j] == 0 : skip[j] != 0));
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

__global__ __launch_bounds__(ATD_THREADS) void k_at_dot(MatA A, const double *__restrict__ y, const unsigned char *__restrict__ skip,
                                                        int ncol, double *__restrict__ out)
{
    at_dot_body(A, y, skip, false, ncol, out);
}

// blu_hip_ratio_test (blu_ratio.inc): the same products, a column skipped where kind[j] == 0
__global__ __launch_bounds__(ATD_THREADS) void k_at_dot_kind(MatA A, const double *__restrict__ y, const signed char *__restrict__ kind,
                                                             int ncol, double *__restrict__ out)
{
    at_dot_body(A, y, (const unsigned char *)kind, true, ncol, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// The batched products (blu_matrix_batch.inc: blu_hip_tableau_row_batch, blu_hip_price_batch): many y against one A.
//
// The y vectors of a call are stored member-interleaved in groups of ATB_G = 8: the tile of group g holds
// Y[g][i * 8 + t] for row i and member t of the group, so the eight y values of a row are one contiguous 64-byte piece.
//
//   k_scatter_lhs_batch   one workgroup per member: k_scatter_lhs of that member's compressed solution (the count read from
//                         its sw.out[0] on the device) into its column of the tile, which the host has cleared
//   k_at_dot_batch        out[member][j] = column j of A dotted with that member's y.  A group has nbx workgroups of the
//                         grid behind each other (blockIdx.x / nbx is the group); a wave takes
//                         a run of 64 consecutive columns, lane l column base + l, exactly as k_at_dot, but every entry
//                         a_i[q] / a_x[q] it loads serves the eight members of the group: A is read once per group, not
//                         once per member.  Each member keeps a sum of its own, s[t] = s[t] + a_x[q] * y_t[a_i[q]] in
//                         storage order (n <= 64), or its own 64 strided partial sums and halving tree p[l] + p[l + w]
//                         (n > 64): the chain of additions of a member is that of k_at_dot, so its bits are.
// A skip is one byte per column per group, bit t for member t: that member's result is forced to +0.0; the column is
// read unless every present member of the group skips it.  A last, partial group has zero y columns for its absent
// members and does not store their rows.  ATB_G is chosen by reasoning ("Shared matrix, batched rows"): 64
// bytes per gather is half a cache line, 16 + 16 VGPRs hold the sums and the y values, and A is fetched n / 8 times.
// No result depends on it.
#define ATB_G 8

struct alignas(16) YRow {
    double v[ATB_G];
};
struct ScatterSrc { // one member's compressed solution on the device
    const long long *cnt;
    const int *ilhs;
    const double *xval;
};

__global__ __launch_bounds__(256) void k_scatter_lhs_batch(const ScatterSrc *__restrict__ src, int m, double *__restrict__ Y)
{
    const ScatterSrc S = src[blockIdx.x];
    double *y = Y + (size_t)(blockIdx.x / ATB_G) * (size_t)m * ATB_G + (blockIdx.x % ATB_G);
    const long long nz = min(S.cnt[0], (long long)m);
    for (long long n = threadIdx.x; n < nz; n += blockDim.x) {
        const int i = S.ilhs[n];
        if ((unsigned)i < (unsigned)m) y[(size_t)i * ATB_G] = S.xval[n];
    }
}

// c members in the chunk: groups 0 .. (c + 7) / 8 - 1, nbx workgroups each; mask may be NULL (no member skips anything)
__global__ __launch_bounds__(ATD_THREADS) void k_at_dot_batch(MatA A, const double *__restrict__ Y, const unsigned char *__restrict__ mask,
                                                              int ncol, int m, int c, int nbx, double *__restrict__ out)
{
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x / (unsigned)nbx);
    const long long base = ((long long)(blockIdx.x % (unsigned)nbx) * (ATD_THREADS / 64) + (long long)(threadIdx.x >> 6)) * 64;
    if (base >= ncol) return; // (the whole wave)
    const int present = min(ATB_G, c - g * ATB_G); // members of this group
    const unsigned all = (1u << present) - 1u;
    const YRow *__restrict__ yg = (const YRow *)(Y + (size_t)g * (size_t)m * ATB_G);
    const long long j = base + lane;
    unsigned sk = 0;
    if (mask && j < ncol) sk = mask[(size_t)g * (size_t)ncol + (size_t)j];
    const bool live = j < ncol && (sk & all) != all;
    long long b = 0;
    int n = 0;
    if (live) {
        b = A.ap[j];
        n = (int)(A.ap[j + 1] - b);
    }
    double s[ATB_G];
#pragma unroll
    for (int t = 0; t < ATB_G; t++) s[t] = 0.0;
    if (n <= 64)
        for (int q = 0; q < n; q++) {
            const double x = A.ax[b + q];
            const YRow yr = yg[A.ai[b + q]];
#pragma unroll
            for (int t = 0; t < ATB_G; t++) s[t] = s[t] + x * yr.v[t];
        }
    unsigned long long longs = __ballot(n > 64);
    while (longs) { // (wave-uniform)
        const int l = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const long long lb = A.ap[base + l];
        const int ln = (int)(A.ap[base + l + 1] - lb);
        double p[ATB_G];
#pragma unroll
        for (int t = 0; t < ATB_G; t++) p[t] = 0.0;
        for (int q = lane; q < ln; q += 64) {
            const double x = A.ax[lb + q];
            const YRow yr = yg[A.ai[lb + q]];
#pragma unroll
            for (int t = 0; t < ATB_G; t++) p[t] = p[t] + x * yr.v[t];
        }
#pragma unroll
        for (int t = 0; t < ATB_G; t++) {
            double v = p[t];
            // p[l] + p[l + w] for l < w; the result is lane 0's
            for (int w = 32; w > 0; w >>= 1) v = v + __shfl_xor(v, w);
            v = __shfl(v, 0);
            if (lane == l) s[t] = v;
        }
    }
    if (j < ncol) {
#pragma unroll
        for (int t = 0; t < ATB_G; t++)
            if (t < present) out[(size_t)(g * ATB_G + t) * (size_t)ncol + (size_t)j] = ((sk >> t) & 1u) ? 0.0 : s[t];
    }
}
