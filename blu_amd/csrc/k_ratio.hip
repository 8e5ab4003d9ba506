// k_ratio.hip -- the dual ratio test on the resident duals (blu_ratio.inc: blu_hip_ratio_test, blu_hip_update_duals,
// blu_hip_copy_duals_batch and their batch entries).
//
//   k_ratio_pick        one workgroup: the selection rule of the contract (include/blu_hip.h, "Ratio test on the device")
//                       over one tableau row, the reduced costs d and the bound status kind of a handle
//   k_ratio_pick_batch  one workgroup per member of a chunk: the same over that member's row of the products block of
//                       k_at_dot_batch, which the first pass also stores into the member's kept-row buffer
//   k_duals_axpy(_batch), k_duals_set(_batch)   the dual step d[j] = d[j] - theta * row[j] where kind[j] != 0 (the product
//                       rounded once, then the difference: the build has -ffp-contract=off), and the overrides behind it
//   k_duals_fanout      d and kind of one handle into those of n others
//
// The pick makes two passes over the row.  Pass 1: a thread walks j = tid, tid + blockDim.x, ... and keeps the smallest
// bound_j = (|d_j| + dualtol) / |alpha_j| of its candidates and their count; the waves reduce with __shfl_xor, the
// workgroup through LDS, and theta = min bound_j is broadcast.  Pass 2 (the data sits in L2): among the candidates with
// step_j = |d_j| / |alpha_j| <= theta the key (|alpha_j| largest, then j smallest) is reduced the same way.  A minimum of
// non-NaN doubles and the maximum of a total order are exact whatever the order of evaluation is, so no bit of the
// record depends on the workgroup size, on ncol or on a member's place in the chunk.  One thread writes the 64-byte
// record with plain vector stores; there are no global atomics.
#include "blu_dev.h"

#define PICK_THREADS 1024      // the single entry: one workgroup over the whole row
#define PICK_THREADS_BATCH 256 // one workgroup per member
#define DUALS_THREADS 256

struct RatioRec { // = blu_ratio_result
    long long q, ncand;
    double alpha_q, d_q, step, bound;
    long long reserved[2];
};

struct PickSrc { // one member of a chunk of blu_hip_ratio_test_batch
    const double *d;
    const signed char *kind;
    double *keep; // its kept-row buffer
    double sigma;
};

// is column j a candidate, and with which a = |alpha| and bound
static __device__ __forceinline__ bool ratio_candidate(double al, double dj, int kd, double sigma, double pivtol, double dualtol, double &a,
                                                       double &bound)
{
    a = fabs(al);
    const double s = sigma * al; // (exact: sigma is +1 or -1)
    if (!((kd == 1 && s > pivtol) || (kd == -1 && s < -pivtol) || (kd == 2 && a > pivtol))) return false;
    const double num = fabs(dj) + dualtol;
    bound = num / a;
    return bound == bound; // (a NaN bound: no candidate)
}

static __device__ __forceinline__ void ratio_pick_body(const double *__restrict__ row, double *__restrict__ keep, const double *__restrict__ d,
                                                       const signed char *__restrict__ kind, int ncol, double sigma, double pivtol,
                                                       double dualtol, RatioRec *__restrict__ rec)
{
    __shared__ double s_val[16];
    __shared__ int s_int[16];
    __shared__ double s_theta;
    __shared__ int s_total;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = (int)(blockDim.x >> 6);

    // pass 1: theta = the smallest bound, and the number of candidates
    double mn = __builtin_inf();
    int cnt = 0;
    for (long long j = tid; j < ncol; j += blockDim.x) {
        const double al = row[j];
        if (keep) keep[j] = al;
        double a, b;
        if (ratio_candidate(al, d[j], kind[j], sigma, pivtol, dualtol, a, b)) {
            cnt++;
            if (b < mn) mn = b;
        }
    }
    for (int w = 32; w > 0; w >>= 1) {
        const double o = __shfl_xor(mn, w);
        if (o < mn) mn = o;
        cnt += __shfl_xor(cnt, w);
    }
    if (lane == 0) {
        s_val[wave] = mn;
        s_int[wave] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nwave; w++) {
            if (s_val[w] < mn) mn = s_val[w];
            cnt += s_int[w];
        }
        s_theta = mn;
        s_total = cnt;
    }
    __syncthreads();
    const double theta = s_theta;
    const int total = s_total;

    // pass 2: among the candidates with step <= theta, the largest |alpha|, then the smallest j
    double ab = -1.0;
    int jb = 0x7fffffff;
    if (total > 0)
        for (long long j = tid; j < ncol; j += blockDim.x) {
            const double dj = d[j];
            double a, b;
            if (!ratio_candidate(row[j], dj, kind[j], sigma, pivtol, dualtol, a, b)) continue;
            if (!(fabs(dj) / a <= theta)) continue;
            if (a > ab || (a == ab && (int)j < jb)) {
                ab = a;
                jb = (int)j;
            }
        }
    for (int w = 32; w > 0; w >>= 1) {
        const double oa = __shfl_xor(ab, w);
        const int oj = __shfl_xor(jb, w);
        if (oa > ab || (oa == ab && oj < jb)) {
            ab = oa;
            jb = oj;
        }
    }
    if (lane == 0) {
        s_val[wave] = ab;
        s_int[wave] = jb;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nwave; w++)
            if (s_val[w] > ab || (s_val[w] == ab && s_int[w] < jb)) {
                ab = s_val[w];
                jb = s_int[w];
            }
        RatioRec R;
        R.q = -1;
        R.ncand = total;
        R.alpha_q = R.d_q = R.step = R.bound = 0.0;
        R.reserved[0] = R.reserved[1] = 0;
        if (total > 0 && jb < ncol) {
            R.q = jb;
            R.alpha_q = row[jb];
            R.d_q = d[jb];
            R.step = fabs(R.d_q) / fabs(R.alpha_q);
            R.bound = theta;
        }
        *rec = R;
    }
}

__global__ __launch_bounds__(PICK_THREADS) void k_ratio_pick(const double *__restrict__ row, const double *__restrict__ d,
                                                              const signed char *__restrict__ kind, int ncol, double sigma, double pivtol,
                                                              double dualtol, RatioRec *__restrict__ rec)
{
    ratio_pick_body(row, nullptr, d, kind, ncol, sigma, pivtol, dualtol, rec);
}

// member blockIdx.x of the chunk: its row of the products block (ncol doubles per member)
__global__ __launch_bounds__(PICK_THREADS_BATCH) void k_ratio_pick_batch(const PickSrc *__restrict__ src, const double *__restrict__ products,
                                                                          int ncol, double pivtol, double dualtol, RatioRec *__restrict__ recs)
{
    const PickSrc S = src[blockIdx.x];
    ratio_pick_body(products + (size_t)blockIdx.x * (size_t)ncol, S.keep, S.d, S.kind, ncol, S.sigma, pivtol, dualtol, recs + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// The dual step and the overrides.  A batch launches nbx workgroups per member behind each other (blockIdx.x / nbx is the
// member), as k_at_dot_batch does.
struct DualSet { // one override: d[j] = d, kind[j] = k
    double d;
    int j, k;
};
struct DualStep { // one member of blu_hip_update_duals_batch
    double *d;
    signed char *kind;
    const double *row;
    double theta;
    long long set0; // its overrides: sets[set0 .. set0 + nset)
    int nset;
};

static __device__ __forceinline__ void duals_axpy_body(double *__restrict__ d, const double *__restrict__ row, const signed char *__restrict__ kind,
                                                       double theta, int ncol, unsigned bx, unsigned nbx)
{
    for (long long j = (long long)bx * blockDim.x + threadIdx.x; j < ncol; j += (long long)nbx * blockDim.x)
        if (kind[j] != 0) {
            const double t = theta * row[j];
            d[j] = d[j] - t;
        }
}
static __device__ __forceinline__ void duals_set_body(double *__restrict__ d, signed char *__restrict__ kind, const DualSet *__restrict__ sets,
                                                      int nset, int ncol)
{
    for (int t = (int)threadIdx.x; t < nset; t += (int)blockDim.x) {
        const DualSet S = sets[t];
        if ((unsigned)S.j < (unsigned)ncol) { // (the host has checked it)
            d[S.j] = S.d;
            kind[S.j] = (signed char)S.k;
        }
    }
}

__global__ __launch_bounds__(DUALS_THREADS) void k_duals_axpy(double *__restrict__ d, const double *__restrict__ row,
                                                               const signed char *__restrict__ kind, double theta, int ncol)
{
    duals_axpy_body(d, row, kind, theta, ncol, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(DUALS_THREADS) void k_duals_set(double *__restrict__ d, signed char *__restrict__ kind,
                                                              const DualSet *__restrict__ sets, int nset, int ncol)
{
    duals_set_body(d, kind, sets, nset, ncol);
}
__global__ __launch_bounds__(DUALS_THREADS) void k_duals_axpy_batch(const DualStep *__restrict__ steps, int ncol, int nbx)
{
    const DualStep S = steps[blockIdx.x / (unsigned)nbx];
    duals_axpy_body(S.d, S.row, S.kind, S.theta, ncol, blockIdx.x % (unsigned)nbx, (unsigned)nbx);
}
// one workgroup per member
__global__ __launch_bounds__(DUALS_THREADS) void k_duals_set_batch(const DualStep *__restrict__ steps, const DualSet *__restrict__ sets, int ncol)
{
    const DualStep S = steps[blockIdx.x];
    duals_set_body(S.d, S.kind, sets + S.set0, S.nset, ncol);
}

struct DualDst {
    double *d;
    signed char *kind;
};
// d and kind of the source into n destinations: nbx workgroups per destination
__global__ __launch_bounds__(DUALS_THREADS) void k_duals_fanout(const double *__restrict__ d, const signed char *__restrict__ kind,
                                                                 const DualDst *__restrict__ dst, int ncol, int nbx)
{
    const DualDst D = dst[blockIdx.x / (unsigned)nbx];
    for (long long j = (long long)(blockIdx.x % (unsigned)nbx) * blockDim.x + threadIdx.x; j < ncol; j += (long long)nbx * blockDim.x) {
        D.d[j] = d[j];
        D.kind[j] = kind[j];
    }
}
