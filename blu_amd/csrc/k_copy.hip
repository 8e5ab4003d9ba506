// k_copy.hip -- k_copy_fanout: the device state of ONE handle copied into n others in one launch
// (blu_hip_copy_batch, blu_copy.inc).
//
// The host describes the source as a list of SEGMENTS -- every array of the handle that carries state, with its live
// length in 4-byte words -- and gives, per segment and destination, the address of the same array in that destination.
// The segments are laid end to end in units of 16-byte TILES (a segment's last tile may be short); a workgroup takes
// COPY_THREADS * COPY_TILES consecutive tiles and a GROUP of destinations: it loads its tiles once, COPY_TILES loads
// per thread in flight, keeps them in registers and stores them to every destination of its group.  The source is read
// once per group, not once per destination; the groups exist so that a small basis still fills the chip when n is large.
// The grid is one-dimensional, tile blocks fastest: blockIdx.x = group * tblocks + tile block.
//
// Descriptors (DevLU, FinishOut) hold the DESTINATION's own pointers: the host builds one per destination and stages
// them as an array, and their segment has a source stride -- destination k reads src + k * stride.
//
// Every array of a handle starts 256-byte aligned (hipMalloc, the slab of blu_hip_new) except the canonical factors
// that live inside the column arena (ensure_out: 8-byte aligned); the host marks a segment `vec` when its source and
// all its destinations are 16-byte aligned, and only those go by 16-byte loads and stores, the others by words.
#include "blu_dev.h"

#define COPY_THREADS 256
#define COPY_TILES 4    // tiles per thread: 16 KB per workgroup and group of destinations

struct CopySeg {
    const char *src;
    long long tile0;    // first tile of the segment in the concatenation
    long long words;    // live length in 4-byte words (> 0)
    long long stride;   // bytes from destination k's source to destination k + 1's (0: one source for all)
    int vec;            // 1: source, stride and every destination are 16-byte aligned
    int pad0;
};

struct CopyTile {
    int seg;            // -1: nothing to do
    int cnt;            // words of the tile: 4, or 1..3 at the end of a segment
    long long off;      // byte offset of the tile inside its segment
};

__device__ __forceinline__ void copy_load(int4 &v, const char *p, int cnt, int vec)
{
    if (vec && cnt == 4) {
        v = *(const int4 *)p;
    } else {
        const int *q = (const int *)p;
        v.x = q[0];
        v.y = cnt > 1 ? q[1] : 0;
        v.z = cnt > 2 ? q[2] : 0;
        v.w = cnt > 3 ? q[3] : 0;
    }
}
__device__ __forceinline__ void copy_store(char *p, const int4 &v, int cnt, int vec)
{
    if (vec && cnt == 4) {
        *(int4 *)p = v;
    } else {
        int *q = (int *)p;
        q[0] = v.x;
        if (cnt > 1) q[1] = v.y;
        if (cnt > 2) q[2] = v.z;
        if (cnt > 3) q[3] = v.w;
    }
}

// dsts[s * n + k]: where segment s of destination k starts
__global__ void __launch_bounds__(COPY_THREADS) k_copy_fanout(const CopySeg *__restrict__ segs, int nseg, char *const *__restrict__ dsts, int n,
                                                              int group, int tblocks, long long ntiles)
{
    const int tb = (int)(blockIdx.x % (unsigned)tblocks), g = (int)(blockIdx.x / (unsigned)tblocks);
    const int k0 = g * group, k1 = min(n, k0 + group);
    CopyTile T[COPY_TILES];
    int4 v[COPY_TILES];
#pragma unroll
    for (int j = 0; j < COPY_TILES; j++) {
        const long long t = ((long long)tb * COPY_TILES + j) * COPY_THREADS + threadIdx.x;
        T[j].seg = -1;
        T[j].cnt = 0;
        T[j].off = 0;
        v[j].x = v[j].y = v[j].z = v[j].w = 0;
        if (t < ntiles) {
            int lo = 0, hi = nseg - 1; // the last segment that starts at or before tile t
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (segs[mid].tile0 <= t) lo = mid;
                else hi = mid - 1;
            }
            const long long w0 = (t - segs[lo].tile0) * 4;
            const long long left = segs[lo].words - w0;
            T[j].seg = lo;
            T[j].cnt = left < 4 ? (int)left : 4;
            T[j].off = w0 * 4;
            if (segs[lo].stride == 0) copy_load(v[j], segs[lo].src + T[j].off, T[j].cnt, segs[lo].vec);
        }
    }
#pragma unroll
    for (int j = 0; j < COPY_TILES; j++) {
        const int s = T[j].seg;
        if (s < 0 || T[j].cnt <= 0) continue;
        const int vec = segs[s].vec;
        const long long stride = segs[s].stride;
        char *const *d = dsts + (size_t)s * (size_t)n;
        for (int k = k0; k < k1; k++) {
            if (stride) copy_load(v[j], segs[s].src + (long long)k * stride + T[j].off, T[j].cnt, vec);
            copy_store(d[k] + T[j].off, v[j], T[j].cnt, vec);
        }
    }
}
