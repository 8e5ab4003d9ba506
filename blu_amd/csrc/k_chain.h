// k_chain.h -- triangular sweeps as a decoupled access / execute pipeline, one workgroup per sweep chain.
//
// A triangular sweep (condest.rs, residual_test.rs, solve_dense.rs) is a chain of m dependent steps.  On the
// banded LP bases the chain is real: the U of the C3 basis has a dependency path of 50 380 steps (SURVEY 8d's
// tri_frac = 0.5 part is one long chain; L has depth 571), so level scheduling has nothing to offer there and
// what counts is the time of ONE step.  k_sweep.h runs a sweep on one wave that also fetches its own operands
// from global memory one and two steps ahead: a step then takes a global round trip (~0.85 us), because the
// wave has to wait for the loads of this step before it can start the next.
//
// Here the waves that walk the chain never load from global memory.  The other waves of the workgroup
// (helpers) stream the operands of the coming steps into LDS rings -- step records (length, pivot, own value,
// output index) and entries (value, and WHERE the operand of the work vector is found) -- hundreds of steps
// ahead of the chain; the chain reads LDS only (the records of a block once, a step's fields by v_readlane)
// and its step is the arithmetic: products, the ordered sum in the reference's order, the step function (one
// f64 division), one LDS and one global store.  Work-vector operands come from
//   * a window of the last CH_W results in LDS (xwin, written by the chain),
//   * for producers at least CH_FAR steps back: the value gathered from global memory by the helper (final by
//     then: a helper stages a block only after every ring wave has published -- stores drained -- a progress
//     that puts every such producer behind it).  The leading terms of a step that are of this kind are added by
//     the helper itself, in the step's order and with the chain's roundings: the chain starts behind them.
//
// The chain is walked by a RING of CH_R waves (waves 0..CH_R-1; ring wave r takes steps r, r + CH_R, ...), because
// what step s truly waits for is little: of its ordered sum only the terms from the first one whose producer is
// less than CH_R steps back, and the step function.  The record fields, the entries, the window operands of older
// producers, their products and the leading part of the sum need nothing newer than step s - CH_R, which the wave
// published itself, and every earlier step was published before that one: steps are published strictly in sweep
// order (xwin slot, LDS fence, then tag[s & (CH_TG-1)] = s + 1; a step waits for its predecessor's tag before it
// sets its own, also when it has no late term).  So a ring wave does that EARLY part while its predecessors are
// still at work, waits for the tag of step s - 1, and the LATE part -- read the window for the late entries,
// products, the rest of the sum in order, step function, publish -- is all that is left on the critical path.
// Every sweep is in GATHER form: step k reads results of earlier steps only.  The reference's scatter-form
// loops (x[i] -= t_k * a_ik over column k, k in sweep order) are run over the transposed storage -- row-wise L
// ascending, U rows descending in the pivot order (k_rows_grid below) -- accumulating into the step's own
// entry in the same order with the same two roundings per term, so all results stay bit-identical.
//
// Flow control (LDS, in-order per wave): helpers take blocks of CH_SB steps round-robin; the entry-ring base of a
// block is handed from the helper of the previous block as soon as that one knows its entry count; a block is
// staged only when its step-ring slots (every ring wave CH_NB blocks behind) and its entry-ring space are free:
// each ring wave drains its own stores when it leaves a block and publishes its own progress, and the room test
// takes the minimum; a ring wave waits for blk_ready of the block it enters.  Steps with more than 64 entries are
// not staged: the ring wave waits for its predecessor and takes the entries straight from global memory, each
// operand from the window (producer less than CH_FAR back) or, final by the argument above, from global memory.
#pragma once
#include "blu_dev.h"

#define CH_SB 32                 // steps per block
#define CH_NB 8                  // blocks in the step ring
#define CH_CS (CH_SB * CH_NB)    // step ring
#define CH_CE 4096               // entry ring (two full blocks of 64-entry steps)
#define CH_W 2048                // window of results kept in LDS (positions)
#define CH_FAR 320               // a producer this many steps back is final and visible when a helper stages (> CH_CS)
#define CH_HAS 0x10000           // record: the step has entries (some or all may have gone into `init` already)
#define CH_HT 16                 // hand-off ring of entry bases
#define CH_SEL_FAR (-1)          // operand: the helper's gathered value
#define CH_SEL_PREV (-2)         // operand: the previous step's result (its window slot)
#define CH_R 4                   // ring waves (waves 0..CH_R-1); the workgroup's other waves are helpers
#define CH_TG 64                 // ring of step tags
#define CH_SPIN 64               // polls of a predecessor's tag before the wait starts to sleep between polls

struct __attribute__((aligned(16))) ChRecA { // what the chain wave reads of a step, in two 16-byte LDS reads
    int n, eb, w, k;
};
struct __attribute__((aligned(16))) ChRecB {
    double diag, own;
};
struct __attribute__((aligned(16))) ChOpsV {
    double val, xv;
};
struct ChainLds {
    ChOpsV ev[CH_CE];
    int sel[CH_CE];
    double xwin[CH_W];
    ChRecA ra[CH_CS];
    ChRecB rb[CH_CS];
    double rinit[CH_CS]; // the accumulator's start: own value or 0, plus the leading terms the helper has added already
    long long s_b[CH_CS];
    volatile int blk_ready[CH_NB];
    volatile int eb_tag[CH_HT];
    volatile int eb_val[CH_HT];
    volatile int tag[CH_TG];        // tag[s & (CH_TG-1)] == s + 1: step s is in the window, and so is every earlier step
    volatile int ring_done[CH_R];    // per ring wave: blocks it has finished with its stores drained
    volatile int ring_eb[CH_R];      // per ring wave: entry-ring position of the first entry of the block it is in
    volatile int abort;      // a wait ran into its bound (a defect, never a valid state): everybody leaves
};

struct ChMeta {
    long long b; // storage offset of the step's entries
    int len;     // number of entries
    int w;       // index of the output vector the step writes
    double diag, own;
};
struct ChEnt {
    int pos;  // sweep position k of the producer (0..m-1)
    int gidx; // its index in the output vector
    double val;
};

// The flags other waves poll are volatile, and a volatile access through a generic pointer stays a FLAT instruction (the
// address-space inference leaves volatile accesses alone): several times the latency of a ds_ instruction on every poll and
// every publication.  They are read and written through these two, with the LDS address space spelled out.
#ifdef BLU_EMU_BUILD
#define CH_LDS(T) T *
#else
#define CH_LDS(T) __attribute__((address_space(3))) T *
#endif
__device__ __forceinline__ int ch_flag(const volatile int *p) { return *(CH_LDS(const volatile int))p; }
__device__ __forceinline__ void ch_set(volatile int *p, int v) { *(CH_LDS(volatile int))p = v; }

// Bounded wait on LDS state written by another wave: 2^24 polls of s_sleep(1) (of the order of a second) and the
// sweep is abandoned with an error instead of hanging the GPU; the callers report the code to the host, which
// never uses the results of an abandoned sweep.  The first `spin` polls follow one another without a sleep (the
// hand-over from step to step); `gave_up` is set when the wait ended without its condition.
#define CH_WAIT_SPIN(L, cond, code, spin, gave_up)                  \
    do {                                                            \
        int it_ = 0;                                                \
        while (!(cond)) {                                           \
            if (++it_ <= (spin)) continue;                          \
            if (ch_flag(&(L)->abort) || it_ > (1 << 24)) {                    \
                if (!ch_flag(&(L)->abort)) ch_set(&(L)->abort, (code));               \
                (gave_up) = true;                                   \
                break;                                              \
            }                                                       \
            __builtin_amdgcn_s_sleep(1);                            \
        }                                                           \
    } while (0)
#define CH_WAIT(L, cond, code)                       \
    do {                                             \
        bool gu_ = false;                            \
        CH_WAIT_SPIN(L, cond, code, 0, gu_);         \
    } while (0)

#ifdef BLU_EMU_BUILD // (CPU emulation build: memory is always current; the DPP sum below through the emulator's exchange)
__device__ __forceinline__ void ch_lds_fence() {}
__device__ __forceinline__ void ch_vm_drain() {}
#else
__device__ __forceinline__ void ch_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void ch_vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#endif
__device__ __forceinline__ double ch_load_final(gdouble_p p)
{
    // a value another wave of this workgroup stored some time ago: read past this CU's vector cache
    const long long b = __hip_atomic_load((GPTR(const long long))p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double(b);
}

// ---- helper side: stage block b ---------------------------------------------------------------------------
// room for block b, whose entries end at entry-ring position `top`: the slowest ring wave decides (each counter only
// grows, so a value read a moment early errs on the safe side)
__device__ __forceinline__ bool ch_room(ChainLds *L, int b, int top)
{
    int done = ch_flag(&L->ring_done[0]), eb = ch_flag(&L->ring_eb[0]);
#pragma unroll
    for (int r = 1; r < CH_R; r++) {
        const int d = ch_flag(&L->ring_done[r]), e = ch_flag(&L->ring_eb[r]);
        done = d < done ? d : done;
        eb = e < eb ? e : eb;
    }
    return done >= b - CH_NB + 1 && top - eb <= CH_CE;
}
template <bool INIT_OWN, bool SUB, class A>
__device__ __forceinline__ void ch_stage_block(const A &ad, ChainLds *L, int b, int k0, int dir, int nsteps, gdouble_p out)
{
    const int lane = lane_id();
    const int s0 = b * CH_SB;
    const int ns = nsteps - s0 < CH_SB ? nsteps - s0 : CH_SB;
    const int k = k0 + dir * (s0 + (lane < ns ? lane : 0));
    ChMeta M = ad.meta(k);
    if (M.len < 0) M.len = 0; // (defensive: a negative length would make the loops below unbounded)
    const bool mine = lane < ns;
    const int st = (mine && M.len <= 64) ? M.len : 0;
    const int incl = wave_incl_scan_i(st);
    const int off = incl - st;
    const int cnt = __builtin_amdgcn_readlane(incl, 63);
    // entry-ring base: from the helper of the previous block
    int base = 0;
    if (b > 0) {
        CH_WAIT(L, ch_flag(&L->eb_tag[b & (CH_HT - 1)]) == b, 1);
        base = ch_flag(&L->eb_val[b & (CH_HT - 1)]);
    }
    if (lane == 0) {
        ch_set(&L->eb_val[(b + 1) & (CH_HT - 1)], base + cnt);
        ch_lds_fence();
        ch_set(&L->eb_tag[(b + 1) & (CH_HT - 1)], b + 1);
    }
    // room: step-ring slots of block b - CH_NB, entry-ring space; this also makes every result further back
    // than the window final and visible (see the header)
    CH_WAIT(L, ch_room(L, b, base + cnt), 2);
    asm volatile("" ::: "memory");
    if (ch_flag(&L->abort)) return;
    const int slot0 = s0 & (CH_CS - 1);
    if (mine) {
        const int sl = slot0 + lane;
        ChRecA a;
        a.n = M.len <= 64 ? (M.len > 0 ? (M.len | CH_HAS) : 0) : -1;
        a.eb = base + off;
        a.w = M.w;
        a.k = k;
        L->ra[sl] = a;
        ChRecB bq;
        bq.diag = M.diag;
        bq.own = M.own;
        L->rb[sl] = bq;
        L->rinit[sl] = INIT_OWN ? M.own : 0.0;
        L->s_b[sl] = M.b;
    }
    ch_lds_fence();
    // entries, flat over the block: 4 x 64 per pass, loads of a pass issued together
    for (int f0 = 0; f0 < cnt; f0 += 256) {
        int tt[4], ee[4];
        ChEnt E[4];
        bool ok[4], far[4];
        double xo[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int f = f0 + u * 64 + lane;
            ok[u] = f < cnt;
            // step of flat entry f: the last t with s_eb[t] - base <= f (binary search over the block's records)
            int lo = 0, hi = ns - 1;
            const int target = base + (ok[u] ? f : 0);
#pragma unroll
            for (int it = 0; it < 5; it++) {
                const int mid = (lo + hi + 1) >> 1;
                const bool ge = (L->ra[slot0 + mid].eb <= target) && (mid <= hi);
                lo = ge ? mid : lo;
                hi = ge ? hi : mid - 1;
            }
            // skip unstaged / empty steps that share the same base: take the LAST step with s_eb <= target that has entries
            tt[u] = lo;
            ee[u] = target - L->ra[slot0 + lo].eb;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            E[u].pos = 0;
            E[u].gidx = 0;
            E[u].val = 0.0;
            if (ok[u]) E[u] = ad.ent(L->ra[slot0 + tt[u]].k, L->s_b[slot0 + tt[u]], ee[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = L->ra[slot0 + tt[u]].k;
            const int d = (kk - E[u].pos) * dir;
            far[u] = ok[u] && d >= CH_FAR;
            xo[u] = 0.0;
            if (far[u]) xo[u] = ch_load_final(out + E[u].gidx);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (ok[u]) {
                const int kk = L->ra[slot0 + tt[u]].k;
                const int r = (base + f0 + u * 64 + lane) & (CH_CE - 1);
                ChOpsV ov;
                ov.val = E[u].val;
                ov.xv = xo[u];
                L->ev[r] = ov;
                L->sel[r] = far[u] ? CH_SEL_FAR : (E[u].pos == kk - dir ? CH_SEL_PREV : (E[u].pos & (CH_W - 1)));
            }
        }
    }
    ch_lds_fence();
    // The leading terms of a step whose producers are that far back are final: this lane (one per step) adds them in
    // the step's order, with the chain wave's two roundings per term, and the chain wave starts behind them.  (Lines
    // sorted in sweep order -- canonical U columns, row-wise L, sorted U rows -- have all such terms in front.)
    if (mine && M.len > 0 && M.len <= 64) {
        const int sl = slot0 + lane;
        const int eb = base + off;
        double acc = INIT_OWN ? M.own : 0.0;
        int p = 0;
        while (p < M.len && L->sel[(eb + p) & (CH_CE - 1)] == CH_SEL_FAR) {
            const ChOpsV ov = L->ev[(eb + p) & (CH_CE - 1)];
            const double term = __dmul_rn(ov.xv, ov.val);
            acc = SUB ? __dsub_rn(acc, term) : __dadd_rn(acc, term);
            p++;
        }
        if (p > 0) {
            L->ra[sl].n = (M.len - p) | CH_HAS;
            L->ra[sl].eb = eb + p;
            L->rinit[sl] = acc;
        }
    }
    ch_lds_fence();
    if (lane == 0) ch_set(&L->blk_ready[b & (CH_NB - 1)], b + 1);
}

// ---- chain side -------------------------------------------------------------------------------------------
struct ChRec {
    int n, eb, w, k; // n: entries left for the chain wave | CH_HAS, or -1 (long step)
    double diag, own, init;
};
struct ChOps {
    double val, xv;
    int sel;
};
// (the four integers stay in vector registers while the record travels through the look-ahead stages: turning them
// into scalars right after the LDS read would make the wave wait for the read in the middle of every step)
__device__ __forceinline__ ChRec ch_read_rec(ChainLds *L, int s)
{
    const int sl = s & (CH_CS - 1);
    const ChRecA a = L->ra[sl];
    const ChRecB b = L->rb[sl];
    ChRec R;
    R.n = a.n;
    R.eb = a.eb;
    R.w = a.w;
    R.k = a.k;
    R.diag = b.diag;
    R.own = b.own;
    R.init = L->rinit[sl];
    return R;
}
// acc -/+= the products of lanes 0..n-1, in lane order (the reference's sequential loop)
template <bool SUB>
__device__ __forceinline__ double ch_accumulate(double acc, double prod, int n)
{
    const unsigned lo = (unsigned)__double_as_longlong(prod), hi = (unsigned)(__double_as_longlong(prod) >> 32);
#define CH_TERM(T)                                                                                              \
    {                                                                                                           \
        const unsigned a_ = __builtin_amdgcn_readlane(lo, (T)), b_ = __builtin_amdgcn_readlane(hi, (T));        \
        const double term_ = __longlong_as_double((long long)(((unsigned long long)b_ << 32) | a_));            \
        acc = SUB ? __dsub_rn(acc, term_) : __dadd_rn(acc, term_);                                              \
    }
    int t = 0;
    for (; t + 4 <= n; t += 4) {
        CH_TERM(t)
        CH_TERM(t + 1)
        CH_TERM(t + 2)
        CH_TERM(t + 3)
    }
    for (; t < n; t++) CH_TERM(t)
#undef CH_TERM
    return acc;
}

// The same for at most 16 terms when every row of 16 lanes holds the products (lane l: term l & 15): one instruction
// per term.  v_fmac_f64 is the one 64-bit VALU operation of gfx90a+ that takes a DPP operand, with row_newbcast:t
// (lane t of the row to the whole row); acc = fma(term_t, +-1.0, acc) rounds once, exactly like acc +- term_t.  Three
// instructions per term otherwise (two v_readlane and the add).  An s_nop covers the VALU-write -> DPP-read hazards (2 wait states after a write of the operand, 5 after a VALU write of EXEC)
// of the products, which the compiler cannot see inside the asm.
template <bool SUB>
__device__ __forceinline__ double ch_accumulate_rows(double acc, double prod, int n)
{
    const double sg = SUB ? -1.0 : 1.0;
#ifdef BLU_EMU_BUILD
#define CH_D(T) acc = fma(__shfl(prod, (lane_id() & ~15) + T), sg, acc);
#define CH_D0 CH_D(0)
#else
#define CH_D(T) asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #T " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(prod), "v"(sg));
// (term 0 is the first in every path: the wait states ride in the same asm statement, where no scheduler can move them)
#define CH_D0 asm volatile("s_nop 4\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(prod), "v"(sg));
#endif
#define CH_TAIL(A, B, C) \
    if (n > A) {         \
        CH_D(A)          \
        if (n > B) {     \
            CH_D(B)      \
            if (n > C) { \
                CH_D(C)  \
            }            \
        }                \
    }
    if (n >= 4) {
        CH_D0 CH_D(1) CH_D(2) CH_D(3)
        if (n >= 8) {
            CH_D(4) CH_D(5) CH_D(6) CH_D(7)
            if (n >= 12) {
                CH_D(8) CH_D(9) CH_D(10) CH_D(11)
                if (n >= 16) {
                    CH_D(12) CH_D(13) CH_D(14) CH_D(15)
                } else {
                    CH_TAIL(12, 13, 14)
                }
            } else {
                CH_TAIL(8, 9, 10)
            }
        } else {
            CH_TAIL(4, 5, 6)
        }
    } else if (n > 0) {
        CH_D0
        CH_TAIL(1, 2, 3)
    }
#undef CH_TAIL
#undef CH_D0
#undef CH_D
    return acc;
}

// One sweep by the whole workgroup: waves 0..CH_R-1 walk the chain as a ring, the other waves stage.  All waves must call it.
//   INIT_OWN: the accumulator starts at the step's own value (scatter-form loops of the reference), else at 0
//   SUB:      terms are subtracted, else added
//   f(k, has_entries, acc, own, diag) -> the step's result, stored to out[w] and the window; f may store more, but it is
//   called by whichever ring wave has the step: it must not carry state from step to step
// The helpers add the leading terms whose producers are at least CH_FAR steps back (ch_stage_block).
// On return every store of the sweep has completed and the workgroup is synchronised; false: abandoned (defect).
template <bool INIT_OWN, bool SUB, class A, class F>
__device__ __forceinline__ bool chain_sweep(const A &ad, ChainLds *L, int k0, int dir, int nsteps, gdouble_p out, F f)
{
    static_assert(CH_R >= 1 && CH_R <= CH_SB && CH_TG >= 2 * CH_R, "ring size");
    const int w = wave_id(), nw = num_waves(), lane = lane_id();
    const int nblk = (nsteps + CH_SB - 1) / CH_SB;
    if (threadIdx.x < CH_NB) ch_set(&L->blk_ready[threadIdx.x], 0);
    if (threadIdx.x < CH_HT) ch_set(&L->eb_tag[threadIdx.x], -1);
    if (threadIdx.x < CH_TG) ch_set(&L->tag[threadIdx.x], 0);
    if (threadIdx.x < CH_R) {
        ch_set(&L->ring_done[threadIdx.x], 0);
        ch_set(&L->ring_eb[threadIdx.x], 0);
    }
    if (threadIdx.x == 0) ch_set(&L->abort, 0);
    __syncthreads();
    if (w >= CH_R) {
        for (int b = w - CH_R; b < nblk && !ch_flag(&L->abort); b += nw - CH_R) ch_stage_block<INIT_OWN, SUB>(ad, L, b, k0, dir, nsteps, out);
    } else {
#ifdef BLU_PROFILE
        long long t_wait = 0, t_tag = 0, t_drain = 0;
        const long long t_begin = (long long)__builtin_amdgcn_s_memtime();
#endif
        const int last = nsteps - 1;
        const int li = lane & 15;
        __builtin_amdgcn_s_setprio(3); // (a ring wave shares its SIMD with helpers: the chain goes first)
        // The records of a block are read once by every ring wave, lane t = step bs + t, and a step takes its fields by
        // v_readlane -- a handful of scalar moves instead of LDS reads and address arithmetic per step.
        const auto rl_d = [](double x, int t) {
            const int lo = __builtin_amdgcn_readlane(__double2loint(x), t), hi = __builtin_amdgcn_readlane(__double2hiint(x), t);
            return __hiloint2double(hi, lo);
        };
        // n entries from entry-ring position eb: lane l has entry l; up to 16 entries: every row of 16 lanes has them all
        // (ch_accumulate_rows).  A lane without an entry reads as a far operand with value 0.
        const auto read_ops = [&](int eb, int n) {
            ChOps E;
            E.val = 0.0;
            E.xv = 0.0;
            E.sel = CH_SEL_FAR;
            const int l = n <= 16 ? li : lane;
            if (l < n) {
                const int r = (eb + l) & (CH_CE - 1);
                const ChOpsV v = L->ev[r];
                E.val = v.val;
                E.xv = v.xv;
                E.sel = L->sel[r];
            }
            return E;
        };
        int cur_b = -1;
        ChRec BR;
        BR.n = BR.eb = BR.w = BR.k = 0;
        BR.diag = BR.own = BR.init = 0.0;
        bool gave_up = false;
        for (int s = w; s < nsteps && !gave_up; s += CH_R) {
            const int b = s / CH_SB;
            if (b != cur_b) {
                // the wave leaves a block: its stores drained, then its progress
                if (cur_b >= 0) {
#ifdef BLU_PROFILE
                    const long long td0 = (long long)__builtin_amdgcn_s_memtime();
#endif
                    ch_vm_drain();
#ifdef BLU_PROFILE
                    t_drain += (long long)__builtin_amdgcn_s_memtime() - td0;
#endif
                    ch_lds_fence();
                    if (lane == 0) ch_set(&L->ring_done[w], b);
                }
#ifdef BLU_PROFILE
                const long long tw0 = (long long)__builtin_amdgcn_s_memtime();
#endif
                CH_WAIT_SPIN(L, ch_flag(&L->blk_ready[b & (CH_NB - 1)]) == b + 1, 3, 0, gave_up);
                asm volatile("" ::: "memory");
#ifdef BLU_PROFILE
                t_wait += (long long)__builtin_amdgcn_s_memtime() - tw0;
#endif
                if (gave_up) break; // (the records are not there: nothing of this block may be used)
                const int sl = b * CH_SB + lane;
                BR = ch_read_rec(L, sl < last ? sl : last);
                if (lane == 0) ch_set(&L->ring_eb[w], BR.eb);
                cur_b = b;
            }
            const int t = s - b * CH_SB;
            const int nf = __builtin_amdgcn_readlane(BR.n, t), eb1 = __builtin_amdgcn_readlane(BR.eb, t);
            const int k1 = __builtin_amdgcn_readlane(BR.k, t), w1 = __builtin_amdgcn_readlane(BR.w, t);
            const double own1 = rl_d(BR.own, t), diag1 = rl_d(BR.diag, t);
            const int n1 = nf < 0 ? -1 : (nf & (CH_HAS - 1));
            double acc = rl_d(BR.init, t);
            // the tag of step s - 1: every result up to it is in the window
            const auto wait_prev = [&]() {
                if (s > 0) {
#ifdef BLU_PROFILE
                    const long long tw0 = (long long)__builtin_amdgcn_s_memtime();
#endif
                    CH_WAIT_SPIN(L, ch_flag(&L->tag[(s - 1) & (CH_TG - 1)]) == s, 4, CH_SPIN, gave_up);
#ifdef BLU_PROFILE
                    t_tag += (long long)__builtin_amdgcn_s_memtime() - tw0;
#endif
                }
                asm volatile("" ::: "memory");
            };
            // window slot of an operand and how many steps back its producer is (a far operand has neither)
            const auto slot_of = [&](int sel) { return (sel == CH_SEL_PREV ? k1 - dir : sel) & (CH_W - 1); };
            const auto dist_of = [&](int slot) { return ((k1 - slot) * dir) & (CH_W - 1); };
            if (n1 > 0 && n1 <= 16) {
                // EARLY: the leading terms up to the first one whose producer is less than CH_R steps back
                const ChOps E = read_ops(eb1, n1);
                const int slot = slot_of(E.sel);
                const bool win = E.sel != CH_SEL_FAR;
                const bool late = win && dist_of(slot) < CH_R;
                const unsigned lm = (unsigned)__ballot(late) & 0xffffu;
                const int p = lm ? __ffs((int)lm) - 1 : n1;
                if (p > 0) {
                    const double x = (win && !late) ? L->xwin[slot] : E.xv;
                    acc = ch_accumulate_rows<SUB>(acc, li < p ? __dmul_rn(x, E.val) : 0.0, p);
                }
                if (p < n1) {
                    // the terms from there on, moved down to lane 0: what is old enough is read and multiplied now ...
                    const int nl = n1 - p;
                    const ChOps EL = read_ops(eb1 + p, nl);
                    const int slot_l = slot_of(EL.sel);
                    const bool win_l = EL.sel != CH_SEL_FAR;
                    const bool late_l = win_l && dist_of(slot_l) < CH_R;
                    const double prod_e = __dmul_rn((win_l && !late_l) ? L->xwin[slot_l] : EL.xv, EL.val);
                    wait_prev();
                    // ... LATE: the window for the late entries, all lanes at once, and the rest of the sum in order
                    const double prod_l = __dmul_rn(L->xwin[slot_l], EL.val);
                    acc = ch_accumulate_rows<SUB>(acc, li < nl ? (late_l ? prod_l : prod_e) : 0.0, nl);
                } else {
                    wait_prev();
                }
            } else if (n1 > 16) { // rare: the whole sum after the wait
                const ChOps E = read_ops(eb1, n1);
                wait_prev();
                const double x = E.sel != CH_SEL_FAR ? L->xwin[slot_of(E.sel)] : E.xv;
                acc = ch_accumulate<SUB>(acc, lane < n1 ? __dmul_rn(x, E.val) : 0.0, n1);
            } else if (n1 < 0) { // long step: straight from global memory; recent producers from the window
                wait_prev();
                const ChMeta M = ad.meta(k1);
                for (int o = 0; o < M.len; o += 64) {
                    ChEnt E;
                    E.pos = k1 - dir * CH_FAR;
                    E.gidx = 0;
                    E.val = 0.0;
                    const int nn = M.len - o < 64 ? M.len - o : 64;
                    double x = 0.0;
                    if (lane < nn) {
                        E = ad.ent(k1, M.b, o + lane);
                        const int d = (k1 - E.pos) * dir;
                        x = (d > 0 && d < CH_FAR) ? L->xwin[E.pos & (CH_W - 1)] : ch_load_final(out + E.gidx);
                    }
                    acc = ch_accumulate<SUB>(acc, lane < nn ? __dmul_rn(x, E.val) : 0.0, nn);
                }
            } else {
                wait_prev();
            }
            if (gave_up) break; // (nothing is published: the others run into their own bounds or see L->abort)
            const double v = f(k1, nf != 0, acc, own1, diag1);
            if (lane == 0) {
                L->xwin[k1 & (CH_W - 1)] = v;
                ch_lds_fence();
                ch_set(&L->tag[s & (CH_TG - 1)], s + 1);
                out[w1] = v;
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // the wave is through: its stores drained, and no helper waits for it any more
        ch_vm_drain();
        ch_lds_fence();
        if (lane == 0) {
            ch_set(&L->ring_eb[w], 0x7fffffff);
            ch_set(&L->ring_done[w], nblk + CH_NB);
        }
#ifdef BLU_PROFILE
        if (lane == 0 && nsteps > 0)
            printf("chain sweep (block %d, ring wave %d of %d): %d steps, %.0f cycles/step of the sweep, waiting for blocks %.0f, for the predecessor %.0f, draining stores %.0f\n",
                   (int)blockIdx.x, w, CH_R, nsteps, (double)((long long)__builtin_amdgcn_s_memtime() - t_begin) / nsteps, (double)t_wait / nsteps,
                   (double)t_tag / nsteps, (double)t_drain / nsteps);
#endif
    }
    __syncthreads();
    return ch_flag(&L->abort) == 0; // (the code of the wait that gave up stays in L->abort for the caller's error line)
}

// sum of |v[k0 + dir * s]| for s = 0 .. n-1, added to 0.0 in that order with one rounding per term -- what a step function
// that accumulated `x1 += fabs(result)` from step to step would have got -- and their maximum.  One wave; the values are
// final (the sweep that wrote them has returned).  64 values per load, four loads ahead of the sum; the sum itself is one
// v_fmac_f64 per term (ch_accumulate_rows).
__device__ __forceinline__ double ch_abs_sum_ordered(gdouble_p v, int k0, int dir, int n, double *vmax)
{
    const int lane = lane_id();
    const auto ld = [&](int s0) {
        const int s = s0 + lane;
        return s < n ? fabs(ch_load_final(v + (k0 + dir * s))) : 0.0;
    };
    double acc = 0.0, mx = 0.0;
    double a0 = ld(0), a1 = ld(64), a2 = ld(128), a3 = ld(192);
    for (int s0 = 0; s0 < n; s0 += 64) {
        const double cur = a0;
        a0 = a1;
        a1 = a2;
        a2 = a3;
        a3 = ld(s0 + 256);
        mx = fmax(mx, cur);
        const int nn = n - s0 < 64 ? n - s0 : 64;
        for (int c = 0; c < nn; c += 16) {
            const double rowv = __shfl(cur, c + (lane & 15));
            acc = ch_accumulate_rows<false>(acc, rowv, nn - c < 16 ? nn - c : 16);
        }
    }
    *vmax = wave_max_d(mx);
    return acc;
}
