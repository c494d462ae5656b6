// The row x channel sweep skeleton of bn.hip (BatchNorm statistics, affine / activation passes and their backward) - shared with se.hip,
// whose gate sweeps leave BatchNorm-backward reduce rows in the SAME geometry and summation order as sgx_bn_bwd_reduce.
#pragma once
#include "sgx_common.h"

#define SW_THREADS 256
#define SW_MAXCG 64  // float4 channel groups per workgroup strip (256 channels)
// every sweep moves float4 (sgx_ld4 / sgx_st4): the addresses of its tensors, per-channel rows and partial rows (NULL passes: an absent
// operand) and its row strides must be multiples of 16 bytes (include/sgx_hip.h, conventions) - checked by the entry points, before any launch
#define SW_ALIGNED(p) (((uintptr_t)(p) % 16) == 0)
#define SW_LD4(ld) ((ld) % 4 == 0)
// (the channel count first: the per-channel rows of one operand sit C floats apart)
#define SW_CHECK_VEC(C, cond, what)                                                                   \
    do {                                                                                              \
        SGX_CHECK_ARG((C) > 0 && (C) % 4 == 0, "%s: need M>0 and C%%4==0 (C=%d)", what, (int)(C));    \
        SGX_CHECK_ARG(cond, "%s: strides and addresses must be multiples of 16 bytes", what);         \
    } while (0)

struct SweepGeom {
    long M;
    int C, C4, CG, RL, nblk, rows_per_blk, ctiles;
};

// nblk: the number of row blocks (0: sgx_stats_blocks(M)) - what a sweep stores does not depend on it, the count of its partial rows does
static SweepGeom sweep_geom(long M, int C, int nblk = 0) {
    SweepGeom g;
    g.M = M;
    g.C = C;
    g.C4 = C / 4;
    g.CG = g.C4 < SW_MAXCG ? g.C4 : SW_MAXCG;
    g.RL = SW_THREADS / g.CG;
    g.nblk = nblk > 0 ? nblk : sgx_stats_blocks(M);
    g.rows_per_blk = (int)((M + g.nblk - 1) / g.nblk);
    g.ctiles = (g.C4 + g.CG - 1) / g.CG;
    return g;
}

// F: struct with  In load(long r, int c)  (all global loads of row r, channels c..c+3),  Cst consts(int c)  (the per-channel
// constants of the lane's four channels - scale / shift / coefficient rows - loaded ONCE, ahead of the row loop) and
// void apply(long r, int c, const In&, const Cst&, float4 (&q)[max(NQ, 1)])  (the arithmetic, the stores and NQ per-channel
// accumulations).  (Round 5: the constants used to be re-read inside apply for every row - the compiler cannot hoist them past the
// row's stores, which may alias them for all it knows: 7 of the 9 load instructions per row of the BatchNorm-backward apply, 14 of 17
// of the QARepVGG one, all L1 hits but each a trip through the texture path, which at 64 B/clk/CU was busier with them than with the
// data.)  The split lets the sweep issue the loads of ROWS rows before the first store: with one row in flight
// per lane these streaming kernels sat at ~40 % of the HBM rate (r1b profile) - latency-bound, not bandwidth-bound.  ROWS is 4 for the
// sweeps over one or two tensors and 2 for those that read three or carry many constants (the registers of a row in flight).
// In-place use (output aliasing an input) stays correct: a row is completely read before it is written, rows are disjoint.
// partials (NQ > 0; may be NULL: no reduction): [NQ][nblk][C], plane k = the lane sums of q[k] (fp32), met in ascending row-lane order in
// fp64 and rounded once.  NQ == 0 reserves no LDS.
template <typename F, int NQ, int ROWS>
__global__ __launch_bounds__(SW_THREADS) void sweep_kernel(F f, SweepGeom g, float* partials) {
    const int tid = threadIdx.x;
    const int cg = tid % g.CG, rl = tid / g.CG;
    const int c4 = blockIdx.y * g.CG + cg;
    const bool live = (rl < g.RL) && (c4 < g.C4);
    const int c = c4 * 4;
    float4 q[NQ > 0 ? NQ : 1];
#pragma unroll
    for (int k = 0; k < (NQ > 0 ? NQ : 1); ++k) q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        long r0 = (long)blockIdx.x * g.rows_per_blk;
        long r1 = r0 + g.rows_per_blk;
        if (r1 > g.M) r1 = g.M;
        long r = r0 + rl;
        const long st = g.RL;
        const typename F::Cst k = f.consts(c);
        for (; r + (ROWS - 1) * st < r1; r += ROWS * st) {
            typename F::In in[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) in[u] = f.load(r + u * st, c);
#pragma unroll
            for (int u = 0; u < ROWS; ++u) f.apply(r + u * st, c, in[u], k, q);
        }
        for (; r < r1; r += st) {
            typename F::In i0 = f.load(r, c);
            f.apply(r, c, i0, k, q);
        }
    }
    if constexpr (NQ > 0) {
        if (!partials) return;  // uniform across the workgroup
        __shared__ float4 red[NQ][SW_THREADS];
#pragma unroll
        for (int k = 0; k < NQ; ++k) red[k][tid] = q[k];
        __syncthreads();
        if (live && rl == 0) {
            // the lane sums meet in double: the partial row carries ONE fp32 rounding (random sign), not a chain of them - the per-channel
            // means the finalize kernels form from these rows (mean of g in the BatchNorm backward above all) are then good to ~1e-9 relative
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                double t[4] = {0.0, 0.0, 0.0, 0.0};
                for (int j = 0; j < g.RL; ++j) {
                    const float4 a = red[k][j * g.CG + cg];
                    t[0] += a.x; t[1] += a.y; t[2] += a.z; t[3] += a.w;
                }
                sgx_st4(partials + ((long)k * g.nblk + blockIdx.x) * g.C + c, make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]));
            }
        }
    }
}

template <typename F, int NQ, int ROWS>
static int32_t run_sweep(const F& f, long M, int C, float* partials, void* stream, const char* what, int nblk = 0) {
    SGX_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0, "%s: need M>0 and C%%4==0 (C=%d)", what, C);
    SGX_CHECK_ARG(nblk >= 0 && nblk <= M, "%s: row blocks %d outside 0..M", what, nblk);
    SweepGeom g = sweep_geom(M, C, nblk);
    SGX_LAUNCH((sweep_kernel<F, NQ, ROWS>), dim3(g.nblk, g.ctiles), dim3(SW_THREADS), 0, stream, f, g, partials);
    SGX_CHECK_LAUNCH(what);
    return SGX_OK;
}
