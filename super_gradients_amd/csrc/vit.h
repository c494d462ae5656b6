// The Vision Transformer's glue kernels (classification_models/vit.py): softmax attention forward / backward, LayerNorm over the channel
// axis, exact-erf GELU, the patch-row gather and the token assembly.  Included by se.hip (the sweep skeleton is there already); the token-wise
// linear layers - more than 95 % of the model's arithmetic - are 1x1 convolutions and run in conv.hip.
// Data layout: tokens are pixels.  A [B, T, D] sequence is the NHWC map [B, T, 1, D]; every operand is a view with contiguous channels,
// explicit pixel / image strides, float4 channel groups and 16-byte aligned addresses (anything else: SGX_ERR_BAD_ARG, nothing launched).
// Every reduction has a fixed order: no floating-point atomics, nothing that depends on which workgroup finishes first.
#pragma once
#include "sgx_common.h"
#include "sgx_sweep.h"

#define VIT_ALIGNED(p) (((uintptr_t)(p) % 16) == 0)
#define VIT_LD4(ld) ((ld) % 4 == 0)

// ---------------------------------------------------------------------------------------------
// GELU, the exact form (nn.GELU()'s default): y = h * Phi(h), dy/dh = Phi(h) + h * phi(h).  Two sweeps on the bn.hip skeleton.
__device__ __forceinline__ float vit_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float vit_gelu_grad(float v) {
    const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * expf(-0.5f * v * v);
    return cdf + v * pdf;
}
struct GeluFwdF {
    const float* x; long x_ld; float* y; long y_ld;
    struct In { float4 v; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(x + r * x_ld + c)}; }
    struct Cst {};
    __device__ Cst consts(int) const { return Cst{}; }
    __device__ void apply(long r, int c, const In& in, const Cst&, float4 (&)[1]) const {
        const float4 v = in.v;
        sgx_st4(y + r * y_ld + c, make_float4(vit_gelu(v.x), vit_gelu(v.y), vit_gelu(v.z), vit_gelu(v.w)));
    }
};
struct GeluBwdF {
    const float* dy; long dy_ld; const float* x; long x_ld; float* dx; long dx_ld;
    struct In { float4 d, v; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(dy + r * dy_ld + c), sgx_ld4(x + r * x_ld + c)}; }
    struct Cst {};
    __device__ Cst consts(int) const { return Cst{}; }
    __device__ void apply(long r, int c, const In& in, const Cst&, float4 (&)[1]) const {
        const float4 d = in.d, v = in.v;
        sgx_st4(dx + r * dx_ld + c, make_float4(d.x * vit_gelu_grad(v.x), d.y * vit_gelu_grad(v.y), d.z * vit_gelu_grad(v.z), d.w * vit_gelu_grad(v.w)));
    }
};
extern "C" int32_t sgx_gelu_fwd(const float* x, int64_t x_ld, float* y, int64_t y_ld, int64_t M, int32_t C, void* stream) {
    SGX_CHECK_ARG(x && y, "gelu_fwd: null pointer");
    SGX_CHECK_ARG(VIT_LD4(x_ld) && VIT_LD4(y_ld) && VIT_ALIGNED(x) && VIT_ALIGNED(y), "gelu_fwd: strides and addresses must be multiples of 16 bytes");
    GeluFwdF f{x, (long)x_ld, y, (long)y_ld};
    return run_sweep<GeluFwdF, 0, 4>(f, M, C, nullptr, stream, "gelu_fwd");
}
extern "C" int32_t sgx_gelu_bwd(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dx, int64_t dx_ld, int64_t M, int32_t C,
                                void* stream) {
    SGX_CHECK_ARG(dy && x && dx, "gelu_bwd: null pointer");
    SGX_CHECK_ARG(VIT_LD4(dy_ld) && VIT_LD4(x_ld) && VIT_LD4(dx_ld) && VIT_ALIGNED(dy) && VIT_ALIGNED(x) && VIT_ALIGNED(dx),
                  "gelu_bwd: strides and addresses must be multiples of 16 bytes");
    GeluBwdF f{dy, (long)dy_ld, x, (long)x_ld, dx, (long)dx_ld};
    return run_sweep<GeluBwdF, 0, 4>(f, M, C, nullptr, stream, "gelu_bwd");
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over the channel axis (biased variance).  One wave per row: a lane holds up to G float4 groups of the row in registers, the
// mean and the centred sum of squares are two butterfly reductions over values that are already on chip (two-pass arithmetic, one pass
// over HBM).  The row count per workgroup is LN_WAVES.
#define LN_THREADS 256
#define LN_WAVES 4
#define LN_MAXG 8             // float4 groups per lane: C <= 64 * 4 * 8 = 2048
#define LN_BWD_BLOCK_ROWS 64  // rows per partial row of dgamma / dbeta

__device__ __forceinline__ float vit_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int G>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(long M, int C, const float* x, long x_ld, const float* gamma, const float* beta, float eps,
                                                            float* y, long y_ld, float* mean, float* rstd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * LN_WAVES + wave;
    if (r >= M) return;  // the whole wave leaves together
    const int C4 = C >> 2;
    float4 v[G];
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c4 = lane + 64 * g;
        v[g] = c4 < C4 ? sgx_ld4(x + r * x_ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[g].x + v[g].y) + (v[g].z + v[g].w);
    }
    const float mu = vit_wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (lane + 64 * g < C4) {
            const float a = v[g].x - mu, b = v[g].y - mu, c = v[g].z - mu, d = v[g].w - mu;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    const float rs = 1.f / sqrtf(vit_wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c4 = lane + 64 * g;
        if (c4 < C4) {
            const float4 w = sgx_ld4(gamma + 4 * c4), b = sgx_ld4(beta + 4 * c4);
            sgx_st4(y + r * y_ld + 4 * c4, make_float4((v[g].x - mu) * rs * w.x + b.x, (v[g].y - mu) * rs * w.y + b.y, (v[g].z - mu) * rs * w.z + b.z,
                                                       (v[g].w - mu) * rs * w.w + b.w));
        }
    }
    if (lane == 0) {
        if (mean) mean[r] = mu;
        if (rstd) rstd[r] = rs;
    }
}

// dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) [+ addend], g = dy * gamma, xhat = (x - mean) * rstd.  dx may alias dy or addend: a
// lane reads its elements of the row before it writes them.
template <int G>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_dx_kernel(long M, int C, const float* dy, long dy_ld, const float* x, long x_ld, const float* gamma,
                                                               const float* mean, const float* rstd, const float* addend, long a_ld, float* dx,
                                                               long dx_ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * LN_WAVES + wave;
    if (r >= M) return;
    const int C4 = C >> 2;
    const float mu = mean[r], rs = rstd[r];
    float4 gg[G], xh[G];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c4 = lane + 64 * g;
        gg[g] = xh[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < C4) {
            const float4 d = sgx_ld4(dy + r * dy_ld + 4 * c4), v = sgx_ld4(x + r * x_ld + 4 * c4), w = sgx_ld4(gamma + 4 * c4);
            gg[g] = make_float4(d.x * w.x, d.y * w.y, d.z * w.z, d.w * w.w);
            xh[g] = make_float4((v.x - mu) * rs, (v.y - mu) * rs, (v.z - mu) * rs, (v.w - mu) * rs);
            s1 += (gg[g].x + gg[g].y) + (gg[g].z + gg[g].w);
            s2 += (gg[g].x * xh[g].x + gg[g].y * xh[g].y) + (gg[g].z * xh[g].z + gg[g].w * xh[g].w);
        }
    }
    const float m1 = vit_wave_sum(s1) / (float)C, m2 = vit_wave_sum(s2) / (float)C;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c4 = lane + 64 * g;
        if (c4 < C4) {
            float4 o = make_float4(rs * (gg[g].x - m1 - xh[g].x * m2), rs * (gg[g].y - m1 - xh[g].y * m2), rs * (gg[g].z - m1 - xh[g].z * m2),
                                   rs * (gg[g].w - m1 - xh[g].w * m2));
            if (addend) {
                const float4 a = sgx_ld4(addend + r * a_ld + 4 * c4);
                o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
            }
            sgx_st4(dx + r * dx_ld + 4 * c4, o);
        }
    }
}

// dgamma / dbeta: a sweep leaves [2][nblk][C] partial rows (sum dy * xhat, sum dy) of LN_BWD_BLOCK_ROWS rows each - lane sums met in fp64
// in ascending lane order (sgx_sweep.h) - and the finalize adds them in block order, in fp64, onto the gradient-arena views.
struct LnBwdParamF {
    const float* dy; long dy_ld; const float* x; long x_ld; const float* mean; const float* rstd;
    struct In { float4 d, v; float mu, rs; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(dy + r * dy_ld + c), sgx_ld4(x + r * x_ld + c), mean[r], rstd[r]}; }
    struct Cst {};
    __device__ Cst consts(int) const { return Cst{}; }
    __device__ void apply(long, int, const In& in, const Cst&, float4 (&q)[2]) const {
        const float4 d = in.d, v = in.v;
        q[0].x += d.x * ((v.x - in.mu) * in.rs); q[0].y += d.y * ((v.y - in.mu) * in.rs);
        q[0].z += d.z * ((v.z - in.mu) * in.rs); q[0].w += d.w * ((v.w - in.mu) * in.rs);
        q[1].x += d.x; q[1].y += d.y; q[1].z += d.z; q[1].w += d.w;
    }
};
__global__ void ln_bwd_param_finalize_kernel(int nblk, int C, const float* partials, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < nblk; ++k) {
        a += (double)partials[(long)k * C + c];
        b += (double)partials[((long)nblk + k) * C + c];
    }
    dgamma[c] += (float)a;
    dbeta[c] += (float)b;
}

#define LN_DISPATCH(kernel, ...)                                                                                          \
    do {                                                                                                                  \
        const int groups__ = sgx_cdiv(C / 4, 64);                                                                         \
        const dim3 grid__((unsigned)((M + LN_WAVES - 1) / LN_WAVES)), block__(LN_THREADS);                                \
        if (groups__ <= 1) SGX_LAUNCH((kernel<1>), grid__, block__, 0, stream, __VA_ARGS__);                              \
        else if (groups__ <= 2) SGX_LAUNCH((kernel<2>), grid__, block__, 0, stream, __VA_ARGS__);                         \
        else if (groups__ <= 4) SGX_LAUNCH((kernel<4>), grid__, block__, 0, stream, __VA_ARGS__);                         \
        else SGX_LAUNCH((kernel<LN_MAXG>), grid__, block__, 0, stream, __VA_ARGS__);                                      \
    } while (0)
#define LN_CHECK_DIMS(what)                                                                                                              \
    SGX_CHECK_ARG(M > 0 && M < 0x7fffffffL * LN_WAVES && C >= 4 && C % 4 == 0 && C <= 256 * LN_MAXG, "%s: need M > 0, C %% 4 == 0 and 4 <= C <= %d (M=%ld C=%d)", \
                  what, 256 * LN_MAXG, (long)M, C)

extern "C" int32_t sgx_layernorm_fwd(const float* x, int64_t x_ld, const float* gamma, const float* beta, float eps, float* y, int64_t y_ld, float* mean,
                                     float* rstd, int64_t M, int32_t C, void* stream) {
    SGX_CHECK_ARG(x && gamma && beta && y, "layernorm_fwd: null pointer");
    LN_CHECK_DIMS("layernorm_fwd");
    SGX_CHECK_ARG(VIT_LD4(x_ld) && VIT_LD4(y_ld) && VIT_ALIGNED(x) && VIT_ALIGNED(y) && VIT_ALIGNED(gamma) && VIT_ALIGNED(beta),
                  "layernorm_fwd: strides and addresses must be multiples of 16 bytes");
    LN_DISPATCH(ln_fwd_kernel, (long)M, C, x, (long)x_ld, gamma, beta, eps, y, (long)y_ld, mean, rstd);
    SGX_CHECK_LAUNCH("layernorm_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_layernorm_bwd_block_rows(void) { return LN_BWD_BLOCK_ROWS; }
extern "C" int64_t sgx_layernorm_bwd_workspace(int64_t M, int32_t C) {
    return 2 * ((M + LN_BWD_BLOCK_ROWS - 1) / LN_BWD_BLOCK_ROWS) * (int64_t)C * (int64_t)sizeof(float) + 256;
}
extern "C" int32_t sgx_layernorm_bwd(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* gamma, const float* mean, const float* rstd,
                                     const float* addend, int64_t addend_ld, float* dx, int64_t dx_ld, float* dgamma, float* dbeta, int64_t M, int32_t C,
                                     void* ws, int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(dy && x && gamma && mean && rstd && dx, "layernorm_bwd: null pointer");
    SGX_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "layernorm_bwd: dgamma and dbeta come together");
    LN_CHECK_DIMS("layernorm_bwd");
    SGX_CHECK_ARG(VIT_LD4(dy_ld) && VIT_LD4(x_ld) && VIT_LD4(dx_ld) && VIT_LD4(addend_ld) && VIT_ALIGNED(dy) && VIT_ALIGNED(x) && VIT_ALIGNED(dx) &&
                      VIT_ALIGNED(addend) && VIT_ALIGNED(gamma) && VIT_ALIGNED(dgamma) && VIT_ALIGNED(dbeta) && VIT_ALIGNED(ws),
                  "layernorm_bwd: strides and addresses must be multiples of 16 bytes");
    if (dgamma) {  // first: dx may alias dy
        SGX_CHECK_ARG(ws && ws_bytes >= sgx_layernorm_bwd_workspace(M, C), "layernorm_bwd: workspace too small");
        const int nblk = (int)((M + LN_BWD_BLOCK_ROWS - 1) / LN_BWD_BLOCK_ROWS);
        LnBwdParamF f{dy, (long)dy_ld, x, (long)x_ld, mean, rstd};
        const int32_t rc = run_sweep<LnBwdParamF, 2, 2>(f, M, C, (float*)ws, stream, "layernorm_bwd (dgamma / dbeta)", nblk);
        if (rc != SGX_OK) return rc;
        SGX_LAUNCH(ln_bwd_param_finalize_kernel, dim3(sgx_cdiv(C, 256)), dim3(256), 0, stream, nblk, C, (const float*)ws, dgamma, dbeta);
        SGX_CHECK_LAUNCH("layernorm_bwd (finalize)");
    }
    LN_DISPATCH(ln_bwd_dx_kernel, (long)M, C, dy, (long)dy_ld, x, (long)x_ld, gamma, mean, rstd, addend, (long)addend_ld, dx, (long)dx_ld);
    SGX_CHECK_LAUNCH("layernorm_bwd");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// Softmax attention per (image, head): o = softmax(scale * q k^T) v.  q, k, v are channel slices of one [B, T, 1, 3D] map (head h at channels
// [h d, (h + 1) d) of each slice; the three pointers share their strides), o a [B, T, 1, D] map written in the same head order: no permute, no
// copy.  The T x T probabilities exist only as 16 x 16 tiles in registers and LDS.
//   forward    one workgroup per (64 query rows, head, image), one wave per 16 of them; key / value rows stream through LDS 32 at a time;
//              running row maximum m and sum l (the maximum is subtracted before every exp); lse = m + log l saved per row.
//   backward   recomputes p = exp(scale * s - lse).  Pass 1 (owned by query rows): Delta_i = sum_c dO_ic O_ic (left in the workspace) and
//              dq = scale * sum_j ds_ij k_j, ds = p (dO v^T - Delta).  Pass 2 (owned by key rows): dv = sum_i p_ij dO_i,
//              dk = scale * sum_i ds_ij q_i.  Every output element has one owner that adds in ascending row order: same inputs, same bits.
// Arithmetic: v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation - exact fp32 FMAs).  A wave keeps its own 16 rows as A fragments
// in registers (lane l: row l & 15, channels 4 s + (l >> 4)), forms a 16 x 16 score tile against 16 streamed rows read from LDS as B fragments
// (accumulator register r of lane l: row 4 (l >> 4) + r, column l & 15 - row reductions are butterflies over the 16 lanes of a quarter
// wave), turns the tile into an A fragment through a 1 KB LDS patch of its own (wave-level ordering, no workgroup barrier) and multiplies it
// with the streamed rows once more, 16 channels per accumulator (NB = 4 or 8 of them: d <= 64 / d <= 128; LDS rows are zero-filled to a
// multiple of 16 channels).
#define ATT_TQ 64  // own rows per workgroup (four waves of 16): query rows in the forward and the dq pass, key rows in the dk / dv pass
#define ATT_TK 32  // streamed rows staged in LDS between two workgroup barriers: two sub-tiles of 16
#define ATT_THREADS 256
#define ATT_MAXD 128
#define ATT_NEG_INF (-__builtin_huge_valf())

__device__ __forceinline__ sgx_f32x4 att_mfma(float a, float b, sgx_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// rows t0 .. t0 + ATT_TK - 1 of a strided [T][d] slice -> LDS rows of dp floats, zeros past T and from d up to the 16-channel boundary
__device__ __forceinline__ void att_stage(float* dst, const float* src, long ld_pix, int t0, int T, int d, int dp) {
    const int g4 = (dp - 4) >> 2;
    for (int i = threadIdx.x; i < ATT_TK * g4; i += ATT_THREADS) {
        const int r = i / g4, c = (i - r * g4) * 4;
        const int t = t0 + r;
        sgx_st4(dst + r * dp + c, (t < T && c < d) ? sgx_ld4(src + (long)t * ld_pix + c) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}
// the wave's own rows t0 .. t0 + 15 as A fragments (zeros past T and past d)
template <int NB>
__device__ __forceinline__ void att_load_frag(float (&f)[4 * NB], const float* src, long ld_pix, int t0, int T, int d, int lane) {
    const int t = t0 + (lane & 15);
    const float* p = src + (long)t * ld_pix + (lane >> 4);
#pragma unroll
    for (int s = 0; s < 4 * NB; ++s) f[s] = (t < T && 4 * s < d) ? p[4 * s] : 0.f;
}
// 16 x 16 tile = (own rows) x (16 LDS rows)^T over d channels
template <int NB>
__device__ __forceinline__ sgx_f32x4 att_nt(const float (&a)[4 * NB], const float* brows, int dp, int d, int lane) {
    sgx_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* b = brows + (lane & 15) * dp + (lane >> 4);
#pragma unroll
    for (int s = 0; s < 4 * NB; ++s)
        if (4 * s < d) acc = att_mfma(a[s], b[4 * s], acc);
    return acc;
}
// a tile in accumulator layout -> the wave's LDS patch [16][16] (row-major)
__device__ __forceinline__ void att_put_tile(float* patch, const float (&v)[4], int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) patch[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = v[r];
}
// acc[nb] += patch (16 x 16) x (16 LDS rows), 16 channels per accumulator
template <int NB>
__device__ __forceinline__ void att_nn(sgx_f32x4 (&acc)[NB], const float* patch, const float* brows, int dp, int d, int lane) {
    float a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = patch[(lane & 15) * 16 + 4 * s + (lane >> 4)];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        if (16 * nb < d) {
            const float* b = brows + (lane >> 4) * dp + 16 * nb + (lane & 15);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[nb] = att_mfma(a[s], b[4 * s * dp], acc[nb]);
        }
}
__device__ __forceinline__ float att_sum16(float v) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float att_max16(float v) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
// own rows of an accumulator-layout result -> a strided [T][d] slice (scaled)
template <int NB>
__device__ __forceinline__ void att_store(float* dst, long ld_pix, int t0, int T, int d, const sgx_f32x4 (&acc)[NB], const float (&mul)[4], int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + (lane >> 4) * 4 + r;
        if (t < T) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int ch = 16 * nb + (lane & 15);
                if (ch < d) dst[(long)t * ld_pix + ch] = acc[nb][r] * mul[r];
            }
        }
    }
}

// Relative position bias (BEiT): s_ij = scale * q_i k_j + table[index(i, j)][h] over a gh x gw token grid behind one class token
// (T = gh gw + 1).  index(i, j) is computed, never read: N - 1 for i = j = 0, N - 3 for i = 0, N - 2 for j = 0, else
// (y_i - y_j + gh - 1) (2 gw - 1) + (x_i - x_j + gw - 1) = lin(i) - lin(j) + c0 with lin(t) = y_t (2 gw - 1) + x_t, (y, x) = divmod(t - 1, gw),
// N = (2 gh - 1)(2 gw - 1) + 3.  Head h's column of the table is staged in LDS once per workgroup: N <= ATT_RPB_MAXN floats.
#define ATT_RPB_MAXN 4096
#define ATT_RPB_BINS (ATT_RPB_MAXN / ATT_THREADS)  // bins of the table gradient a thread of the dq pass owns: 4 up to N = 1024 (16 x 16 grids), else 16
#define ATT_T2(a, b) a, b
struct AttRpb {
    const float* table;  // [N][ld] (+ h: head h's column)
    long ld;
    int gh, gw, N, c0;  // c0 = (gh - 1) (2 gw - 1) + gw - 1
};
// lin(t) of a token clamped into 1 .. T - 1 (rows and columns past T are masked by their callers; their index must stay inside the table)
__device__ __forceinline__ int rpb_lin(int t, int T, int gw) {
    t = t < T ? t : T - 1;
    t = t > 0 ? t - 1 : 0;
    const int y = t / gw;
    return y * (2 * gw - 1) + (t - y * gw);
}
__device__ __forceinline__ int rpb_index(int i, int j, int li, int lj, const AttRpb& rp) {
    return i == 0 ? (j == 0 ? rp.N - 1 : rp.N - 3) : (j == 0 ? rp.N - 2 : li - lj + rp.c0);
}
__device__ __forceinline__ void rpb_stage(float* Ts, const AttRpb& rp, int h) {
    for (int i = threadIdx.x; i < rp.N; i += ATT_THREADS) Ts[i] = rp.table[(long)i * rp.ld + h];
}

template <int NB, bool BIAS>
__global__ __launch_bounds__(ATT_THREADS) void attn_fwd_kernel(int T, int d, int heads, const float* q, const float* k, const float* v, long ld_pix,
                                                               long ld_img, float scale, float* o, long o_ld_pix, long o_ld_img, float* lse, AttRpb rp) {
    SGX_DYN_SMEM(float, sm);
    const int dp = ((d + 15) & ~15) + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Ks = sm;
    float* Vs = Ks + ATT_TK * dp;
    float* Ps = Vs + ATT_TK * dp + wave * 256;
    const float* Ts = Vs + ATT_TK * dp + 4 * 256;
    const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * ATT_TQ + 16 * wave;
    const long base = (long)b * ld_img + (long)h * d;
    float qf[4 * NB];
    att_load_frag<NB>(qf, q + base, ld_pix, q0, T, d, lane);
    int li[4];  // lin() of the lane's four accumulator rows
    if constexpr (BIAS) {
        rpb_stage(Vs + ATT_TK * dp + 4 * 256, rp, h);  // (visible after the loop's first barrier)
#pragma unroll
        for (int r = 0; r < 4; ++r) li[r] = rpb_lin(q0 + (lane >> 4) * 4 + r, T, rp.gw);
    }
    float m[4], l[4];
    sgx_f32x4 acc[NB];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = ATT_NEG_INF; l[r] = 0.f; }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < T; k0 += ATT_TK) {
        __syncthreads();  // the previous rows' readers are done
        att_stage(Ks, k + base, ld_pix, k0, T, d, dp);
        att_stage(Vs, v + base, ld_pix, k0, T, d, dp);
        __syncthreads();
        for (int u = 0; u < ATT_TK / 16; ++u) {
            const int kk = k0 + 16 * u;
            if (kk >= T) break;  // the same for every thread of the workgroup
            const sgx_f32x4 s = att_nt<NB>(qf, Ks + 16 * u * dp, dp, d, lane);
            const bool valid = kk + (lane & 15) < T;
            float p[4], alpha[4], bias[4];
            if constexpr (BIAS) {
                const int j = kk + (lane & 15), lj = rpb_lin(j, T, rp.gw);
#pragma unroll
                for (int r = 0; r < 4; ++r) bias[r] = Ts[rpb_index(q0 + (lane >> 4) * 4 + r, valid ? j : T - 1, li[r], lj, rp)];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sv = valid ? (BIAS ? fmaf(scale, s[r], bias[r]) : scale * s[r]) : ATT_NEG_INF;
                const float mn = fmaxf(m[r], att_max16(sv));  // finite: key kk is valid
                p[r] = expf(sv - mn);                          // masked keys: exp(-inf) = 0
                alpha[r] = expf(m[r] - mn);
                l[r] = l[r] * alpha[r] + att_sum16(p[r]);
                m[r] = mn;
            }
            sgx_wave_lds_sync();  // the patch's previous readers (this wave) are done
            att_put_tile(Ps, p, lane);
            sgx_wave_lds_sync();
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[nb][r] *= alpha[r];
            att_nn<NB>(acc, Ps, Vs + 16 * u * dp, dp, d, lane);
        }
    }
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        inv[r] = 1.f / l[r];
        const int t = q0 + (lane >> 4) * 4 + r;
        if (t < T && (lane & 15) == 0) lse[((long)b * heads + h) * T + t] = m[r] + logf(l[r]);
    }
    att_store<NB>(o + (long)b * o_ld_img + (long)h * d, o_ld_pix, q0, T, d, acc, inv, lane);
}

// The table gradient inside the dq pass: dtable[r][h] = sum_b sum_{index(i, j) = r} ds_bhij.  The workgroup parks the ds of its 64 rows x the
// staged ATT_TK columns in LDS (Dp, [64][ATT_TK + 1]); thread t owns bins t, t + 256, ... and adds, per staged tile, the elements of its
// bins in ascending row order into registers - a regular bin (dy, dx) meets row i at column j = i - (dy gw + dx) wherever x_i - dx stays
// inside the grid, so a bin walks only the rows whose column is staged: 64 x ATT_TK additions per tile over the whole workgroup.  One
// partial row [N] per (image, row tile, head) goes to the workspace; attn_rpb_dtable_finalize_kernel adds them in (image, tile) order.
template <int BINS>
__device__ __forceinline__ void rpb_gather(float (&bin)[BINS], const float* Dp, int I0, int k0, int T, const AttRpb& rp) {
    const int W = 2 * rp.gw - 1, gw = rp.gw;
    const int jlo = k0 > 1 ? k0 : 1, jhi = k0 + ATT_TK < T ? k0 + ATT_TK : T;  // the staged patch-token columns
    const int ilo = I0 > 1 ? I0 : 1, ihi = I0 + ATT_TQ < T ? I0 + ATT_TQ : T;  // the workgroup's patch-token rows
#pragma unroll
    for (int m = 0; m < BINS; ++m) {
        const int r = (int)threadIdx.x + ATT_THREADS * m;
        if (r >= rp.N) continue;
        float a = bin[m];
        if (r < rp.N - 3) {
            const int by = r / W;
            const int dx = r - by * W - (gw - 1), off = (by - (rp.gh - 1)) * gw + dx;  // i - j of the bin's pairs
            int i = ilo > jlo + off ? ilo : jlo + off;
            const int iend = ihi < jhi + off ? ihi : jhi + off;
            if (i < iend) {
                int xi = (i - 1) % gw;
                const float* p = Dp + (i - I0) * (ATT_TK + 1) + (i - off - k0);  // (the next row's element: one row down, one column on)
                for (; i < iend; ++i, p += ATT_TK + 2) {
                    if ((unsigned)(xi - dx) < (unsigned)gw) a += *p;
                    if (++xi == gw) xi = 0;
                }
            }
        } else if (r == rp.N - 3) {  // the class token's row
            if (I0 == 0)
                for (int j = jlo; j < jhi; ++j) a += Dp[j - k0];
        } else if (r == rp.N - 2) {  // the class token's column
            if (k0 == 0)
                for (int i = ilo; i < ihi; ++i) a += Dp[(i - I0) * (ATT_TK + 1)];
        } else if (I0 == 0 && k0 == 0) {
            a += Dp[0];
        }
        bin[m] = a;
    }
}

template <int NB, bool BIAS, int BINS>
__global__ __launch_bounds__(ATT_THREADS) void attn_bwd_dq_kernel(int T, int d, int heads, const float* q, const float* k, const float* v, long ld_pix,
                                                                  long ld_img, const float* o, const float* dout, long o_ld_pix, long o_ld_img,
                                                                  const float* lse, float scale, float* dq, long g_ld_pix, long g_ld_img,
                                                                  float* delta, AttRpb rp, float* dt_part) {
    SGX_DYN_SMEM(float, sm);
    const int dp = ((d + 15) & ~15) + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Ks = sm;
    float* Vs = Ks + ATT_TK * dp;
    float* Ss = Vs + ATT_TK * dp + wave * 256;
    float* Ts = Vs + ATT_TK * dp + 4 * 256;  // BIAS: head h's table column [N], then Dp [ATT_TQ][ATT_TK + 1]
    float* Dp = Ts + rp.N;
    const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * ATT_TQ + 16 * wave;
    const long base = (long)b * ld_img + (long)h * d, obase = (long)b * o_ld_img + (long)h * d;
    const long sbase = ((long)b * heads + h) * T;
    float qf[4 * NB], df[4 * NB];
    att_load_frag<NB>(qf, q + base, ld_pix, q0, T, d, lane);
    att_load_frag<NB>(df, dout + obase, o_ld_pix, q0, T, d, lane);
    float dl[4], L[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = q0 + (lane >> 4) * 4 + r;
        float part = 0.f;
        if (t < T) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int ch = 16 * nb + (lane & 15);
                if (ch < d) part = fmaf(dout[obase + (long)t * o_ld_pix + ch], o[obase + (long)t * o_ld_pix + ch], part);
            }
        }
        dl[r] = att_sum16(part);
        L[r] = t < T ? lse[sbase + t] : 0.f;
        if (t < T && (lane & 15) == 0) delta[sbase + t] = dl[r];
    }
    int li[4];
    float bin[BINS];
    if constexpr (BIAS) {
        rpb_stage(Ts, rp, h);  // (visible after the loop's first barrier)
#pragma unroll
        for (int r = 0; r < 4; ++r) li[r] = rpb_lin(q0 + (lane >> 4) * 4 + r, T, rp.gw);
#pragma unroll
        for (int m = 0; m < BINS; ++m) bin[m] = 0.f;
    }
    sgx_f32x4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < T; k0 += ATT_TK) {
        __syncthreads();
        att_stage(Ks, k + base, ld_pix, k0, T, d, dp);
        att_stage(Vs, v + base, ld_pix, k0, T, d, dp);
        __syncthreads();
        for (int u = 0; u < ATT_TK / 16; ++u) {
            const int kk = k0 + 16 * u;
            if (kk >= T) break;
            const sgx_f32x4 s = att_nt<NB>(qf, Ks + 16 * u * dp, dp, d, lane), dpv = att_nt<NB>(df, Vs + 16 * u * dp, dp, d, lane);
            const bool valid = kk + (lane & 15) < T;
            float ds[4];
            if constexpr (BIAS) {
                // p = exp(scale s + b - lse) written as scale s - (lse - b): with b = 0 the expression the plain kernel evaluates, bit for bit
                const int j = kk + (lane & 15), lj = rpb_lin(j, T, rp.gw);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float bias = Ts[rpb_index(q0 + (lane >> 4) * 4 + r, valid ? j : T - 1, li[r], lj, rp)];
                    ds[r] = valid ? expf(scale * s[r] - (L[r] - bias)) * (dpv[r] - dl[r]) : 0.f;
                    Dp[(16 * wave + (lane >> 4) * 4 + r) * (ATT_TK + 1) + 16 * u + (lane & 15)] = ds[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) ds[r] = valid ? expf(scale * s[r] - L[r]) * (dpv[r] - dl[r]) : 0.f;
            }
            sgx_wave_lds_sync();
            att_put_tile(Ss, ds, lane);
            sgx_wave_lds_sync();
            att_nn<NB>(acc, Ss, Ks + 16 * u * dp, dp, d, lane);
        }
        if constexpr (BIAS) {
            __syncthreads();  // the four waves' ds rows of this tile are parked
            rpb_gather<BINS>(bin, Dp, blockIdx.x * ATT_TQ, k0, T, rp);
        }
    }
    const float mul[4] = {scale, scale, scale, scale};
    att_store<NB>(dq + (long)b * g_ld_img + (long)h * d, g_ld_pix, q0, T, d, acc, mul, lane);
    if constexpr (BIAS) {
        float* row = dt_part + (((long)b * gridDim.x + blockIdx.x) * heads + h) * rp.N;
#pragma unroll
        for (int m = 0; m < BINS; ++m) {
            const int r = (int)threadIdx.x + ATT_THREADS * m;
            if (r < rp.N) row[r] = bin[m];
        }
    }
}

// dtable[r][h] += the partial rows of bin (r, h), one rounding onto the arena view.  A workgroup owns 16 bins of one head; 16 threads per bin
// each add a contiguous sixteenth of the (image, row tile) sequence in ascending order in fp64, and the bin's first thread adds the sixteen
// sub-sums in ascending order: a fixed order that depends on the shape alone (36 workgroups of one serial chain each took as long as a
// fifth of the attention backward at batch 64).
#define RPB_FIN_BINS 16
#define RPB_FIN_CHUNKS 16
__global__ __launch_bounds__(RPB_FIN_BINS * RPB_FIN_CHUNKS) void attn_rpb_dtable_finalize_kernel(int nparts, int heads, int N, const float* __restrict__ parts,
                                                                                                 float* dtable, long ld) {
    __shared__ double sub[RPB_FIN_CHUNKS][RPB_FIN_BINS];
    const int rb = threadIdx.x % RPB_FIN_BINS, c = threadIdx.x / RPB_FIN_BINS;
    const int r = blockIdx.x * RPB_FIN_BINS + rb, h = blockIdx.y;
    const int per = (nparts + RPB_FIN_CHUNKS - 1) / RPB_FIN_CHUNKS;
    const int i0 = c * per, i1 = i0 + per < nparts ? i0 + per : nparts;
    double a = 0.0;
    if (r < N) {
        const float* p = parts + (long)h * N + r;
        const long step = (long)heads * N;
#pragma unroll 4
        for (int i = i0; i < i1; ++i) a += (double)p[i * step];
    }
    sub[c][rb] = a;
    __syncthreads();
    if (c == 0 && r < N) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < RPB_FIN_CHUNKS; ++k) t += sub[k][rb];
        dtable[(long)r * ld + h] += (float)t;
    }
}

template <int NB, bool BIAS>
__global__ __launch_bounds__(ATT_THREADS) void attn_bwd_dkv_kernel(int T, int d, int heads, const float* q, const float* k, const float* v, long ld_pix,
                                                                   long ld_img, const float* dout, long o_ld_pix, long o_ld_img, const float* lse,
                                                                   const float* delta, float scale, float* dk, float* dv, long g_ld_pix,
                                                                   long g_ld_img, AttRpb rp) {
    SGX_DYN_SMEM(float, sm);
    const int dp = ((d + 15) & ~15) + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Qs = sm;
    float* Ds = Qs + ATT_TK * dp;
    float* Pt = Ds + ATT_TK * dp + wave * 512;
    float* St = Pt + 256;
    float* Ts = Ds + ATT_TK * dp + 4 * 512;
    const int h = blockIdx.y, b = blockIdx.z, j0 = blockIdx.x * ATT_TQ + 16 * wave;  // the wave's own key rows
    const long base = (long)b * ld_img + (long)h * d, obase = (long)b * o_ld_img + (long)h * d;
    const long sbase = ((long)b * heads + h) * T;
    float kf[4 * NB], vf[4 * NB];
    att_load_frag<NB>(kf, k + base, ld_pix, j0, T, d, lane);
    att_load_frag<NB>(vf, v + base, ld_pix, j0, T, d, lane);
    int lj[4];  // lin() of the lane's four accumulator rows (keys)
    if constexpr (BIAS) {
        rpb_stage(Ts, rp, h);
#pragma unroll
        for (int r = 0; r < 4; ++r) lj[r] = rpb_lin(j0 + (lane >> 4) * 4 + r, T, rp.gw);
    }
    sgx_f32x4 ak[NB], av[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) ak[nb] = av[nb] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < T; q0 += ATT_TK) {
        __syncthreads();
        att_stage(Qs, q + base, ld_pix, q0, T, d, dp);
        att_stage(Ds, dout + obase, o_ld_pix, q0, T, d, dp);
        __syncthreads();
        for (int u = 0; u < ATT_TK / 16; ++u) {
            const int qq = q0 + 16 * u;
            if (qq >= T) break;
            // transposed tiles: row = own key, column = streamed query
            const sgx_f32x4 s = att_nt<NB>(kf, Qs + 16 * u * dp, dp, d, lane), dpv = att_nt<NB>(vf, Ds + 16 * u * dp, dp, d, lane);
            const int i = qq + (lane & 15);
            const bool valid = i < T;
            const float Li = valid ? lse[sbase + i] : 0.f, Di = valid ? delta[sbase + i] : 0.f;
            float p[4], ds[4];
            if constexpr (BIAS) {
                const int li = rpb_lin(i, T, rp.gw);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + (lane >> 4) * 4 + r;
                    const float bias = Ts[rpb_index(valid ? i : T - 1, j < T ? j : T - 1, li, lj[r], rp)];
                    p[r] = valid ? expf(scale * s[r] - (Li - bias)) : 0.f;
                    ds[r] = p[r] * (dpv[r] - Di);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = valid ? expf(scale * s[r] - Li) : 0.f;
                    ds[r] = p[r] * (dpv[r] - Di);
                }
            }
            sgx_wave_lds_sync();
            att_put_tile(Pt, p, lane);
            att_put_tile(St, ds, lane);
            sgx_wave_lds_sync();
            att_nn<NB>(av, Pt, Ds + 16 * u * dp, dp, d, lane);
            att_nn<NB>(ak, St, Qs + 16 * u * dp, dp, d, lane);
        }
    }
    const float one[4] = {1.f, 1.f, 1.f, 1.f}, mul[4] = {scale, scale, scale, scale};
    att_store<NB>(dk + (long)b * g_ld_img + (long)h * d, g_ld_pix, j0, T, d, ak, mul, lane);
    att_store<NB>(dv + (long)b * g_ld_img + (long)h * d, g_ld_pix, j0, T, d, av, one, lane);
}

#define ATT_CHECK_DIMS(what)                                                                                                                  \
    SGX_CHECK_ARG(B > 0 && B <= 65535 && heads > 0 && heads <= 65535 && T > 0 && d >= 4 && d % 4 == 0 && d <= ATT_MAXD,                        \
                  "%s: need 1 <= B, heads <= 65535, T >= 1, d %% 4 == 0 and 4 <= d <= %d (B=%d heads=%d T=%d d=%d)", what, ATT_MAXD, B, heads, T, d)
#define ATT_DISPATCH(kernel, BIAS, patches, extra, ...)                                                                            \
    do {                                                                                                                           \
        const size_t smem__ = ((size_t)2 * ATT_TK * (((d + 15) & ~15) + 4) + 4 * 256 * (patches) + (extra)) * sizeof(float);       \
        const dim3 grid__(sgx_cdiv(T, ATT_TQ), heads, B), block__(ATT_THREADS);                                                    \
        if (d <= 64) SGX_LAUNCH((kernel<4, BIAS>), grid__, block__, smem__, stream, __VA_ARGS__);                                  \
        else SGX_LAUNCH((kernel<8, BIAS>), grid__, block__, smem__, stream, __VA_ARGS__);                                          \
    } while (0)

extern "C" int32_t sgx_attn_tile_rows(int32_t which) { return which == 0 ? ATT_TQ : ATT_TK; }
extern "C" int32_t sgx_attn_fwd(int32_t B, int32_t heads, int32_t T, int32_t d, const float* q, const float* k, const float* v, int64_t ld_pix,
                                int64_t ld_img, float scale, float* o, int64_t o_ld_pix, int64_t o_ld_img, float* lse, void* stream) {
    SGX_CHECK_ARG(q && k && v && o && lse, "attn_fwd: null pointer");
    ATT_CHECK_DIMS("attn_fwd");
    SGX_CHECK_ARG(VIT_LD4(ld_pix) && VIT_LD4(ld_img) && VIT_LD4(o_ld_pix) && VIT_LD4(o_ld_img) && VIT_ALIGNED(q) && VIT_ALIGNED(k) && VIT_ALIGNED(v) && VIT_ALIGNED(o),
                  "attn_fwd: strides and addresses must be multiples of 16 bytes");
    ATT_DISPATCH(attn_fwd_kernel, false, 1, 0, T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, scale, o, (long)o_ld_pix, (long)o_ld_img, lse, AttRpb{});
    SGX_CHECK_LAUNCH("attn_fwd");
    return SGX_OK;
}
extern "C" int64_t sgx_attn_bwd_workspace(int32_t B, int32_t heads, int32_t T) { return (int64_t)B * heads * T * (int64_t)sizeof(float) + 256; }
extern "C" int32_t sgx_attn_bwd(int32_t B, int32_t heads, int32_t T, int32_t d, const float* q, const float* k, const float* v, int64_t ld_pix,
                                int64_t ld_img, const float* o, const float* dout, int64_t o_ld_pix, int64_t o_ld_img, const float* lse, float scale,
                                float* dq, float* dk, float* dv, int64_t g_ld_pix, int64_t g_ld_img, void* ws, int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(q && k && v && o && dout && lse && dq && dk && dv, "attn_bwd: null pointer");
    ATT_CHECK_DIMS("attn_bwd");
    SGX_CHECK_ARG(VIT_LD4(ld_pix) && VIT_LD4(ld_img) && VIT_LD4(o_ld_pix) && VIT_LD4(o_ld_img) && VIT_LD4(g_ld_pix) && VIT_LD4(g_ld_img) && VIT_ALIGNED(q) &&
                      VIT_ALIGNED(k) && VIT_ALIGNED(v) && VIT_ALIGNED(o) && VIT_ALIGNED(dout) && VIT_ALIGNED(dq) && VIT_ALIGNED(dk) && VIT_ALIGNED(dv) &&
                      VIT_ALIGNED(ws),
                  "attn_bwd: strides and addresses must be multiples of 16 bytes");
    SGX_CHECK_ARG(ws && ws_bytes >= sgx_attn_bwd_workspace(B, heads, T), "attn_bwd: workspace too small");
    ATT_DISPATCH(attn_bwd_dq_kernel, ATT_T2(false, 1), 1, 0, T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, o, dout, (long)o_ld_pix, (long)o_ld_img, lse, scale, dq,
                 (long)g_ld_pix, (long)g_ld_img, (float*)ws, AttRpb{}, (float*)nullptr);
    SGX_CHECK_LAUNCH("attn_bwd (dq)");
    ATT_DISPATCH(attn_bwd_dkv_kernel, false, 2, 0, T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, dout, (long)o_ld_pix, (long)o_ld_img, lse, (const float*)ws,
                 scale, dk, dv, (long)g_ld_pix, (long)g_ld_img, AttRpb{});
    SGX_CHECK_LAUNCH("attn_bwd (dk, dv)");
    return SGX_OK;
}

// With a relative position bias: the same operands plus the token grid (T == gh gw + 1) and the table [N][heads] with its row stride
// (tab_ld >= heads floats; the parameter's own layout has tab_ld == heads).  N = (2 gh - 1)(2 gw - 1) + 3 <= ATT_RPB_MAXN (4096: grids up to
// 32 x 32; 16 KB of LDS beside the 38 KB of the staged rows at d = 128) - anything else is SGX_ERR_BAD_ARG with nothing launched.
// The backward adds the table's gradient onto dtable (same layout, its own row stride).  Workspace: Delta [B heads T], then one partial row
// [N] of the table gradient per (image, row tile, head).
#define ATT_RPB_CHECK(what)                                                                                                                          \
    SGX_CHECK_ARG(gh > 0 && gw > 0 && (long)gh * gw + 1 == T, "%s: T = %d is not gh * gw + 1 (grid %d x %d)", what, T, gh, gw);                      \
    SGX_CHECK_ARG((2L * gh - 1) * (2L * gw - 1) + 3 <= ATT_RPB_MAXN, "%s: the %d x %d grid has %ld table rows, the LDS cap is %d", what, gh, gw,     \
                  (2L * gh - 1) * (2L * gw - 1) + 3, ATT_RPB_MAXN);                                                                                  \
    SGX_CHECK_ARG(table && tab_ld >= heads, "%s: the table's row stride (%ld) must be at least heads (%d)", what, (long)tab_ld, heads)
static AttRpb att_rpb(const float* table, int64_t tab_ld, int gh, int gw) {
    return AttRpb{table, (long)tab_ld, gh, gw, (2 * gh - 1) * (2 * gw - 1) + 3, (gh - 1) * (2 * gw - 1) + gw - 1};
}
extern "C" int32_t sgx_attn_rpb_max_rows(void) { return ATT_RPB_MAXN; }
extern "C" int32_t sgx_attn_rpb_fwd(int32_t B, int32_t heads, int32_t T, int32_t d, int32_t gh, int32_t gw, const float* q, const float* k, const float* v,
                                    int64_t ld_pix, int64_t ld_img, float scale, const float* table, int64_t tab_ld, float* o, int64_t o_ld_pix,
                                    int64_t o_ld_img, float* lse, void* stream) {
    SGX_CHECK_ARG(q && k && v && o && lse, "attn_rpb_fwd: null pointer");
    ATT_CHECK_DIMS("attn_rpb_fwd");
    ATT_RPB_CHECK("attn_rpb_fwd");
    SGX_CHECK_ARG(VIT_LD4(ld_pix) && VIT_LD4(ld_img) && VIT_LD4(o_ld_pix) && VIT_LD4(o_ld_img) && VIT_ALIGNED(q) && VIT_ALIGNED(k) && VIT_ALIGNED(v) && VIT_ALIGNED(o),
                  "attn_rpb_fwd: strides and addresses must be multiples of 16 bytes");
    const AttRpb rp = att_rpb(table, tab_ld, gh, gw);
    ATT_DISPATCH(attn_fwd_kernel, true, 1, rp.N, T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, scale, o, (long)o_ld_pix, (long)o_ld_img, lse, rp);
    SGX_CHECK_LAUNCH("attn_rpb_fwd");
    return SGX_OK;
}
extern "C" int64_t sgx_attn_rpb_bwd_workspace(int32_t B, int32_t heads, int32_t T, int32_t gh, int32_t gw) {
    const int64_t N = (2L * gh - 1) * (2L * gw - 1) + 3, tiles = (T + ATT_TQ - 1) / ATT_TQ;
    return ((int64_t)B * heads * T + (int64_t)B * tiles * heads * N) * (int64_t)sizeof(float) + 256;
}
extern "C" int32_t sgx_attn_rpb_bwd(int32_t B, int32_t heads, int32_t T, int32_t d, int32_t gh, int32_t gw, const float* q, const float* k, const float* v,
                                    int64_t ld_pix, int64_t ld_img, const float* o, const float* dout, int64_t o_ld_pix, int64_t o_ld_img, const float* lse,
                                    float scale, const float* table, int64_t tab_ld, float* dq, float* dk, float* dv, int64_t g_ld_pix, int64_t g_ld_img,
                                    float* dtable, int64_t dtab_ld, void* ws, int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(q && k && v && o && dout && lse && dq && dk && dv && dtable, "attn_rpb_bwd: null pointer");
    ATT_CHECK_DIMS("attn_rpb_bwd");
    ATT_RPB_CHECK("attn_rpb_bwd");
    SGX_CHECK_ARG(dtab_ld >= heads, "attn_rpb_bwd: the table gradient's row stride (%ld) must be at least heads (%d)", (long)dtab_ld, heads);
    SGX_CHECK_ARG(VIT_LD4(ld_pix) && VIT_LD4(ld_img) && VIT_LD4(o_ld_pix) && VIT_LD4(o_ld_img) && VIT_LD4(g_ld_pix) && VIT_LD4(g_ld_img) && VIT_ALIGNED(q) &&
                      VIT_ALIGNED(k) && VIT_ALIGNED(v) && VIT_ALIGNED(o) && VIT_ALIGNED(dout) && VIT_ALIGNED(dq) && VIT_ALIGNED(dk) && VIT_ALIGNED(dv) &&
                      VIT_ALIGNED(ws),
                  "attn_rpb_bwd: strides and addresses must be multiples of 16 bytes");
    SGX_CHECK_ARG(ws && ws_bytes >= sgx_attn_rpb_bwd_workspace(B, heads, T, gh, gw), "attn_rpb_bwd: workspace too small");
    const AttRpb rp = att_rpb(table, tab_ld, gh, gw);
    float* delta = (float*)ws;
    float* parts = delta + (((long)B * heads * T + 3) & ~3L);
    const int tiles = sgx_cdiv(T, ATT_TQ);
    if (rp.N <= 4 * ATT_THREADS)
        ATT_DISPATCH(attn_bwd_dq_kernel, ATT_T2(true, 4), 1, rp.N + ATT_TQ * (ATT_TK + 1), T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, o, dout,
                     (long)o_ld_pix, (long)o_ld_img, lse, scale, dq, (long)g_ld_pix, (long)g_ld_img, delta, rp, parts);
    else
        ATT_DISPATCH(attn_bwd_dq_kernel, ATT_T2(true, ATT_RPB_BINS), 1, rp.N + ATT_TQ * (ATT_TK + 1), T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, o, dout,
                     (long)o_ld_pix, (long)o_ld_img, lse, scale, dq, (long)g_ld_pix, (long)g_ld_img, delta, rp, parts);
    SGX_CHECK_LAUNCH("attn_rpb_bwd (dq)");
    ATT_DISPATCH(attn_bwd_dkv_kernel, true, 2, rp.N, T, d, heads, q, k, v, (long)ld_pix, (long)ld_img, dout, (long)o_ld_pix, (long)o_ld_img, lse,
                 (const float*)delta, scale, dk, dv, (long)g_ld_pix, (long)g_ld_img, rp);
    SGX_CHECK_LAUNCH("attn_rpb_bwd (dk, dv)");
    SGX_LAUNCH(attn_rpb_dtable_finalize_kernel, dim3(sgx_cdiv(rp.N, RPB_FIN_BINS), heads), dim3(RPB_FIN_BINS * RPB_FIN_CHUNKS), 0, stream, B * tiles, heads, rp.N, (const float*)parts, dtable,
               (long)dtab_ld);
    SGX_CHECK_LAUNCH("attn_rpb_bwd (table gradient)");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// Layer scale with an optional per-image multiplier (BEiT's gamma_1 / gamma_2 and stochastic depth): y = x + m_b (gamma * t) over the rows of a
// [B, T, 1, C] stream (row r belongs to image r / rows_per_img); gamma [C] or NULL (ones), m [B] or NULL (ones); y may alias x.  Backward:
// dt = m_b gamma * dy (dt may alias dy; the skip's gradient is dy itself), dgamma += sum_rows m_b dy * t - partial rows of LS_BLOCK_ROWS rows
// on the sweep skeleton, added in block order in fp64 onto the arena view.
#define LS_BLOCK_ROWS 64
struct LayerScaleFwdF {
    const float* x; long x_ld; const float* t; long t_ld; const float* gamma; const float* m; long rows_per_img; float* y; long y_ld;
    struct In { float4 a, b; float mul; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(x + r * x_ld + c), sgx_ld4(t + r * t_ld + c), m ? m[r / rows_per_img] : 1.f}; }
    struct Cst { float4 g; };
    __device__ Cst consts(int c) const { return Cst{gamma ? sgx_ld4(gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f)}; }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        sgx_st4(y + r * y_ld + c, make_float4(in.a.x + in.mul * (k.g.x * in.b.x), in.a.y + in.mul * (k.g.y * in.b.y), in.a.z + in.mul * (k.g.z * in.b.z),
                                              in.a.w + in.mul * (k.g.w * in.b.w)));
    }
};
template <bool WITH_T>
struct LayerScaleBwdF {
    const float* dy; long dy_ld; const float* t; long t_ld; const float* gamma; const float* m; long rows_per_img; float* dt; long dt_ld;
    struct In { float4 d, b; float mul; };
    __device__ In load(long r, int c) const {
        return In{sgx_ld4(dy + r * dy_ld + c), WITH_T ? sgx_ld4(t + r * t_ld + c) : make_float4(0.f, 0.f, 0.f, 0.f), m ? m[r / rows_per_img] : 1.f};
    }
    struct Cst { float4 g; };
    __device__ Cst consts(int c) const { return Cst{gamma ? sgx_ld4(gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f)}; }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&q)[1]) const {
        const float4 md = make_float4(in.mul * in.d.x, in.mul * in.d.y, in.mul * in.d.z, in.mul * in.d.w);
        if (WITH_T) { q[0].x += md.x * in.b.x; q[0].y += md.y * in.b.y; q[0].z += md.z * in.b.z; q[0].w += md.w * in.b.w; }
        sgx_st4(dt + r * dt_ld + c, make_float4(md.x * k.g.x, md.y * k.g.y, md.z * k.g.z, md.w * k.g.w));
    }
};
__global__ void layerscale_dgamma_finalize_kernel(int nblk, int C, const float* partials, float* dgamma) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0;
    for (int k = 0; k < nblk; ++k) a += (double)partials[(long)k * C + c];
    dgamma[c] += (float)a;
}
extern "C" int32_t sgx_layerscale_fwd(const float* x, int64_t x_ld, const float* t, int64_t t_ld, const float* gamma, const float* m, int64_t rows_per_img,
                                      float* y, int64_t y_ld, int64_t M, int32_t C, void* stream) {
    SGX_CHECK_ARG(x && t && y && rows_per_img > 0 && M % rows_per_img == 0, "layerscale_fwd: null pointer, or M is not a whole number of images");
    SGX_CHECK_ARG(VIT_LD4(x_ld) && VIT_LD4(t_ld) && VIT_LD4(y_ld) && VIT_ALIGNED(x) && VIT_ALIGNED(t) && VIT_ALIGNED(y) && VIT_ALIGNED(gamma),
                  "layerscale_fwd: strides and addresses must be multiples of 16 bytes");
    LayerScaleFwdF f{x, (long)x_ld, t, (long)t_ld, gamma, m, (long)rows_per_img, y, (long)y_ld};
    return run_sweep<LayerScaleFwdF, 0, 2>(f, M, C, nullptr, stream, "layerscale_fwd");
}
extern "C" int32_t sgx_layerscale_block_rows(void) { return LS_BLOCK_ROWS; }
extern "C" int64_t sgx_layerscale_bwd_workspace(int64_t M, int32_t C) {
    return ((M + LS_BLOCK_ROWS - 1) / LS_BLOCK_ROWS) * (int64_t)C * (int64_t)sizeof(float) + 256;
}
extern "C" int32_t sgx_layerscale_bwd(const float* dy, int64_t dy_ld, const float* t, int64_t t_ld, const float* gamma, const float* m, int64_t rows_per_img,
                                      float* dt, int64_t dt_ld, float* dgamma, int64_t M, int32_t C, void* ws, int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(dy && dt && rows_per_img > 0 && M % rows_per_img == 0, "layerscale_bwd: null pointer, or M is not a whole number of images");
    SGX_CHECK_ARG((dgamma == nullptr) || (gamma && t), "layerscale_bwd: dgamma needs gamma and the branch output t");
    SGX_CHECK_ARG(VIT_LD4(dy_ld) && VIT_LD4(t_ld) && VIT_LD4(dt_ld) && VIT_ALIGNED(dy) && VIT_ALIGNED(t) && VIT_ALIGNED(dt) && VIT_ALIGNED(gamma) &&
                      VIT_ALIGNED(dgamma) && VIT_ALIGNED(ws),
                  "layerscale_bwd: strides and addresses must be multiples of 16 bytes");
    if (!dgamma) {
        LayerScaleBwdF<false> f{dy, (long)dy_ld, nullptr, 0, gamma, m, (long)rows_per_img, dt, (long)dt_ld};
        return run_sweep<LayerScaleBwdF<false>, 0, 2>(f, M, C, nullptr, stream, "layerscale_bwd");
    }
    SGX_CHECK_ARG(ws && ws_bytes >= sgx_layerscale_bwd_workspace(M, C), "layerscale_bwd: workspace too small");
    const int nblk = (int)((M + LS_BLOCK_ROWS - 1) / LS_BLOCK_ROWS);
    LayerScaleBwdF<true> f{dy, (long)dy_ld, t, (long)t_ld, gamma, m, (long)rows_per_img, dt, (long)dt_ld};
    const int32_t rc = run_sweep<LayerScaleBwdF<true>, 1, 2>(f, M, C, (float*)ws, stream, "layerscale_bwd", nblk);
    if (rc != SGX_OK) return rc;
    SGX_LAUNCH(layerscale_dgamma_finalize_kernel, dim3(sgx_cdiv(C, 256)), dim3(256), 0, stream, nblk, C, (const float*)ws, dgamma);
    SGX_CHECK_LAUNCH("layerscale_bwd (finalize)");
    return SGX_OK;
}

// Mean over the patch tokens (BEiT's global_pool = "avg"): y[b] = mean of rows 1 .. T - 1 of x[b] in ascending row order.  Backward: the whole
// [B, T, 1, D] gradient - row 0 zero, every other row dy[b] / (T - 1).
__global__ __launch_bounds__(256) void token_mean_fwd_kernel(int B, int T, int D4, const float* x, long x_ld_pix, long x_ld_img, float* y, long y_ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D4) return;
    const int c = (i % D4) * 4, b = i / D4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 1; t < T; ++t) {
        const float4 a = sgx_ld4(x + (long)b * x_ld_img + (long)t * x_ld_pix + c);
        s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
    }
    const float inv = 1.f / (float)(T - 1);
    sgx_st4(y + (long)b * y_ld + c, make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv));
}
__global__ __launch_bounds__(256) void token_mean_bwd_kernel(int B, int T, int D4, const float* dy, long dy_ld, float* dx, long x_ld_pix, long x_ld_img) {
    const long n = (long)B * T * D4;
    const float inv = 1.f / (float)(T - 1);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % D4) * 4;
        const long r = i / D4;
        const int t = (int)(r % T);
        const long b = r / T;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t > 0) {
            const float4 a = sgx_ld4(dy + b * dy_ld + c);
            g = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
        }
        sgx_st4(dx + b * x_ld_img + (long)t * x_ld_pix + c, g);
    }
}
extern "C" int32_t sgx_token_mean_fwd(int32_t B, int32_t T, int32_t D, const float* x, int64_t x_ld_pix, int64_t x_ld_img, float* y, int64_t y_ld, void* stream) {
    SGX_CHECK_ARG(x && y && B > 0 && T > 1 && D > 0 && D % 4 == 0 && (long)B * (D / 4) < 0x7fffffffL, "token_mean_fwd: bad args (T=%d D=%d)", T, D);
    SGX_CHECK_ARG(VIT_LD4(x_ld_pix) && VIT_LD4(x_ld_img) && VIT_LD4(y_ld) && VIT_ALIGNED(x) && VIT_ALIGNED(y),
                  "token_mean_fwd: strides and addresses must be multiples of 16 bytes");
    SGX_LAUNCH(token_mean_fwd_kernel, dim3(sgx_cdiv((long)B * (D / 4), 256)), dim3(256), 0, stream, B, T, D / 4, x, (long)x_ld_pix, (long)x_ld_img, y, (long)y_ld);
    SGX_CHECK_LAUNCH("token_mean_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_token_mean_bwd(int32_t B, int32_t T, int32_t D, const float* dy, int64_t dy_ld, float* dx, int64_t x_ld_pix, int64_t x_ld_img, void* stream) {
    SGX_CHECK_ARG(dy && dx && B > 0 && T > 1 && D > 0 && D % 4 == 0, "token_mean_bwd: bad args (T=%d D=%d)", T, D);
    SGX_CHECK_ARG(VIT_LD4(x_ld_pix) && VIT_LD4(x_ld_img) && VIT_LD4(dy_ld) && VIT_ALIGNED(dx) && VIT_ALIGNED(dy),
                  "token_mean_bwd: strides and addresses must be multiples of 16 bytes");
    const long n = (long)B * T * (D / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(token_mean_bwd_kernel, dim3((unsigned)SGX_STRIDE_GRID(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, B, T, D / 4, dy, (long)dy_ld, dx,
               (long)x_ld_pix, (long)x_ld_img);
    SGX_CHECK_LAUNCH("token_mean_bwd");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// Patch rows: the standardised NHWC input [B, gh * ph, gw * pw, C] -> [B, gh * gw, 1, ph * pw * C] rows in (py, px, c) order - the order of a
// [D, C, ph, pw] filter stored OHWI, so the patch embedding is a 1x1 convolution.  One thread moves one float4; nothing is computed.
__global__ __launch_bounds__(256) void patch_rows_kernel(int B, int gh, int gw, int ph, int pw, int C4, const float* x, long x_ld_pix, long x_ld_img,
                                                         float* y, long y_ld_pix, long y_ld_img) {
    const long n = (long)B * gh * gw * ph * pw * C4;
    const long W = (long)gw * pw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        long t = i;
        const int c4 = (int)(t % C4); t /= C4;
        const int px = (int)(t % pw); t /= pw;
        const int py = (int)(t % ph); t /= ph;
        const int gx = (int)(t % gw); t /= gw;
        const int gy = (int)(t % gh);
        const long b = t / gh;
        const float4 v = sgx_ld4(x + b * x_ld_img + (((long)gy * ph + py) * W + (long)gx * pw + px) * x_ld_pix + 4 * c4);
        sgx_st4(y + b * y_ld_img + ((long)gy * gw + gx) * y_ld_pix + ((long)(py * pw + px) * C4 + c4) * 4, v);
    }
}
extern "C" int32_t sgx_patch_rows(int32_t B, int32_t gh, int32_t gw, int32_t ph, int32_t pw, int32_t C, const float* x, int64_t x_ld_pix, int64_t x_ld_img,
                                  float* y, int64_t y_ld_pix, int64_t y_ld_img, void* stream) {
    SGX_CHECK_ARG(x && y && B > 0 && gh > 0 && gw > 0 && ph > 0 && pw > 0 && C > 0 && C % 4 == 0, "patch_rows: bad args (C=%d)", C);
    SGX_CHECK_ARG(VIT_LD4(x_ld_pix) && VIT_LD4(x_ld_img) && VIT_LD4(y_ld_pix) && VIT_LD4(y_ld_img) && VIT_ALIGNED(x) && VIT_ALIGNED(y),
                  "patch_rows: strides and addresses must be multiples of 16 bytes");
    const long n = (long)B * gh * gw * ph * pw * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(patch_rows_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, B, gh, gw, ph, pw, C / 4, x, (long)x_ld_pix,
               (long)x_ld_img, y, (long)y_ld_pix, (long)y_ld_img);
    SGX_CHECK_LAUNCH("patch_rows");
    return SGX_OK;
}

// Token assembly: x[b][0] = cls + pos[0], x[b][1 + i] = patch[b][i] + pos[1 + i] (T = 1 + patches per image), one launch; pos / dpos may be
// NULL (no position embedding: the rows move unchanged, the backward sums the class-token row only).  Backward:
// dpos[t] += sum_b dx[b][t] in ascending image order (fp64 accumulator, one rounding), dcls += the row-0 sum; the patch rows' gradient is the
// view dx[:, 1:] and needs no kernel.
__global__ __launch_bounds__(256) void token_assemble_kernel(int B, int T, int D4, const float* patch, long p_ld_pix, long p_ld_img, const float* cls,
                                                             const float* pos, float* x, long x_ld_pix, long x_ld_img) {
    const long n = (long)B * T * D4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % D4) * 4;
        const long r = i / D4;
        const int t = (int)(r % T);
        const long b = r / T;
        const float4 a = t == 0 ? sgx_ld4(cls + c) : sgx_ld4(patch + b * p_ld_img + (long)(t - 1) * p_ld_pix + c);
        if (!pos) {  // (BEiT without an absolute position embedding: the rows move as they are)
            sgx_st4(x + b * x_ld_img + (long)t * x_ld_pix + c, a);
            continue;
        }
        const float4 p = sgx_ld4(pos + (long)t * D4 * 4 + c);
        sgx_st4(x + b * x_ld_img + (long)t * x_ld_pix + c, make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w));
    }
}
__global__ __launch_bounds__(256) void token_assemble_bwd_kernel(int B, int T, int D4, const float* dx, long x_ld_pix, long x_ld_img, float* dcls,
                                                                 float* dpos) {
    const long n = (long)(dpos ? T : 1) * D4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % D4) * 4;
        const int t = (int)(i / D4);
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < B; ++b) {
            const float4 a = sgx_ld4(dx + (long)b * x_ld_img + (long)t * x_ld_pix + c);
            s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
        }
        const float4 r = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
        float4 o;
        if (dpos) {
            o = sgx_ld4(dpos + (long)t * D4 * 4 + c);
            sgx_st4(dpos + (long)t * D4 * 4 + c, make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w));
        }
        if (t == 0) {
            o = sgx_ld4(dcls + c);
            sgx_st4(dcls + c, make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w));
        }
    }
}
extern "C" int32_t sgx_token_assemble_fwd(int32_t B, int32_t T, int32_t D, const float* patch, int64_t p_ld_pix, int64_t p_ld_img, const float* cls,
                                          const float* pos, float* x, int64_t x_ld_pix, int64_t x_ld_img, void* stream) {
    SGX_CHECK_ARG(cls && x && (patch || T == 1) && B > 0 && T > 0 && D > 0 && D % 4 == 0, "token_assemble_fwd: bad args (D=%d)", D);
    SGX_CHECK_ARG(VIT_LD4(p_ld_pix) && VIT_LD4(p_ld_img) && VIT_LD4(x_ld_pix) && VIT_LD4(x_ld_img) && VIT_ALIGNED(patch) && VIT_ALIGNED(cls) && VIT_ALIGNED(pos) &&
                      VIT_ALIGNED(x),
                  "token_assemble_fwd: strides and addresses must be multiples of 16 bytes");
    const long n = (long)B * T * (D / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(token_assemble_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, B, T, D / 4, patch, (long)p_ld_pix,
               (long)p_ld_img, cls, pos, x, (long)x_ld_pix, (long)x_ld_img);
    SGX_CHECK_LAUNCH("token_assemble_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_token_assemble_bwd(int32_t B, int32_t T, int32_t D, const float* dx, int64_t x_ld_pix, int64_t x_ld_img, float* dcls, float* dpos,
                                          void* stream) {
    SGX_CHECK_ARG(dx && dcls && B > 0 && T > 0 && D > 0 && D % 4 == 0, "token_assemble_bwd: bad args (D=%d)", D);
    SGX_CHECK_ARG(VIT_LD4(x_ld_pix) && VIT_LD4(x_ld_img) && VIT_ALIGNED(dx) && VIT_ALIGNED(dcls) && VIT_ALIGNED(dpos),
                  "token_assemble_bwd: strides and addresses must be multiples of 16 bytes");
    const long n = (long)(dpos ? T : 1) * (D / 4), blocks = (n + 255) / 256;  // (no position embedding: the class-token row alone)
    SGX_LAUNCH(token_assemble_bwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, B, T, D / 4, dx, (long)x_ld_pix,
               (long)x_ld_img, dcls, dpos);
    SGX_CHECK_LAUNCH("token_assemble_bwd");
    return SGX_OK;
}
