// DenseNet kernels (classification_models/densenet.py) - included by bn.hip, built on its sweep skeleton and finalize pieces.
//
// A dense block keeps ONE concat buffer [N, H, W, C_total]; every layer reads a channel prefix of it and writes growth_rate channels behind
// that prefix.  The batch sum and sum of squares of a channel do not depend on which BatchNorm looks at it, so they are folded ONCE - where
// the slice is produced, from the partial rows its producer leaves - into the block's statistics record: fp64 [2][rec_ld] (plane 0 sums,
// plane 1 sums of squares).  Every BatchNorm over a prefix of the buffer (each layer's norm1, the transition's norm, norm5) finalises its
// own scale / shift / running statistics from the record's prefix: no statistics sweep ever re-reads the concat buffer.
//   sgx_dense_stats_reduce      producer's [2][nblk][C_slice] partial rows -> record[:, c_off : c_off + C_slice]
//   sgx_dense_bn_finalize       record[:, 0 : C_in] -> one BatchNorm's scale, shift, save_mean, save_invstd, running statistics
//   sgx_dense_bn_bwd_apply      sgx_bn_bwd_apply with dx += ...: a layer's norm1 adds its input gradient to the prefix of the block's gradient
//                               buffer that the layers behind it have already written
//   sgx_bn_act_avgpool2_*       the transition's BatchNorm -> activation -> AvgPool2d(2, 2) as one sweep, forward and backward
// No atomics; every sum has a fixed order, so every output repeats bit for bit.
#pragma once

// ---------------------------------------------------------------------------------------------
// the column totals of the partial rows, stored with the record's plane stride (col_totals: the order of sgx_bn_reduce_sums, bit for bit)
__global__ void dense_stats_kernel(ColSrc src, int C, double* rec, long rec_ld) {
    SGX_FIN_THREAD(src, C);
    double tot[2];
    col_totals<2>(src, C, c, cok, tot);
    if (writer) {
        rec[c] = tot[0];
        rec[rec_ld + c] = tot[1];
    }
}
extern "C" int32_t sgx_dense_stats_reduce(const float* partials, int32_t nblk, int32_t C_slice, double* record, int64_t rec_ld, int32_t c_off, void* ws,
                                          int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(partials && record && nblk > 0, "dense_stats_reduce: bad args");
    SW_CHECK_VEC(C_slice, SW_LD4(rec_ld) && SW_LD4(c_off) && SW_ALIGNED(partials) && SW_ALIGNED(record), "dense_stats_reduce");
    SGX_CHECK_ARG(c_off >= 0 && (int64_t)c_off + C_slice <= rec_ld, "dense_stats_reduce: channels %d..%d outside the record's %ld", c_off, c_off + C_slice, (long)rec_ld);
    ColSrc src;
    int32_t rc = col_prereduce<2>(partials, nblk, C_slice, ws, ws_bytes, stream, &src);
    if (rc) return rc;
    SGX_LAUNCH(dense_stats_kernel, fin_grid(src, C_slice), fin_block(src), 0, stream, src, C_slice, record + c_off, (long)rec_ld);
    SGX_CHECK_LAUNCH("dense_stats_reduce");
    return SGX_OK;
}

__global__ void dense_bn_finalize_kernel(const double* rec, long rec_ld, long M, int C, const float* gamma, const float* beta, float eps, float momentum,
                                         float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_finalize_channel(rec[c], rec[rec_ld + c], M, c, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd, scale, shift);
}
extern "C" int32_t sgx_dense_bn_finalize(const double* record, int64_t rec_ld, int64_t M, int32_t C_in, const float* gamma, const float* beta, float eps,
                                         float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* scale,
                                         float* shift, void* stream) {
    SGX_CHECK_ARG(record && scale && shift && M > 0, "dense_bn_finalize: bad args");
    SW_CHECK_VEC(C_in, SW_LD4(rec_ld) && SW_ALIGNED(record) && SW_ALIGNED(gamma) && SW_ALIGNED(beta) && SW_ALIGNED(running_mean) && SW_ALIGNED(running_var) &&
                           SW_ALIGNED(save_mean) && SW_ALIGNED(save_invstd) && SW_ALIGNED(scale) && SW_ALIGNED(shift),
                 "dense_bn_finalize");
    SGX_CHECK_ARG(C_in <= rec_ld, "dense_bn_finalize: prefix of %d channels outside the record's %ld", C_in, (long)rec_ld);
    SGX_LAUNCH(dense_bn_finalize_kernel, dim3(sgx_cdiv(C_in, 64)), dim3(64), 0, stream, record, (long)rec_ld, (long)M, C_in, gamma, beta, eps, momentum,
               running_mean, running_var, save_mean, save_invstd, scale, shift);
    SGX_CHECK_LAUNCH("dense_bn_finalize");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm backward, stage 3, accumulating: three tensors are read per row (dy, x, the gradient already in dx), two rows in flight
struct DenseBnBwdApplyF : BnBwdApplyF {
    struct In { float4 d, v, a; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(dy + r * dy_ld + c), sgx_ld4(x + r * x_ld + c), sgx_ld4(dx + r * dx_ld + c)}; }
    __device__ void apply(long r, int c, const In& in, const Cst& kc, float4 (&)[1]) const {
        float4 g;
        const float4 o = dx_of(in.d, in.v, kc, g), a = in.a;
        sgx_st4(dx + r * dx_ld + c, make_float4(a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w));
    }
};
extern "C" int32_t sgx_dense_bn_bwd_apply(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* scale, const float* shift,
                                          const float* coef, float* dx, int64_t dx_ld, int64_t M, int32_t C, int32_t act, void* stream) {
    SGX_CHECK_ARG(dy && x && scale && shift && coef && dx, "dense_bn_bwd_apply: null pointer");
    SGX_CHECK_ACT4(act, "dense_bn_bwd_apply");
    SW_CHECK_VEC(C, SW_LD4(dy_ld) && SW_LD4(x_ld) && SW_LD4(dx_ld) && SW_ALIGNED(dy) && SW_ALIGNED(x) && SW_ALIGNED(scale) && SW_ALIGNED(shift) && SW_ALIGNED(coef) &&
                        SW_ALIGNED(dx),
                 "dense_bn_bwd_apply");
    DenseBnBwdApplyF f{{dy, dy_ld, x, x_ld, scale, shift, coef, C, dx, dx_ld, nullptr, 0, act}};
    return run_sweep<DenseBnBwdApplyF, 0, 2>(f, M, C, nullptr, stream, "dense_bn_bwd_apply");
}

// ---------------------------------------------------------------------------------------------
// BatchNorm -> activation -> AvgPool2d(2, 2) (the reference's _Transition runs its 1x1 convolution before the pool; both are linear, so the
// product pools first and convolves a quarter of the pixels).  Odd H or W: the last row / column lies outside every window.
// Pixel indices stay below 2^31 (checked by the entry points): rows split into (image, y, x) with two multiply-high divisions.
struct PoolGeom {
    int H, W, Ho, Wo;
    sgx_fastdiv dW, dH;  // divisors of the map the sweep's rows run over: the pooled map forward, the full map backward
};
static int32_t pool_geom(int32_t N, int32_t H, int32_t W, bool pooled_rows, PoolGeom* g, const char* what) {
    SGX_CHECK_ARG(N > 0 && H >= 2 && W >= 2, "%s: need N>0 and a map of at least 2x2 (N=%d H=%d W=%d)", what, N, H, W);
    SGX_CHECK_ARG((int64_t)N * H * W <= 0x7fffffffL, "%s: more than 2^31 pixels", what);
    g->H = H, g->W = W, g->Ho = H / 2, g->Wo = W / 2;
    g->dW = sgx_make_fastdiv(pooled_rows ? g->Wo : W);
    g->dH = sgx_make_fastdiv(pooled_rows ? g->Ho : H);
    return SGX_OK;
}

// forward: a row is one POOLED pixel; its four source pixels are loaded together, two rows (eight loads) in flight
struct BnActAvgpool2F {
    const float* x; long x_ld; const float* scale; const float* shift; float* y; long y_ld; PoolGeom g; int act;
    struct In { float4 a, b, c, d; };
    __device__ In load(long r, int c) const {
        const int t = sgx_fdiv((int)r, g.dW), wo = (int)r - t * g.Wo, n = sgx_fdiv(t, g.dH), ho = t - n * g.Ho;
        const float* p = x + (((long)n * g.H + 2 * ho) * g.W + 2 * wo) * x_ld + c;
        return In{sgx_ld4(p), sgx_ld4(p + x_ld), sgx_ld4(p + g.W * x_ld), sgx_ld4(p + (g.W + 1) * x_ld)};
    }
    struct Cst { float4 s, t; };
    __device__ Cst consts(int c) const { return Cst{sgx_ld4(scale + c), sgx_ld4(shift + c)}; }
    __device__ float4 act4(const float4& v, const Cst& k) const {
        return make_float4(sgx_act6(k.s.x * v.x + k.t.x, act), sgx_act6(k.s.y * v.y + k.t.y, act), sgx_act6(k.s.z * v.z + k.t.z, act),
                           sgx_act6(k.s.w * v.w + k.t.w, act));
    }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        const float4 a = act4(in.a, k), b = act4(in.b, k), e = act4(in.c, k), d = act4(in.d, k);
        sgx_st4(y + r * y_ld + c, make_float4(0.25f * ((a.x + b.x) + (e.x + d.x)), 0.25f * ((a.y + b.y) + (e.y + d.y)), 0.25f * ((a.z + b.z) + (e.z + d.z)),
                                              0.25f * ((a.w + b.w) + (e.w + d.w))));
    }
};
extern "C" int32_t sgx_bn_act_avgpool2_fwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* x, int64_t x_ld, const float* scale, const float* shift,
                                           int32_t act, float* y, int64_t y_ld, void* stream) {
    SGX_CHECK_ARG(x && scale && shift && y, "bn_act_avgpool2_fwd: null pointer");
    SGX_CHECK_ACT4(act, "bn_act_avgpool2_fwd");
    SW_CHECK_VEC(C, SW_LD4(x_ld) && SW_LD4(y_ld) && SW_ALIGNED(x) && SW_ALIGNED(scale) && SW_ALIGNED(shift) && SW_ALIGNED(y), "bn_act_avgpool2_fwd");
    BnActAvgpool2F f{x, x_ld, scale, shift, y, y_ld, {}, act};
    int32_t rc = pool_geom(N, H, W, true, &f.g, "bn_act_avgpool2_fwd");
    if (rc) return rc;
    // (a pooled row is four source pixels: the row blocks of a sweep over the source map, 64 source pixels per workgroup - with 64 pooled
    // rows the 14 x 14 x 1024 map of densenet121 ran on 196 workgroups, fewer than the chip has CUs)
    const long Mo = (long)N * f.g.Ho * f.g.Wo;
    return run_sweep<BnActAvgpool2F, 0, 2>(f, Mo, C, nullptr, stream, "bn_act_avgpool2_fwd", sgx_stats_blocks(4 * Mo));
}

// backward: a row is one FULL-RESOLUTION pixel, its upstream gradient a quarter of the pooled gradient of its window (zero outside every
// window) - from there on the two sweeps ARE the BatchNorm backward's: the reduce leaves sgx_bn_bwd_reduce's partial rows
// ([2][sgx_stats_blocks(N*H*W)][C]), the apply writes every pixel of dx.
__device__ __forceinline__ void pool_bwd_load(const PoolGeom& g, const float* dz, long dz_ld, const float* x, long x_ld, long r, int c, float4& d, float4& v) {
    const int t = sgx_fdiv((int)r, g.dW), w = (int)r - t * g.W, n = sgx_fdiv(t, g.dH), h = t - n * g.H;
    const int ho = h >> 1, wo = w >> 1;
    v = sgx_ld4(x + r * x_ld + c);
    d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ho < g.Ho && wo < g.Wo) {
        const float4 u = sgx_ld4(dz + (((long)n * g.Ho + ho) * g.Wo + wo) * dz_ld + c);
        d = make_float4(0.25f * u.x, 0.25f * u.y, 0.25f * u.z, 0.25f * u.w);
    }
}
struct BnActAvgpool2BwdReduceF : BnBwdReduceF {  // dy / dy_ld: the pooled gradient dz
    PoolGeom g;
    __device__ In load(long r, int c) const {
        In in;
        pool_bwd_load(g, dy, dy_ld, x, x_ld, r, c, in.d, in.v);
        return in;
    }
};
struct BnActAvgpool2BwdApplyF : BnBwdApplyF {
    PoolGeom g;
    __device__ In load(long r, int c) const {
        In in;
        pool_bwd_load(g, dy, dy_ld, x, x_ld, r, c, in.d, in.v);
        return in;
    }
};
extern "C" int32_t sgx_bn_act_avgpool2_bwd_reduce(int32_t N, int32_t H, int32_t W, int32_t C, const float* dz, int64_t dz_ld, const float* x, int64_t x_ld,
                                                  const float* scale, const float* shift, const float* save_mean, int32_t act, float* partials, void* stream) {
    SGX_CHECK_ARG(dz && x && scale && shift && save_mean && partials, "bn_act_avgpool2_bwd_reduce: null pointer");
    SGX_CHECK_ACT4(act, "bn_act_avgpool2_bwd_reduce");
    SW_CHECK_VEC(C, SW_LD4(dz_ld) && SW_LD4(x_ld) && SW_ALIGNED(dz) && SW_ALIGNED(x) && SW_ALIGNED(scale) && SW_ALIGNED(shift) && SW_ALIGNED(save_mean) && SW_ALIGNED(partials),
                 "bn_act_avgpool2_bwd_reduce");
    BnActAvgpool2BwdReduceF f{{dz, dz_ld, x, x_ld, scale, shift, save_mean, act}, {}};
    int32_t rc = pool_geom(N, H, W, false, &f.g, "bn_act_avgpool2_bwd_reduce");
    if (rc) return rc;
    return run_sweep<BnActAvgpool2BwdReduceF, 2, 4>(f, (long)N * H * W, C, partials, stream, "bn_act_avgpool2_bwd_reduce");
}
extern "C" int32_t sgx_bn_act_avgpool2_bwd_apply(int32_t N, int32_t H, int32_t W, int32_t C, const float* dz, int64_t dz_ld, const float* x, int64_t x_ld,
                                                 const float* scale, const float* shift, const float* coef, int32_t act, float* dx, int64_t dx_ld, void* stream) {
    SGX_CHECK_ARG(dz && x && scale && shift && coef && dx, "bn_act_avgpool2_bwd_apply: null pointer");
    SGX_CHECK_ACT4(act, "bn_act_avgpool2_bwd_apply");
    SW_CHECK_VEC(C, SW_LD4(dz_ld) && SW_LD4(x_ld) && SW_LD4(dx_ld) && SW_ALIGNED(dz) && SW_ALIGNED(x) && SW_ALIGNED(scale) && SW_ALIGNED(shift) && SW_ALIGNED(coef) &&
                        SW_ALIGNED(dx),
                 "bn_act_avgpool2_bwd_apply");
    BnActAvgpool2BwdApplyF f{{dz, dz_ld, x, x_ld, scale, shift, coef, C, dx, dx_ld, nullptr, 0, act}, {}};
    int32_t rc = pool_geom(N, H, W, false, &f.g, "bn_act_avgpool2_bwd_apply");
    if (rc) return rc;
    return run_sweep<BnActAvgpool2BwdApplyF, 0, 4>(f, (long)N * H * W, C, nullptr, stream, "bn_act_avgpool2_bwd_apply");
}
