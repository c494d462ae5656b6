// Squeeze-excitation gates and nearest x2 up-sampling of PP-YOLOE (HBM-bound, no MFMA).
//   EffectiveSEBlock  modules/se_blocks.py:29-42           y = x * hardsigmoid(project(mean_hw x))
//   ESEAttn           pp_yolo_e/pp_yolo_head.py:79-93      conv(feat * sigmoid(fc(avg_feat)))
//   F.interpolate(x2, nearest)  pp_yolo_e/pan.py:170
// and, further down, the fused BatchNorm / gate / activation sweeps of MobileNetV3 (gate, then activation) and EfficientNet (activation,
// then gate; drop-connect).
// Data layout: NHWC views with explicit pixel / image strides (channel slices of concat buffers are read and written in place);
// per-image vectors ([N][C] means, gate pre-activations, their gradients) are contiguous.
// Every per-image reduction ([N][C] sums over an image's pixels: plain and product sums, the gate gradients, the means of the activated
// map) is ONE skeleton, image_reduce_kernel, with a functor for the per-pixel term, and one finalize kernel.  Two stages, deterministic:
// a (image, pixel chunk, channel strip) grid leaves fp32 partial rows, the finalize kernel adds them in fp64 in chunk order.  No atomics.
// Every row x channel sweep (the fused forward and data-gradient passes) is a functor on bn.hip's skeleton (sgx_sweep.h).
#include <initializer_list>

#include "sgx_common.h"
#include "sgx_sweep.h"

#define SE_THREADS 256
#define SE_MAXCG 64      // float4 channel groups per workgroup strip
#define SE_CHUNK_ROWS 512  // pixels per chunk: 160x160 maps -> 50 chunks per image, 32 images -> 1600 workgroups per strip

// every kernel here moves float4: addresses (NULL passes: an absent operand) and strides must be multiples of 16 bytes (SW_ALIGNED / SW_LD4)
static bool se_vec(std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
    bool ok = true;
    for (const void* p : ptrs) ok = ok && SW_ALIGNED(p);
    for (int64_t ld : lds) ok = ok && SW_LD4(ld);
    return ok;
}

__device__ __forceinline__ float se_gate(float p, int gate) {
    if (gate == SGX_GATE_HARDSIGMOID) return fminf(fmaxf(p * (1.f / 6.f) + 0.5f, 0.f), 1.f);
    if (gate == SGX_GATE_SIGMOID) return 1.f / (1.f + expf(-p));
    return p;
}
__device__ __forceinline__ float se_gate_grad(float p, int gate) {
    if (gate == SGX_GATE_HARDSIGMOID) return (p > -3.f && p < 3.f) ? (1.f / 6.f) : 0.f;
    if (gate == SGX_GATE_SIGMOID) {
        float s = 1.f / (1.f + expf(-p));
        return s * (1.f - s);
    }
    return 1.f;
}

// Geometry of a per-image reduction: a workgroup is CG float4 channel groups x RL row lanes and owns `rows` pixels (one chunk) of one image
struct ImgGeom {
    int N, HW, C, C4, CG, RL, rows, chunks, ctiles;
};
static int se_strip(int C) { return C < 4 ? 1 : C / 4 < SE_MAXCG ? C / 4 : SE_MAXCG; }  // (>= 1: the workspace queries take any C)
static int se_row_lanes(int C) { return SE_THREADS / se_strip(C); }
static ImgGeom img_geom(int N, int HW, int C, int rows_per_chunk) {
    ImgGeom g;
    g.N = N; g.HW = HW; g.C = C; g.C4 = C / 4;
    g.CG = se_strip(C);
    g.RL = SE_THREADS / g.CG;
    g.rows = rows_per_chunk;
    g.chunks = (int)(((long)HW + g.rows - 1) / g.rows);
    g.ctiles = (g.C4 + g.CG - 1) / g.CG;
    return g;
}
static int64_t img_workspace(const ImgGeom& g) { return (int64_t)g.N * g.chunks * g.C * (int64_t)sizeof(float) + 256; }

// The per-image reduction skeleton.  F: struct with  Cst consts(int img, int c)  (what a lane keeps for its image and its four channels -
// the BatchNorm constants, the gate, the image's base pointers - loaded ONCE, ahead of the pixel loop),  In load(int p, int c, const Cst&)
// (all global loads of pixel p, channels c..c+3) and  void add(const In&, const Cst&, float4& q)  (the arithmetic: q += the pixel's
// term).  ROWS pixels of a lane are in flight: their loads are issued before the first add.  The order of summation is fixed: a lane
// adds its pixels (p0 + rl, + RL, ...) in ascending order into one fp32 q, row lane 0 then adds the lanes' q in ascending lane order
// in fp32 (not the fp64 of sweep_kernel) and stores one row of partials [N][chunks][C].
template <typename F, int ROWS>
__global__ __launch_bounds__(SE_THREADS) void image_reduce_kernel(F f, ImgGeom g, float* partials) {
    __shared__ float4 red[SE_THREADS];
    const int tid = threadIdx.x;
    const int cg = tid % g.CG, rl = tid / g.CG;
    const int c4 = blockIdx.y * g.CG + cg;
    const int chunk = blockIdx.x % g.chunks, img = blockIdx.x / g.chunks;
    const bool live = (rl < g.RL) && (c4 < g.C4);
    const int c = c4 * 4;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        int p0 = chunk * g.rows, p1 = p0 + g.rows;
        if (p1 > g.HW) p1 = g.HW;
        const typename F::Cst k = f.consts(img, c);
        const int st = g.RL;
        int p = p0 + rl;
        if constexpr (ROWS > 1) {
            for (; p + (ROWS - 1) * st < p1; p += ROWS * st) {
                typename F::In in[ROWS];
#pragma unroll
                for (int u = 0; u < ROWS; ++u) in[u] = f.load(p + u * st, c, k);
#pragma unroll
                for (int u = 0; u < ROWS; ++u) f.add(in[u], k, q);
            }
        }
        for (; p < p1; p += st) {
            const typename F::In i0 = f.load(p, c, k);
            f.add(i0, k, q);
        }
    }
    red[tid] = q;
    __syncthreads();
    if (live && rl == 0) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < g.RL; ++k) {
            float4 a = red[k * g.CG + cg];
            s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        }
        sgx_st4(partials + ((long)img * g.chunks + chunk) * g.C + c, s);
    }
}
// out[n][c] = scale * f'(pre[n][c]) * the fp64 sum of the image's partial rows (pre NULL: no gate factor)
__global__ void image_colsum_finalize_kernel(int N, int chunks, int C, const float* partials, float scale, const float* pre, int gate,
                                             float* out) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * C) return;
    int c = (int)(i % C), img = (int)(i / C);
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += (double)partials[((long)img * chunks + k) * C + c];
    float r = (float)(s * (double)scale);
    if (pre) r *= se_gate_grad(pre[i], gate);
    out[i] = r;
}
// both stages: partial rows into ws (img_workspace(g) bytes), then out
template <typename F, int ROWS>
static int32_t image_reduce_run(const F& f, const ImgGeom& g, void* ws, float scale, const float* pre, int gate, float* out, void* stream, const char* what) {
    SGX_LAUNCH((image_reduce_kernel<F, ROWS>), dim3((unsigned)((long)g.N * g.chunks), g.ctiles), dim3(SE_THREADS), 0, stream, f, g, (float*)ws);
    SGX_CHECK_LAUNCH(what);
    SGX_LAUNCH(image_colsum_finalize_kernel, dim3(sgx_cdiv((long)g.N * g.C, 256)), dim3(256), 0, stream, g.N, g.chunks, g.C, (const float*)ws, scale, pre, gate, out);
    SGX_CHECK_LAUNCH(what);
    return SGX_OK;
}

// sum_p u (v NULL) or sum_p u * v over NHWC views with explicit pixel / image strides
struct ImageColsumF {
    const float* u; long u_ld_pix, u_ld_img; const float* v; long v_ld_pix, v_ld_img;
    struct Cst { const float* ub; const float* vb; };
    __device__ Cst consts(int img, int) const { return Cst{u + (long)img * u_ld_img, v ? v + (long)img * v_ld_img : nullptr}; }
    struct In { float4 a, b; };
    __device__ In load(int p, int c, const Cst& k) const {
        return In{sgx_ld4(k.ub + (long)p * u_ld_pix + c), k.vb ? sgx_ld4(k.vb + (long)p * v_ld_pix + c) : make_float4(0.f, 0.f, 0.f, 0.f)};
    }
    __device__ void add(const In& in, const Cst& k, float4& q) const {
        const float4 a = in.a, b = in.b;
        if (k.vb) {
            q.x += a.x * b.x; q.y += a.y * b.y; q.z += a.z * b.z; q.w += a.w * b.w;
        } else {
            q.x += a.x; q.y += a.y; q.z += a.z; q.w += a.w;
        }
    }
};
extern "C" int64_t sgx_image_colsum_workspace(int32_t N, int32_t HW, int32_t C) { return img_workspace(img_geom(N, HW, C, SE_CHUNK_ROWS)); }
extern "C" int32_t sgx_image_colsum(int32_t N, int32_t HW, int32_t C, const float* u, int64_t u_ld_pix, int64_t u_ld_img, const float* v,
                                    int64_t v_ld_pix, int64_t v_ld_img, float scale, const float* pre, int32_t gate, float* out, void* ws,
                                    int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(u && out && ws && N > 0 && HW > 0 && C > 0 && C % 4 == 0, "image_colsum: bad args (C=%d)", C);
    SGX_CHECK_ARG(ws_bytes >= sgx_image_colsum_workspace(N, HW, C), "image_colsum: workspace too small");
    SGX_CHECK_ARG(se_vec({u, v, pre, out, ws}, {u_ld_pix, u_ld_img, v ? v_ld_pix : 0, v ? v_ld_img : 0}),
                  "image_colsum: strides and addresses must be multiples of 16 bytes");
    ImageColsumF f{u, (long)u_ld_pix, (long)u_ld_img, v, (long)v_ld_pix, (long)v_ld_img};
    return image_reduce_run<ImageColsumF, 1>(f, img_geom(N, HW, C, SE_CHUNK_ROWS), ws, scale, pre, gate, out, stream, "image_colsum");
}

// One thread: one float4 channel group of one pixel; the gate / bias of (image, channel group) come from L2-resident [N][C] vectors.
__global__ __launch_bounds__(256) void channel_gate_kernel(int N, int HW, int C, const float* x, long x_ld_pix, long x_ld_img, const float* pre,
                                                           int gate, const float* bias, float bias_scale, float* y, long y_ld_pix,
                                                           long y_ld_img, int accumulate) {
    const int C4 = C / 4;
    const long n = (long)N * HW * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        long t = i / C4;
        int p = (int)(t % HW), img = (int)(t / HW);
        float4 v = sgx_ld4(x + (long)img * x_ld_img + (long)p * x_ld_pix + c);
        float4 w = sgx_ld4(pre + (long)img * C + c);
        float4 o = make_float4(v.x * se_gate(w.x, gate), v.y * se_gate(w.y, gate), v.z * se_gate(w.z, gate), v.w * se_gate(w.w, gate));
        if (bias) {
            float4 b = sgx_ld4(bias + (long)img * C + c);
            o.x += bias_scale * b.x; o.y += bias_scale * b.y; o.z += bias_scale * b.z; o.w += bias_scale * b.w;
        }
        float* yp = y + (long)img * y_ld_img + (long)p * y_ld_pix + c;
        if (accumulate) {
            float4 a = sgx_ld4(yp);
            o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
        }
        sgx_st4(yp, o);
    }
}
extern "C" int32_t sgx_channel_gate(int32_t N, int32_t HW, int32_t C, const float* x, int64_t x_ld_pix, int64_t x_ld_img, const float* pre,
                                    int32_t gate, const float* bias, float bias_scale, float* y, int64_t y_ld_pix, int64_t y_ld_img,
                                    int32_t accumulate, void* stream) {
    SGX_CHECK_ARG(x && pre && y && N > 0 && HW > 0 && C > 0 && C % 4 == 0, "channel_gate: bad args (C=%d)", C);
    SGX_CHECK_ARG(gate >= SGX_GATE_NONE && gate <= SGX_GATE_SIGMOID, "channel_gate: unknown gate %d", gate);
    SGX_CHECK_ARG(SW_LD4(x_ld_pix) && SW_LD4(x_ld_img) && SW_LD4(y_ld_pix) && SW_LD4(y_ld_img) && SW_ALIGNED(x) && SW_ALIGNED(y) && SW_ALIGNED(pre) && SW_ALIGNED(bias),
                  "channel_gate: strides and addresses must be multiples of 16 bytes");
    long n = (long)N * HW * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(channel_gate_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, HW, C, x, (long)x_ld_pix,
               (long)x_ld_img, pre, gate, bias, bias_scale, y, (long)y_ld_pix, (long)y_ld_img, accumulate);
    SGX_CHECK_LAUNCH("channel_gate");
    return SGX_OK;
}

// One thread: one float4 channel group of one INPUT pixel (read once, written to its 2x2 output block / gathered from it).
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(int N, int H, int W, int C, const float* x, long x_ld_pix, long x_ld_img, float* y,
                                                             long y_ld_pix, long y_ld_img) {
    const int C4 = C / 4;
    const long n = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        long t = i / C4;
        int w = (int)(t % W);
        t /= W;
        int h = (int)(t % H), img = (int)(t / H);
        float4 v = sgx_ld4(x + (long)img * x_ld_img + ((long)h * W + w) * x_ld_pix + c);
        float* yb = y + (long)img * y_ld_img + c;
        const long W2 = 2L * W;
        sgx_st4(yb + ((2L * h) * W2 + 2 * w) * y_ld_pix, v);
        sgx_st4(yb + ((2L * h) * W2 + 2 * w + 1) * y_ld_pix, v);
        sgx_st4(yb + ((2L * h + 1) * W2 + 2 * w) * y_ld_pix, v);
        sgx_st4(yb + ((2L * h + 1) * W2 + 2 * w + 1) * y_ld_pix, v);
    }
}
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(int N, int H, int W, int C, const float* dy, long dy_ld_pix, long dy_ld_img,
                                                             float* dx, long dx_ld_pix, long dx_ld_img, int accumulate) {
    const int C4 = C / 4;
    const long n = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        long t = i / C4;
        int w = (int)(t % W);
        t /= W;
        int h = (int)(t % H), img = (int)(t / H);
        const float* db = dy + (long)img * dy_ld_img + c;
        const long W2 = 2L * W;
        float4 a = sgx_ld4(db + ((2L * h) * W2 + 2 * w) * dy_ld_pix), b = sgx_ld4(db + ((2L * h) * W2 + 2 * w + 1) * dy_ld_pix);
        float4 e = sgx_ld4(db + ((2L * h + 1) * W2 + 2 * w) * dy_ld_pix), f = sgx_ld4(db + ((2L * h + 1) * W2 + 2 * w + 1) * dy_ld_pix);
        float4 o = make_float4((a.x + b.x) + (e.x + f.x), (a.y + b.y) + (e.y + f.y), (a.z + b.z) + (e.z + f.z), (a.w + b.w) + (e.w + f.w));
        float* xp = dx + (long)img * dx_ld_img + ((long)h * W + w) * dx_ld_pix + c;
        if (accumulate) {
            float4 u = sgx_ld4(xp);
            o.x += u.x; o.y += u.y; o.z += u.z; o.w += u.w;
        }
        sgx_st4(xp, o);
    }
}
extern "C" int32_t sgx_upsample2x_fwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* x, int64_t x_ld_pix, int64_t x_ld_img, float* y,
                                      int64_t y_ld_pix, int64_t y_ld_img, void* stream) {
    SGX_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "upsample2x_fwd: bad args (C=%d)", C);
    SGX_CHECK_ARG(SW_LD4(x_ld_pix) && SW_LD4(x_ld_img) && SW_LD4(y_ld_pix) && SW_LD4(y_ld_img) && SW_ALIGNED(x) && SW_ALIGNED(y),
                  "upsample2x_fwd: strides and addresses must be multiples of 16 bytes");
    long n = (long)N * H * W * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(upsample2x_fwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, H, W, C, x, (long)x_ld_pix,
               (long)x_ld_img, y, (long)y_ld_pix, (long)y_ld_img);
    SGX_CHECK_LAUNCH("upsample2x_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_upsample2x_bwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* dy, int64_t dy_ld_pix, int64_t dy_ld_img,
                                      float* dx, int64_t dx_ld_pix, int64_t dx_ld_img, int32_t accumulate, void* stream) {
    SGX_CHECK_ARG(dy && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "upsample2x_bwd: bad args (C=%d)", C);
    SGX_CHECK_ARG(SW_LD4(dy_ld_pix) && SW_LD4(dy_ld_img) && SW_LD4(dx_ld_pix) && SW_LD4(dx_ld_img) && SW_ALIGNED(dy) && SW_ALIGNED(dx),
                  "upsample2x_bwd: strides and addresses must be multiples of 16 bytes");
    long n = (long)N * H * W * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(upsample2x_bwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, H, W, C, dy, (long)dy_ld_pix,
               (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate);
    SGX_CHECK_LAUNCH("upsample2x_bwd");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm -> squeeze-excitation gate -> activation as fused sweeps (MobileNetV3's expanded block: dw -> BN -> SE -> act,
// classification_models/mobilenetv3.py:103-108).  z = scale[c] * x + shift[c] (NULL scale / shift: z = x, the folded eval form),
// s = f(pre[n][c]), y = act(s * z).  The per-image means the SE layer needs are affine in the means of x (sgx_image_colsum on the raw
// convolution output, mapped through scale / shift on the [N,C] matrix): z is never stored.  Rows are pixels, uniformly strided across
// images (row r belongs to image r / HW).  The data-gradient sweep runs on bn.hip's skeleton: its reduce rows are sgx_bn_bwd_reduce's.
struct GateZ {
    float4 s, t;
    int on;
    __device__ float4 z(const float4& v) const { return on ? make_float4(s.x * v.x + t.x, s.y * v.y + t.y, s.z * v.z + t.z, s.w * v.w + t.w) : v; }
};
__device__ __forceinline__ GateZ gate_z(const float* scale, const float* shift, int c) {
    const float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    return GateZ{scale ? sgx_ld4(scale + c) : o, scale ? sgx_ld4(shift + c) : o, scale ? 1 : 0};
}
__device__ __forceinline__ float4 se_gate4(const float4& p, int gate) { return make_float4(se_gate(p.x, gate), se_gate(p.y, gate), se_gate(p.z, gate), se_gate(p.w, gate)); }
// gv = dy * act'(s * z)
__device__ __forceinline__ float4 gate_gv(const float4& d, const float4& z, const float4& s, int act) {
    return make_float4(d.x * sgx_act6_grad(s.x * z.x, act), d.y * sgx_act6_grad(s.y * z.y, act), d.z * sgx_act6_grad(s.z * z.z, act),
                       d.w * sgx_act6_grad(s.w * z.w, act));
}
__device__ __forceinline__ float4 act4(const float4& z, int act) { return make_float4(sgx_act6(z.x, act), sgx_act6(z.y, act), sgx_act6(z.z, act), sgx_act6(z.w, act)); }
__device__ __forceinline__ float4 act4_grad(const float4& z, int act) {
    return make_float4(sgx_act6_grad(z.x, act), sgx_act6_grad(z.y, act), sgx_act6_grad(z.z, act), sgx_act6_grad(z.w, act));
}

// The argument check of every entry point below, before any launch: `need` may not be NULL, `opt` may; all of them, scale, shift and
// the strides `lds` are float4-aligned.  (An entry point without a gate or an activation passes SGX_GATE_NONE / SGX_ACT_NONE.)
static int32_t se_check(const char* what, int N, int HW, int C, int gate, int act, const float* scale, const float* shift,
                        std::initializer_list<const void*> need, std::initializer_list<const void*> opt, std::initializer_list<int64_t> lds) {
    bool have = true;
    for (const void* p : need) have = have && p;
    SGX_CHECK_ARG(have, "%s: null pointer", what);
    SGX_CHECK_ARG(N > 0 && HW > 0 && C > 0 && C % 4 == 0 && (long)N * HW < 0x7fffffffL, "%s: bad dims N=%d HW=%d C=%d", what, N, HW, C);
    SGX_CHECK_ARG(gate >= SGX_GATE_NONE && gate <= SGX_GATE_SIGMOID, "%s: unknown gate %d", what, gate);
    SGX_CHECK_ACT4(act, what);
    SGX_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift go together", what);
    SGX_CHECK_ARG(se_vec(need, lds) && se_vec(opt, {}) && se_vec({scale, shift}, {}), "%s: strides and addresses must be multiples of 16 bytes", what);
    return SGX_OK;
}
#define SE_CHECK(...)                                        \
    do {                                                     \
        if (int32_t e__ = se_check(__VA_ARGS__)) return e__; \
    } while (0)

// What the gate sweeps share: a row's x and its image's pre, the BatchNorm constants of the lane's channels
struct GateSweepF {
    const float* x; long x_ld; const float* scale; const float* shift; const float* pre; int gate; sgx_fastdiv hw; int C;
    struct In { float4 v, p; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(x + r * x_ld + c), sgx_ld4(pre + (long)sgx_fdiv((int)r, hw) * C + c)}; }
    typedef GateZ Cst;
    __device__ Cst consts(int c) const { return gate_z(scale, shift, c); }
};
struct BnGateActFwdF : GateSweepF {
    float* y; long y_ld; int act;
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        const float4 z = k.z(in.v), s = se_gate4(in.p, gate);
        sgx_st4(y + r * y_ld + c, make_float4(sgx_act6(s.x * z.x, act), sgx_act6(s.y * z.y, act), sgx_act6(s.z * z.z, act), sgx_act6(s.w * z.w, act)));
    }
};
extern "C" int32_t sgx_bn_gate_act_fwd(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* pre, int32_t gate,
                                       float* y, int64_t y_ld, int32_t N, int32_t HW, int32_t C, int32_t act, void* stream) {
    SE_CHECK("bn_gate_act_fwd", N, HW, C, gate, act, scale, shift, {x, pre, y}, {}, {x_ld, y_ld});
    BnGateActFwdF f{{x, x_ld, scale, shift, pre, gate, sgx_make_fastdiv(HW), C}, y, y_ld, act};
    return run_sweep<BnGateActFwdF, 0, 4>(f, (long)N * HW, C, nullptr, stream, "bn_gate_act_fwd");
}

// What the per-image reductions over (dy, x) share.  A lane keeps the BatchNorm constants, the image's gate s and the image's first rows
// (dy / pre NULL: a sum that does not read them)
struct GateImgF {
    const float* dy; long dy_ld; const float* x; long x_ld; const float* scale; const float* shift; const float* pre; int gate; int act; int HW; int C;
    struct In { float4 v, d; };
    struct Cst { GateZ k; float4 s; const float* xb; const float* db; };
    __device__ Cst consts(int img, int c) const {
        return Cst{gate_z(scale, shift, c), pre ? se_gate4(sgx_ld4(pre + (long)img * C + c), gate) : make_float4(0.f, 0.f, 0.f, 0.f), x + (long)img * HW * x_ld,
                   dy ? dy + (long)img * HW * dy_ld : nullptr};
    }
};
// d pre[n][c] = f'(pre) * sum over the image's pixels of gv * z
struct BnGateActBwdGateF : GateImgF {
    __device__ In load(int p, int c, const Cst& k) const { return In{sgx_ld4(k.xb + (long)p * x_ld + c), sgx_ld4(k.db + (long)p * dy_ld + c)}; }
    __device__ void add(const In& in, const Cst& k, float4& q) const {
        const float4 z = k.k.z(in.v);
        const float4 gv = gate_gv(in.d, z, k.s, act);
        q.x += gv.x * z.x; q.y += gv.y * z.y; q.z += gv.z * z.z; q.w += gv.w * z.w;
    }
};
extern "C" int64_t sgx_bn_gate_act_bwd_gate_workspace(int32_t N, int32_t HW, int32_t C) { return sgx_image_colsum_workspace(N, HW, C); }
extern "C" int32_t sgx_bn_gate_act_bwd_gate(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* scale, const float* shift,
                                            const float* pre, int32_t gate, int32_t act, float* dpre, int32_t N, int32_t HW, int32_t C, void* ws,
                                            int64_t ws_bytes, void* stream) {
    SE_CHECK("bn_gate_act_bwd_gate", N, HW, C, gate, act, scale, shift, {dy, x, pre, dpre, ws}, {}, {dy_ld, x_ld});
    if (ws_bytes < sgx_bn_gate_act_bwd_gate_workspace(N, HW, C)) SGX_FAIL(SGX_ERR_WORKSPACE, "bn_gate_act_bwd_gate: workspace too small (sgx_bn_gate_act_bwd_gate_workspace)");
    BnGateActBwdGateF f{{dy, dy_ld, x, x_ld, scale, shift, pre, gate, act, HW, C}};
    return image_reduce_run<BnGateActBwdGateF, 1>(f, img_geom(N, HW, C, SE_CHUNK_ROWS), ws, 1.f, pre, gate, dpre, stream, "bn_gate_act_bwd_gate");
}

// ---------------------------------------------------------------------------------------------
// BatchNorm -> activation -> squeeze-excitation gate as fused sweeps (EfficientNet's MBConv block: dw -> BN -> SiLU -> SE,
// classification_models/efficientnet.py:370-380).  z and s as above, a = act(z), y = s * a.  The per-image means the SE layer needs are
// those of a - not affine in anything cheaper - so they take a pass of their own (_mean: one read of x, a is never stored); the gate
// multiplies the activated value, so act'(z) does not see it.  Same row convention, same reduce rows as the family above.

// Geometry of the two reductions over the activated map.  image_colsum's 512-pixel chunks leave 128 workgroups for a 64 x 28 x 28 x 240
// map, each lane walking ~200 rows - with an exponential and a division per element that is a serial ALU chain on a quarter-filled chip.
// Here a chunk is 16 rows per row lane (RL * 16 pixels: 512 at 32 channels, 64 from 256 channels up), a function of C alone, so the
// partial rows [N][chunks][C] and the fp64 sums over them do not depend on anything but the shape.
#define ACT_LANE_ROWS 16
static ImgGeom act_geom(int N, int HW, int C) { return img_geom(N, HW, C, se_row_lanes(C) * ACT_LANE_ROWS); }
static int64_t act_workspace(int32_t N, int32_t HW, int32_t C) {
    if (N <= 0 || HW <= 0 || C < 4) return 256;
    return img_workspace(act_geom(N, HW, C));
}
// sum_p act(z) (DY false) or sum_p dy * act(z), four rows of a lane in flight
template <bool DY>
struct BnActSumF : GateImgF {
    __device__ In load(int p, int c, const Cst& k) const {
        return In{sgx_ld4(k.xb + (long)p * x_ld + c), DY ? sgx_ld4(k.db + (long)p * dy_ld + c) : make_float4(0.f, 0.f, 0.f, 0.f)};
    }
    __device__ void add(const In& in, const Cst& k, float4& q) const {
        const float4 a = act4(k.k.z(in.v), act), d = in.d;
        if (DY) {
            q.x += d.x * a.x; q.y += d.y * a.y; q.z += d.z * a.z; q.w += d.w * a.w;
        } else {
            q.x += a.x; q.y += a.y; q.z += a.z; q.w += a.w;
        }
    }
};
extern "C" int64_t sgx_bn_act_gate_mean_workspace(int32_t N, int32_t HW, int32_t C) { return act_workspace(N, HW, C); }
extern "C" int32_t sgx_bn_act_gate_mean(const float* x, int64_t x_ld, const float* scale, const float* shift, int32_t act, float* out, int32_t N, int32_t HW,
                                        int32_t C, void* ws, int64_t ws_bytes, void* stream) {
    SE_CHECK("bn_act_gate_mean", N, HW, C, SGX_GATE_NONE, act, scale, shift, {x, out, ws}, {}, {x_ld});
    if (ws_bytes < sgx_bn_act_gate_mean_workspace(N, HW, C)) SGX_FAIL(SGX_ERR_WORKSPACE, "bn_act_gate_mean: workspace too small (sgx_bn_act_gate_mean_workspace)");
    BnActSumF<false> f{{nullptr, 0L, x, x_ld, scale, shift, nullptr, SGX_GATE_NONE, act, HW, C}};
    return image_reduce_run<BnActSumF<false>, 4>(f, act_geom(N, HW, C), ws, 1.f / (float)HW, nullptr, SGX_GATE_NONE, out, stream, "bn_act_gate_mean");
}

struct BnActGateFwdF : GateSweepF {
    float* y; long y_ld; int act;
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        const float4 a = act4(k.z(in.v), act), s = se_gate4(in.p, gate);
        sgx_st4(y + r * y_ld + c, make_float4(s.x * a.x, s.y * a.y, s.z * a.z, s.w * a.w));
    }
};
extern "C" int32_t sgx_bn_act_gate_fwd(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* pre, int32_t gate,
                                       float* y, int64_t y_ld, int32_t N, int32_t HW, int32_t C, int32_t act, void* stream) {
    SE_CHECK("bn_act_gate_fwd", N, HW, C, gate, act, scale, shift, {x, pre, y}, {}, {x_ld, y_ld});
    BnActGateFwdF f{{x, x_ld, scale, shift, pre, gate, sgx_make_fastdiv(HW), C}, y, y_ld, act};
    return run_sweep<BnActGateFwdF, 0, 4>(f, (long)N * HW, C, nullptr, stream, "bn_act_gate_fwd");
}

// d pre[n][c] = f'(pre) * sum over the image's pixels of dy * act(z)
extern "C" int64_t sgx_bn_act_gate_bwd_gate_workspace(int32_t N, int32_t HW, int32_t C) { return act_workspace(N, HW, C); }
extern "C" int32_t sgx_bn_act_gate_bwd_gate(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* scale, const float* shift,
                                            const float* pre, int32_t gate, int32_t act, float* dpre, int32_t N, int32_t HW, int32_t C, void* ws,
                                            int64_t ws_bytes, void* stream) {
    SE_CHECK("bn_act_gate_bwd_gate", N, HW, C, gate, act, scale, shift, {dy, x, pre, dpre, ws}, {}, {dy_ld, x_ld});
    if (ws_bytes < sgx_bn_act_gate_bwd_gate_workspace(N, HW, C)) SGX_FAIL(SGX_ERR_WORKSPACE, "bn_act_gate_bwd_gate: workspace too small (sgx_bn_act_gate_bwd_gate_workspace)");
    BnActSumF<true> f{{dy, dy_ld, x, x_ld, scale, shift, nullptr, SGX_GATE_NONE, act, HW, C}};
    return image_reduce_run<BnActSumF<true>, 4>(f, act_geom(N, HW, C), ws, 1.f, pre, gate, dpre, stream, "bn_act_gate_bwd_gate");
}

// The data gradient of either order, stored to dz; with `partials` also the rows sum dz, sum dz * (x - save_mean) of the BatchNorm backward.
//   gate, then activation (ACT_FIRST false):  dz = gv * s + dmean[n][c] / HW
//   activation, then gate:                    dz = (dy * s + dmean[n][c] / HW) * act'(z)
template <bool ACT_FIRST>
struct BnGateBwdDataF : GateSweepF {
    const float* dy; long dy_ld; int act; const float* dmean; float inv_hw; float* dz; long dz_ld; const float* mean;
    struct In { float4 d, v, p, m; };
    __device__ In load(long r, int c) const {
        const long o = (long)sgx_fdiv((int)r, hw) * C + c;
        return In{sgx_ld4(dy + r * dy_ld + c), sgx_ld4(x + r * x_ld + c), sgx_ld4(pre + o), dmean ? sgx_ld4(dmean + o) : make_float4(0.f, 0.f, 0.f, 0.f)};
    }
    struct Cst { GateZ k; float4 mu; };
    __device__ Cst consts(int c) const { return Cst{gate_z(scale, shift, c), mean ? sgx_ld4(mean + c) : make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ float4 grad_gate_act(const float4& gv, const float4& s, const float4& m) const {
        return make_float4(gv.x * s.x + m.x * inv_hw, gv.y * s.y + m.y * inv_hw, gv.z * s.z + m.z * inv_hw, gv.w * s.w + m.w * inv_hw);
    }
    // (dz ends in a product: contracted into the row sums below it would enter them unrounded, and the rows would not be the ones
    // sgx_bn_bwd_reduce forms from the stored dz)
    __device__ float4 grad_act_gate(const float4& d, const float4& s, const float4& m, const float4& ga) const {
#pragma clang fp contract(off)
        return make_float4((d.x * s.x + m.x * inv_hw) * ga.x, (d.y * s.y + m.y * inv_hw) * ga.y, (d.z * s.z + m.z * inv_hw) * ga.z, (d.w * s.w + m.w * inv_hw) * ga.w);
    }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&q)[2]) const {
        const float4 v = in.v, mu = k.mu, z = k.k.z(v), s = se_gate4(in.p, gate);
        const float4 o = ACT_FIRST ? grad_act_gate(in.d, s, in.m, act4_grad(z, act)) : grad_gate_act(gate_gv(in.d, z, s, act), s, in.m);
        sgx_st4(dz + r * dz_ld + c, o);
        q[0].x += o.x; q[0].y += o.y; q[0].z += o.z; q[0].w += o.w;
        q[1].x += o.x * (v.x - mu.x); q[1].y += o.y * (v.y - mu.y); q[1].z += o.z * (v.z - mu.z); q[1].w += o.w * (v.w - mu.w);
    }
};
template <bool ACT_FIRST>
static int32_t gate_bwd_data(const char* what, const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* scale, const float* shift, const float* pre,
                             int32_t gate, int32_t act, const float* dmean, float* dz, int64_t dz_ld, const float* save_mean, float* partials, int32_t N, int32_t HW,
                             int32_t C, void* stream) {
    SE_CHECK(what, N, HW, C, gate, act, scale, shift, {dy, x, pre, dz}, {dmean, save_mean, partials}, {dy_ld, x_ld, dz_ld});
    SGX_CHECK_ARG(!partials || save_mean, "%s: the reduce rows need save_mean", what);
    BnGateBwdDataF<ACT_FIRST> f{{x, x_ld, scale, shift, pre, gate, sgx_make_fastdiv(HW), C}, dy, dy_ld, act, dmean, 1.f / (float)HW, dz, dz_ld, save_mean};
    return run_sweep<BnGateBwdDataF<ACT_FIRST>, 2, 2>(f, (long)N * HW, C, partials, stream, what);
}
extern "C" int32_t sgx_bn_gate_act_bwd_data(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* scale, const float* shift,
                                            const float* pre, int32_t gate, int32_t act, const float* dmean, float* dz, int64_t dz_ld,
                                            const float* save_mean, float* partials, int32_t N, int32_t HW, int32_t C, void* stream) {
    return gate_bwd_data<false>("bn_gate_act_bwd_data", dy, dy_ld, x, x_ld, scale, shift, pre, gate, act, dmean, dz, dz_ld, save_mean, partials, N, HW, C, stream);
}
extern "C" int32_t sgx_bn_act_gate_bwd_data(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, const float* scale, const float* shift,
                                            const float* pre, int32_t gate, int32_t act, const float* dmean, float* dz, int64_t dz_ld,
                                            const float* save_mean, float* partials, int32_t N, int32_t HW, int32_t C, void* stream) {
    return gate_bwd_data<true>("bn_act_gate_bwd_data", dy, dy_ld, x, x_ld, scale, shift, pre, gate, act, dmean, dz, dz_ld, save_mean, partials, N, HW, C, stream);
}

// y = f(pre[n][c]) * z + r: a per-image multiplier inside the BatchNorm sweep together with the residual (drop-connect: gate NONE,
// pre[n][:] = the image's 0 or 1 / keep).  Backward: sgx_bn_gate_act_bwd_data(gate, act NONE) writes f(pre) * dy and the reduce rows.
struct BnGateAddFwdF : GateSweepF {
    const float* res; long r_ld; float* y; long y_ld;
    struct In { float4 v, p, r; };
    __device__ In load(long r, int c) const {
        const GateSweepF::In in = GateSweepF::load(r, c);
        return In{in.v, in.p, sgx_ld4(res + r * r_ld + c)};
    }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        const float4 z = k.z(in.v), s = se_gate4(in.p, gate);
        sgx_st4(y + r * y_ld + c, make_float4(s.x * z.x + in.r.x, s.y * z.y + in.r.y, s.z * z.z + in.r.z, s.w * z.w + in.r.w));
    }
};
extern "C" int32_t sgx_bn_gate_add_fwd(const float* x, int64_t x_ld, const float* scale, const float* shift, const float* pre, int32_t gate,
                                       const float* r, int64_t r_ld, float* y, int64_t y_ld, int32_t N, int32_t HW, int32_t C, void* stream) {
    SE_CHECK("bn_gate_add_fwd", N, HW, C, gate, SGX_ACT_NONE, scale, shift, {x, pre, r, y}, {}, {x_ld, r_ld, y_ld});
    BnGateAddFwdF f{{x, x_ld, scale, shift, pre, gate, sgx_make_fastdiv(HW), C}, r, r_ld, y, y_ld};
    return run_sweep<BnGateAddFwdF, 0, 2>(f, (long)N * HW, C, nullptr, stream, "bn_gate_add_fwd");
}

// The Vision Transformer's kernels (attention, LayerNorm, GELU, patch rows, token assembly) build in this translation unit: they share the
// sweep skeleton and the float4 / alignment conventions above.
#include "vit.h"
