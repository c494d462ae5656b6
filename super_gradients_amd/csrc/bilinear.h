// Bilinear interpolation by integer scale factors (ATen's upsample_bilinear2d, both align_corners settings) and the 2x2 ceil-mode average
// pool.  Included by se.hip behind the nearest-neighbour up-sampling.  Memory-bound sweeps, no matrix pipe; deterministic: the backward
// kernels are gathers - every dx element finds the dy rows / columns whose two-tap footprint contains it and adds them in ascending order.
//   NHWC form   x [N,H,W,C] -> y [N,sh H,sw W,C] (+ addend), operands may be channel slices (C and strides multiples of 4): a lane owns one
//               float4 channel group of one output pixel.
//   NCHW form   the segmentation head: x is the NHWC logits (any C, any pixel stride), y the contiguous NCHW [N,C,sh H,sw W]; lanes run
//               along the output row (four columns per lane, one 16-byte store), one plane per (n, c): up-sampling and layout change in one pass.
// Source coordinates and weights are computed in float exactly as ATen computes them, in ONE function both directions call.
#pragma once

struct BlAxis {
    int in, out;
    float scale;  // align_corners: (in - 1) / (out - 1) (0 when out == 1), else 1 / factor
    int align;
};
static BlAxis bl_axis(int in, int factor, int align) {
    BlAxis a;
    a.in = in; a.out = in * factor; a.align = align;
    a.scale = align ? (a.out > 1 ? (float)(in - 1) / (float)(a.out - 1) : 0.f) : 1.f / (float)factor;
    return a;
}
// output index o reads inputs i0 and i1 with weights 1 - l1 and l1
__device__ __forceinline__ void bl_src(const BlAxis& a, int o, int& i0, int& i1, float& l1) {
    float s = a.align ? a.scale * (float)o : a.scale * ((float)o + 0.5f) - 0.5f;
    if (!a.align && s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > a.in - 1) i0 = a.in - 1;
    i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
    l1 = s - (float)i0;
}
// the outputs [lo, hi] that can read input i: the inverse map with a one-pixel guard (weights are not periodic under align_corners)
__device__ __forceinline__ void bl_range(const BlAxis& a, int i, int& lo, int& hi) {
    lo = 0; hi = a.out - 1;
    if (a.scale > 0.f) {
        const float off = a.align ? 0.f : 0.5f;
        const int l = (int)floorf(((float)(i - 1) + off) / a.scale - off) - 1, h = (int)ceilf(((float)(i + 1) + off) / a.scale - off) + 1;
        if (l > lo) lo = l;
        if (h < hi) hi = h;
    }
}
// weight of input i in output o (0 outside the footprint; both taps when they coincide at the edge)
__device__ __forceinline__ float bl_weight(const BlAxis& a, int o, int i) {
    int i0, i1;
    float l1;
    bl_src(a, o, i0, i1, l1);
    return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

__global__ __launch_bounds__(256) void bilinear_fwd_kernel(int N, int C, BlAxis ah, BlAxis aw, const float* __restrict__ x, long x_ld_pix, long x_ld_img,
                                                           const float* __restrict__ addend, long a_ld_pix, long a_ld_img, float* __restrict__ y,
                                                           long y_ld_pix, long y_ld_img) {
    const int C4 = C / 4;
    const long n = (long)N * ah.out * aw.out * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int ow = (int)(t % aw.out);
        t /= aw.out;
        const int oh = (int)(t % ah.out), img = (int)(t / ah.out);
        int h0, h1, w0, w1;
        float lh, lw;
        bl_src(ah, oh, h0, h1, lh);
        bl_src(aw, ow, w0, w1, lw);
        const float* xb = x + (long)img * x_ld_img + c;
        const float4 v00 = sgx_ld4(xb + ((long)h0 * aw.in + w0) * x_ld_pix), v01 = sgx_ld4(xb + ((long)h0 * aw.in + w1) * x_ld_pix);
        const float4 v10 = sgx_ld4(xb + ((long)h1 * aw.in + w0) * x_ld_pix), v11 = sgx_ld4(xb + ((long)h1 * aw.in + w1) * x_ld_pix);
        const float kh = 1.f - lh, kw = 1.f - lw;
        float4 o = make_float4(kh * (kw * v00.x + lw * v01.x) + lh * (kw * v10.x + lw * v11.x), kh * (kw * v00.y + lw * v01.y) + lh * (kw * v10.y + lw * v11.y),
                               kh * (kw * v00.z + lw * v01.z) + lh * (kw * v10.z + lw * v11.z), kh * (kw * v00.w + lw * v01.w) + lh * (kw * v10.w + lw * v11.w));
        const long opix = (long)oh * aw.out + ow;
        if (addend) {
            const float4 u = sgx_ld4(addend + (long)img * a_ld_img + opix * a_ld_pix + c);
            o.x += u.x; o.y += u.y; o.z += u.z; o.w += u.w;
        }
        sgx_st4(y + (long)img * y_ld_img + opix * y_ld_pix + c, o);
    }
}
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(int N, int C, BlAxis ah, BlAxis aw, const float* __restrict__ dy, long dy_ld_pix, long dy_ld_img,
                                                           float* __restrict__ dx, long dx_ld_pix, long dx_ld_img, int accumulate) {
    const int C4 = C / 4;
    const long n = (long)N * ah.in * aw.in * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int w = (int)(t % aw.in);
        t /= aw.in;
        const int h = (int)(t % ah.in), img = (int)(t / ah.in);
        int hlo, hhi, wlo, whi;
        bl_range(ah, h, hlo, hhi);
        bl_range(aw, w, wlo, whi);
        const float* db = dy + (long)img * dy_ld_img + c;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int oh = hlo; oh <= hhi; ++oh) {
            const float kh = bl_weight(ah, oh, h);
            if (kh == 0.f) continue;
            for (int ow = wlo; ow <= whi; ++ow) {
                const float k = kh * bl_weight(aw, ow, w);
                if (k == 0.f) continue;
                const float4 v = sgx_ld4(db + ((long)oh * aw.out + ow) * dy_ld_pix);
                s.x += k * v.x; s.y += k * v.y; s.z += k * v.z; s.w += k * v.w;
            }
        }
        float* xp = dx + (long)img * dx_ld_img + ((long)h * aw.in + w) * dx_ld_pix + c;
        if (accumulate) {
            const float4 u = sgx_ld4(xp);
            s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        sgx_st4(xp, s);
    }
}

// NCHW head: a lane owns four consecutive columns of one output row of one (n, c) plane
__global__ __launch_bounds__(256) void bilinear_nchw_fwd_kernel(int N, int C, BlAxis ah, BlAxis aw, const float* __restrict__ x, long x_ld_pix, long x_ld_img,
                                                                float* __restrict__ y) {
    const int W4 = (aw.out + 3) / 4;
    const long n = (long)N * C * ah.out * W4;
    const bool vec = aw.out % 4 == 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int ow0 = (int)(i % W4) * 4;
        long t = i / W4;
        const int oh = (int)(t % ah.out);
        t /= ah.out;
        const int c = (int)(t % C), img = (int)(t / C);
        int h0, h1;
        float lh;
        bl_src(ah, oh, h0, h1, lh);
        const float* r0 = x + (long)img * x_ld_img + (long)h0 * aw.in * x_ld_pix + c;
        const float* r1 = x + (long)img * x_ld_img + (long)h1 * aw.in * x_ld_pix + c;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ow0 + j >= aw.out) break;
            int w0, w1;
            float lw;
            bl_src(aw, ow0 + j, w0, w1, lw);
            o[j] = (1.f - lh) * ((1.f - lw) * r0[w0 * x_ld_pix] + lw * r0[w1 * x_ld_pix]) + lh * ((1.f - lw) * r1[w0 * x_ld_pix] + lw * r1[w1 * x_ld_pix]);
        }
        float* yp = y + (((long)img * C + c) * ah.out + oh) * aw.out + ow0;
        if (vec) {
            sgx_st4(yp, make_float4(o[0], o[1], o[2], o[3]));
        } else {
            for (int j = 0; j < 4 && ow0 + j < aw.out; ++j) yp[j] = o[j];
        }
    }
}
// dx [N,H,W,C] (NHWC logit gradient) from the NCHW dy: lanes run along the input row, so a wave's dy reads stay inside a few rows of one plane
__global__ __launch_bounds__(256) void bilinear_nchw_bwd_kernel(int N, int C, BlAxis ah, BlAxis aw, const float* __restrict__ dy, float* __restrict__ dx,
                                                                long dx_ld_pix, long dx_ld_img) {
    const long n = (long)N * C * ah.in * aw.in;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int w = (int)(i % aw.in);
        long t = i / aw.in;
        const int h = (int)(t % ah.in);
        t /= ah.in;
        const int c = (int)(t % C), img = (int)(t / C);
        int hlo, hhi, wlo, whi;
        bl_range(ah, h, hlo, hhi);
        bl_range(aw, w, wlo, whi);
        const float* db = dy + ((long)img * C + c) * ah.out * aw.out;
        float s = 0.f;
        for (int oh = hlo; oh <= hhi; ++oh) {
            const float kh = bl_weight(ah, oh, h);
            if (kh == 0.f) continue;
            for (int ow = wlo; ow <= whi; ++ow) s += kh * bl_weight(aw, ow, w) * db[(long)oh * aw.out + ow];
        }
        dx[(long)img * dx_ld_img + ((long)h * aw.in + w) * dx_ld_pix + c] = s;
    }
}

// nn.AvgPool2d(2, 2, ceil_mode=True), pad 0: the bottom / right windows are clipped and divide by the in-bounds count
__global__ __launch_bounds__(256) void avgpool2_ceil_kernel(int N, int H, int W, int C, const float* __restrict__ src, long s_ld_pix, long s_ld_img,
                                                            float* __restrict__ dst, long d_ld_pix, long d_ld_img, int backward, int accumulate) {
    const int C4 = C / 4, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int A = backward ? H : Ho, B = backward ? W : Wo;  // the map this launch writes
    const long n = (long)N * A * B * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        long t = i / C4;
        const int b = (int)(t % B);
        t /= B;
        const int a = (int)(t % A), img = (int)(t / A);
        const int ho = backward ? a / 2 : a, wo = backward ? b / 2 : b;
        const int nh = min(2, H - 2 * ho), nw = min(2, W - 2 * wo);
        const float k = 1.f / (float)(nh * nw);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (backward) {
            const float4 v = sgx_ld4(src + (long)img * s_ld_img + ((long)ho * Wo + wo) * s_ld_pix + c);
            s = make_float4(v.x * k, v.y * k, v.z * k, v.w * k);
        } else {
            for (int r = 0; r < nh; ++r)
                for (int q = 0; q < nw; ++q) {
                    const float4 v = sgx_ld4(src + (long)img * s_ld_img + ((long)(2 * ho + r) * W + 2 * wo + q) * s_ld_pix + c);
                    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
                }
            s = make_float4(s.x * k, s.y * k, s.z * k, s.w * k);
        }
        float* dp = dst + (long)img * d_ld_img + ((long)a * B + b) * d_ld_pix + c;
        if (accumulate) {
            const float4 u = sgx_ld4(dp);
            s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        sgx_st4(dp, s);
    }
}

#define BL_GRID(n) dim3((unsigned)SGX_STRIDE_GRID(((n) + 255) / 256 > 16384 ? 16384 : ((n) + 255) / 256))
static int32_t bl_check(int N, int H, int W, int C, int sh, int sw, const char* what) {
    SGX_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "%s: bad dims N=%d H=%d W=%d C=%d", what, N, H, W, C);
    SGX_CHECK_ARG(sh >= 1 && sw >= 1 && sh <= 64 && sw <= 64, "%s: scale factors %d x %d must be 1 .. 64", what, sh, sw);
    SGX_CHECK_ARG((long)N * H * sh * W * sw < 0x7fffffffL, "%s: more than 2^31 output pixels", what);
    return SGX_OK;
}
extern "C" int32_t sgx_bilinear_fwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t sh, int32_t sw, int32_t align_corners, const float* x,
                                    int64_t x_ld_pix, int64_t x_ld_img, const float* addend, int64_t a_ld_pix, int64_t a_ld_img, float* y,
                                    int64_t y_ld_pix, int64_t y_ld_img, void* stream) {
    int32_t rc = bl_check(N, H, W, C, sh, sw, "bilinear_fwd");
    if (rc) return rc;
    SGX_CHECK_ARG(x && y && C % 4 == 0, "bilinear_fwd: null pointer or C=%d no multiple of 4", C);
    SGX_CHECK_ARG(SW_LD4(x_ld_pix) && SW_LD4(x_ld_img) && SW_LD4(y_ld_pix) && SW_LD4(y_ld_img) && SW_ALIGNED(x) && SW_ALIGNED(y) &&
                      (!addend || (SW_LD4(a_ld_pix) && SW_LD4(a_ld_img) && SW_ALIGNED(addend))),
                  "bilinear_fwd: strides and addresses must be multiples of 16 bytes");
    const long n = (long)N * H * sh * W * sw * (C / 4);
    SGX_LAUNCH(bilinear_fwd_kernel, BL_GRID(n), dim3(256), 0, stream, N, C, bl_axis(H, sh, align_corners), bl_axis(W, sw, align_corners), x, (long)x_ld_pix,
               (long)x_ld_img, addend, (long)a_ld_pix, (long)a_ld_img, y, (long)y_ld_pix, (long)y_ld_img);
    SGX_CHECK_LAUNCH("bilinear_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_bilinear_bwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t sh, int32_t sw, int32_t align_corners, const float* dy,
                                    int64_t dy_ld_pix, int64_t dy_ld_img, float* dx, int64_t dx_ld_pix, int64_t dx_ld_img, int32_t accumulate,
                                    void* stream) {
    int32_t rc = bl_check(N, H, W, C, sh, sw, "bilinear_bwd");
    if (rc) return rc;
    SGX_CHECK_ARG(dy && dx && C % 4 == 0, "bilinear_bwd: null pointer or C=%d no multiple of 4", C);
    SGX_CHECK_ARG(SW_LD4(dy_ld_pix) && SW_LD4(dy_ld_img) && SW_LD4(dx_ld_pix) && SW_LD4(dx_ld_img) && SW_ALIGNED(dy) && SW_ALIGNED(dx),
                  "bilinear_bwd: strides and addresses must be multiples of 16 bytes");
    const long n = (long)N * H * W * (C / 4);
    SGX_LAUNCH(bilinear_bwd_kernel, BL_GRID(n), dim3(256), 0, stream, N, C, bl_axis(H, sh, align_corners), bl_axis(W, sw, align_corners), dy, (long)dy_ld_pix,
               (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate ? 1 : 0);
    SGX_CHECK_LAUNCH("bilinear_bwd");
    return SGX_OK;
}
extern "C" int32_t sgx_bilinear_nchw_fwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t sh, int32_t sw, int32_t align_corners, const float* x,
                                         int64_t x_ld_pix, int64_t x_ld_img, float* y, void* stream) {
    int32_t rc = bl_check(N, H, W, C, sh, sw, "bilinear_nchw_fwd");
    if (rc) return rc;
    SGX_CHECK_ARG(x && y && x_ld_pix >= C && SW_ALIGNED(y), "bilinear_nchw_fwd: null pointer, pixel stride below C or y not 16-byte aligned");
    const long n = (long)N * C * H * sh * ((W * sw + 3) / 4);
    SGX_LAUNCH(bilinear_nchw_fwd_kernel, BL_GRID(n), dim3(256), 0, stream, N, C, bl_axis(H, sh, align_corners), bl_axis(W, sw, align_corners), x, (long)x_ld_pix,
               (long)x_ld_img, y);
    SGX_CHECK_LAUNCH("bilinear_nchw_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_bilinear_nchw_bwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t sh, int32_t sw, int32_t align_corners, const float* dy,
                                         float* dx, int64_t dx_ld_pix, int64_t dx_ld_img, void* stream) {
    int32_t rc = bl_check(N, H, W, C, sh, sw, "bilinear_nchw_bwd");
    if (rc) return rc;
    SGX_CHECK_ARG(dy && dx && dx_ld_pix >= C, "bilinear_nchw_bwd: null pointer or pixel stride below C");
    const long n = (long)N * C * H * W;
    SGX_LAUNCH(bilinear_nchw_bwd_kernel, BL_GRID(n), dim3(256), 0, stream, N, C, bl_axis(H, sh, align_corners), bl_axis(W, sw, align_corners), dy, dx,
               (long)dx_ld_pix, (long)dx_ld_img);
    SGX_CHECK_LAUNCH("bilinear_nchw_bwd");
    return SGX_OK;
}
static int32_t ap2_launch(int N, int H, int W, int C, const float* src, long s_ld_pix, long s_ld_img, float* dst, long d_ld_pix, long d_ld_img, int backward,
                          int accumulate, void* stream, const char* what) {
    SGX_CHECK_ARG(src && dst && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "%s: bad args (C=%d)", what, C);
    SGX_CHECK_ARG(SW_LD4(s_ld_pix) && SW_LD4(s_ld_img) && SW_LD4(d_ld_pix) && SW_LD4(d_ld_img) && SW_ALIGNED(src) && SW_ALIGNED(dst),
                  "%s: strides and addresses must be multiples of 16 bytes", what);
    SGX_CHECK_ARG((long)N * H * W < 0x7fffffffL, "%s: more than 2^31 pixels", what);
    const long n = (long)N * (backward ? (long)H * W : (long)((H + 1) / 2) * ((W + 1) / 2)) * (C / 4);
    SGX_LAUNCH(avgpool2_ceil_kernel, BL_GRID(n), dim3(256), 0, stream, N, H, W, C, src, s_ld_pix, s_ld_img, dst, d_ld_pix, d_ld_img, backward, accumulate);
    SGX_CHECK_LAUNCH(what);
    return SGX_OK;
}
extern "C" int32_t sgx_avgpool2_ceil_fwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* x, int64_t x_ld_pix, int64_t x_ld_img, float* y,
                                         int64_t y_ld_pix, int64_t y_ld_img, void* stream) {
    return ap2_launch(N, H, W, C, x, (long)x_ld_pix, (long)x_ld_img, y, (long)y_ld_pix, (long)y_ld_img, 0, 0, stream, "avgpool2_ceil_fwd");
}
extern "C" int32_t sgx_avgpool2_ceil_bwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* dy, int64_t dy_ld_pix, int64_t dy_ld_img, float* dx,
                                         int64_t dx_ld_pix, int64_t dx_ld_img, int32_t accumulate, void* stream) {
    return ap2_launch(N, H, W, C, dy, (long)dy_ld_pix, (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, 1, accumulate ? 1 : 0, stream, "avgpool2_ceil_bwd");
}
