// Pooling kernels (HBM/L2-bound, no MFMA): SPP max-pool k=5/9/13 stride 1, ResNet 3x3 s2 max-pool,
// global average pool.  One thread owns a float4 channel group of one output pixel.
// Below them: the depthwise 3x3 convolution (forward, data gradient, weight gradient) - the other per-channel window kernels.
// Reference call sites: include/sgx_hip.h (Pooling section).
#include "sgx_common.h"
#include <atomic>

#define SGX_ALIGNED16(p) (((uintptr_t)(p) % 16) == 0)
// output extent of a pooling window walk; 0 when the padded map is smaller than the window (a truncating division alone would say 1 at stride > 1)
static int maxpool_out(int in, int k, int stride, int pad) { return in + 2 * pad < k ? 0 : (in + 2 * pad - k) / stride + 1; }

__global__ void maxpool_fwd_kernel(int N, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, const float* x, long x_ld_pix,
                                   long x_ld_img, float* y, long y_ld_pix, long y_ld_img, int* argmax) {
    const int C4 = C / 4;
    long n = (long)N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        long pix = i / C4;
        int wo = (int)(pix % Wo);
        long t = pix / Wo;
        int ho = (int)(t % Ho);
        int img = (int)(t / Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        int ix = -1, iy = -1, iz = -1, iw = -1;
        for (int r = 0; r < k; ++r) {
            int hi = ho * stride - pad + r;
            if (hi < 0 || hi >= H) continue;
            for (int q = 0; q < k; ++q) {
                int wi = wo * stride - pad + q;
                if (wi < 0 || wi >= W) continue;
                float4 v = sgx_ld4(x + (long)img * x_ld_img + ((long)hi * W + wi) * x_ld_pix + c);
                int idx = hi * W + wi;
                if (v.x > m.x || ix < 0) { m.x = v.x; ix = idx; }
                if (v.y > m.y || iy < 0) { m.y = v.y; iy = idx; }
                if (v.z > m.z || iz < 0) { m.z = v.z; iz = idx; }
                if (v.w > m.w || iw < 0) { m.w = v.w; iw = idx; }
            }
        }
        sgx_st4(y + (long)img * y_ld_img + ((long)ho * Wo + wo) * y_ld_pix + c, m);
        if (argmax) {
            int* a = argmax + pix * C + c;
            a[0] = ix; a[1] = iy; a[2] = iz; a[3] = iw;
        }
    }
}

// ---- stride-1 pooling of a map that fits LDS (the SPP's 5 / 9 / 13 windows on the last backbone map): one workgroup owns MP_CG channels of one
// image.  The direct kernel above reads k x k inputs per output (169 float4 loads at k = 13: 88 us per call on the 32 x 20 x 20 x 384 map,
// r4r); here the map is staged once and the window is walked separably - per row the first largest value of the k columns, then down the k rows
// the first row holding the largest of those: exactly the first maximum in row-major window order, which is what ATen returns.
#define MP_CG 8
#define MP_TILE_MAX_LDS 65536  // dynamic LDS a launch may ask for without raising the function's limit
static long maxpool_fwd_tile_lds(int H, int W, int Wo) { return (long)H * W * MP_CG * 4 + (long)H * Wo * MP_CG * 6; }
// The kernel a forward launch runs: 0 the direct kernel, 1 the LDS tile.  sgx_maxpool_fwd and sgx_debug_maxpool_form both ask here.
static int maxpool_fwd_form(int H, int W, int C, int k, int stride, int pad) {
    const int Ho = maxpool_out(H, k, stride, pad), Wo = maxpool_out(W, k, stride, pad);
    return (stride == 1 && C % MP_CG == 0 && Ho > 0 && Wo > 0 && (long)H * W < 65536 && maxpool_fwd_tile_lds(H, W, Wo) <= MP_TILE_MAX_LDS && k > 2) ? 1 : 0;
}
__global__ __launch_bounds__(256) void maxpool_fwd_tile_kernel(int H, int W, int C, int k, int pad, int Ho, int Wo, const float* x, long x_ld_pix,
                                                               long x_ld_img, float* y, long y_ld_pix, long y_ld_img, int* argmax) {
    SGX_DYN_SMEM(float, smem);
    float* s_x = smem;                                                   // [H * W][MP_CG]
    float* s_v = smem + (long)H * W * MP_CG;                              // [H * Wo][MP_CG]: row maxima
    unsigned short* s_q = (unsigned short*)(s_v + (long)H * Wo * MP_CG);  // their columns
    const int groups = C / MP_CG;
    const int img = blockIdx.x / groups, c0 = (blockIdx.x % groups) * MP_CG;
    for (int i = threadIdx.x; i < H * W * (MP_CG / 4); i += blockDim.x) {
        const int pix = i / (MP_CG / 4), h4 = (i % (MP_CG / 4)) * 4;
        const float4 v = sgx_ld4(x + (long)img * x_ld_img + (long)pix * x_ld_pix + c0 + h4);
        float* d = s_x + pix * MP_CG + h4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    // (a lane owns FOUR channels: 16-byte LDS reads and 16-byte stores - as one channel per lane the kernel took 52 / 67 / 82 us for k = 5 / 9 /
    // 13 on the 32 x 20 x 20 x 384 map, r4w, bound by its instruction count and its 4-byte stores)
    for (int i = threadIdx.x; i < H * Wo * (MP_CG / 4); i += blockDim.x) {
        const int c4 = (i % (MP_CG / 4)) * 4, t = i / (MP_CG / 4), wo = t % Wo, hi = t / Wo;
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int q[4] = {-1, -1, -1, -1};
        for (int j = 0; j < k; ++j) {
            const int wi = wo - pad + j;
            if (wi < 0 || wi >= W) continue;
            const float4 v4 = sgx_ld4(s_x + (hi * W + wi) * MP_CG + c4);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int z = 0; z < 4; ++z)
                if (v[z] > m[z] || q[z] < 0) { m[z] = v[z]; q[z] = wi; }
        }
        sgx_st4(s_v + t * MP_CG + c4, make_float4(m[0], m[1], m[2], m[3]));
        unsigned short* sq = s_q + t * MP_CG + c4;
        sq[0] = (unsigned short)q[0]; sq[1] = (unsigned short)q[1]; sq[2] = (unsigned short)q[2]; sq[3] = (unsigned short)q[3];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < Ho * Wo * (MP_CG / 4); i += blockDim.x) {
        const int c4 = (i % (MP_CG / 4)) * 4, o = i / (MP_CG / 4), wo = o % Wo, ho = o / Wo;
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int idx[4] = {-1, -1, -1, -1};
        for (int r = 0; r < k; ++r) {
            const int hi = ho - pad + r;
            if (hi < 0 || hi >= H) continue;
            const int e = (hi * Wo + wo) * MP_CG + c4;
            const float4 v4 = sgx_ld4(s_v + e);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int z = 0; z < 4; ++z)
                if (v[z] > m[z] || idx[z] < 0) { m[z] = v[z]; idx[z] = hi * W + (int)s_q[e + z]; }
        }
        sgx_st4(y + (long)img * y_ld_img + (long)o * y_ld_pix + c0 + c4, make_float4(m[0], m[1], m[2], m[3]));
        if (argmax) {
            int* am = argmax + ((long)img * Ho * Wo + o) * C + c0 + c4;
            am[0] = idx[0]; am[1] = idx[1]; am[2] = idx[2]; am[3] = idx[3];
        }
    }
}

extern "C" int32_t sgx_maxpool_fwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, const float* x,
                                   int64_t x_ld_pix, int64_t x_ld_img, float* y, int64_t y_ld_pix, int64_t y_ld_img, int32_t* argmax,
                                   void* stream) {
    SGX_CHECK_ARG(x && y && C % 4 == 0 && k > 0 && stride > 0, "maxpool_fwd: bad args");
    SGX_CHECK_ARG(pad >= 0 && 2 * pad <= k, "maxpool_fwd: pad %d must be at most half the window %d (F.max_pool2d's own rule)", pad, k);
    SGX_CHECK_ARG(x_ld_pix % 4 == 0 && x_ld_img % 4 == 0 && y_ld_pix % 4 == 0 && y_ld_img % 4 == 0 && SGX_ALIGNED16(x) && SGX_ALIGNED16(y),
                  "maxpool_fwd: strides and addresses must be multiples of 16 bytes");
    const int Ho = maxpool_out(H, k, stride, pad), Wo = maxpool_out(W, k, stride, pad);
    SGX_CHECK_ARG(Ho > 0 && Wo > 0, "maxpool_fwd: empty output");
    if (maxpool_fwd_form(H, W, C, k, stride, pad) == 1) {
        SGX_LAUNCH(maxpool_fwd_tile_kernel, dim3((unsigned)(N * (C / MP_CG))), dim3(256), (unsigned)maxpool_fwd_tile_lds(H, W, Wo), stream, H, W, C, k, pad,
                   Ho, Wo, x, (long)x_ld_pix, (long)x_ld_img, y, (long)y_ld_pix, (long)y_ld_img, argmax);
        SGX_CHECK_LAUNCH("maxpool_fwd (tile)");
        return SGX_OK;
    }
    long n = (long)N * Ho * Wo * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(maxpool_fwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, H, W, C, k, stride, pad, Ho, Wo,
               x, (long)x_ld_pix, (long)x_ld_img, y, (long)y_ld_pix, (long)y_ld_img, argmax);
    SGX_CHECK_LAUNCH("maxpool_fwd");
    return SGX_OK;
}

__global__ void maxpool_bwd_kernel(int N, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, const int* argmax, const float* dy,
                                   long dy_ld_pix, long dy_ld_img, float* dx, long dx_ld_pix, long dx_ld_img, int accumulate) {
    const int C4 = C / 4;
    long n = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        long pix = i / C4;
        int wi = (int)(pix % W);
        long t = pix / W;
        int hi = (int)(t % H);
        int img = (int)(t / H);
        const int me = hi * W + wi;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        // output windows containing (hi, wi): ho*stride - pad <= hi <= ho*stride - pad + k - 1
        int ho_lo = (hi + pad - k + 1 + stride - 1);
        ho_lo = ho_lo < 0 ? 0 : ho_lo / stride;
        int ho_hi = (hi + pad) / stride;
        if (ho_hi > Ho - 1) ho_hi = Ho - 1;
        int wo_lo = (wi + pad - k + 1 + stride - 1);
        wo_lo = wo_lo < 0 ? 0 : wo_lo / stride;
        int wo_hi = (wi + pad) / stride;
        if (wo_hi > Wo - 1) wo_hi = Wo - 1;
        for (int ho = ho_lo; ho <= ho_hi; ++ho)
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                long op = ((long)img * Ho + ho) * Wo + wo;
                const int* a = argmax + op * C + c;
                float4 d = sgx_ld4(dy + (long)img * dy_ld_img + ((long)ho * Wo + wo) * dy_ld_pix + c);
                if (a[0] == me) g.x += d.x;
                if (a[1] == me) g.y += d.y;
                if (a[2] == me) g.z += d.z;
                if (a[3] == me) g.w += d.w;
            }
        float* o = dx + (long)img * dx_ld_img + (long)me * dx_ld_pix + c;
        if (accumulate) {
            float4 u = sgx_ld4(o);
            g.x += u.x; g.y += u.y; g.z += u.z; g.w += u.w;
        }
        sgx_st4(o, g);
    }
}

// The same for the backward pass: the direct kernel reads the argmax (16 B) and the gradient (16 B) of every window an input pixel lies in -
// 169 x 32 B per float4 at k = 13, 150 - 350 us per call (r4r: 0.68 ms per step for the SPP's three pools).  Here the output map's argmax
// (as 16-bit pixel indices) and gradient are staged once per MP_CG channels of an image and the windows are walked in LDS, in the same order:
// the sums are bit-identical to the direct kernel's.
__global__ __launch_bounds__(256) void maxpool_bwd_tile_kernel(int H, int W, int C, int k, int pad, int Ho, int Wo, const int* argmax, const float* dy,
                                                               long dy_ld_pix, long dy_ld_img, float* dx, long dx_ld_pix, long dx_ld_img, int accumulate) {
    SGX_DYN_SMEM(float, smem);
    float* s_dy = smem;                                                        // [Ho * Wo][MP_CG]
    unsigned short* s_ix = (unsigned short*)(smem + (long)Ho * Wo * MP_CG);     // [Ho * Wo][MP_CG]
    const int groups = C / MP_CG;
    const int img = blockIdx.x / groups, c0 = (blockIdx.x % groups) * MP_CG;
    for (int i = threadIdx.x; i < Ho * Wo * (MP_CG / 4); i += blockDim.x) {
        const int o = i / (MP_CG / 4), h4 = (i % (MP_CG / 4)) * 4;
        const float4 d = sgx_ld4(dy + (long)img * dy_ld_img + (long)o * dy_ld_pix + c0 + h4);
        const int* a = argmax + ((long)img * Ho * Wo + o) * C + c0 + h4;
        float* sd = s_dy + o * MP_CG + h4;
        unsigned short* si = s_ix + o * MP_CG + h4;
        sd[0] = d.x; sd[1] = d.y; sd[2] = d.z; sd[3] = d.w;
        si[0] = (unsigned short)a[0]; si[1] = (unsigned short)a[1]; si[2] = (unsigned short)a[2]; si[3] = (unsigned short)a[3];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < H * W * MP_CG; i += blockDim.x) {
        const int c = i % MP_CG, me = i / MP_CG, wi = me % W, hi = me / W;
        int ho_lo = hi + pad - k + 1, ho_hi = hi + pad, wo_lo = wi + pad - k + 1, wo_hi = wi + pad;
        if (ho_lo < 0) ho_lo = 0;
        if (wo_lo < 0) wo_lo = 0;
        if (ho_hi > Ho - 1) ho_hi = Ho - 1;
        if (wo_hi > Wo - 1) wo_hi = Wo - 1;
        float g = 0.f;
        for (int ho = ho_lo; ho <= ho_hi; ++ho)
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                const int e = (ho * Wo + wo) * MP_CG + c;
                if ((int)s_ix[e] == me) g += s_dy[e];
            }
        float* o = dx + (long)img * dx_ld_img + (long)me * dx_ld_pix + c0 + c;
        *o = accumulate ? *o + g : g;
    }
}

// The gather forms above cost k x k window tests per input element whatever they read from (r4z: the LDS form 198 us per call against the
// direct kernel's 226 - 1.35 G tests per step for the SPP's 5 / 9 / 13 pools, bound by their ~5 vector instructions each).  The scatter form
// costs ONE add per OUTPUT element: a wave owns 64 channels of one image, lane = channel, keeps that (image, channels) slice of dx in LDS
// (H x W x 64 floats: 100 KB for the 20 x 20 map) and walks the outputs in ascending order - every lane adds its gradient at its arg-max
// pixel.  Lanes never share an address (different channels) and a lane's additions happen in output order: the sums are deterministic and in
// the order of ATen's CPU kernel.  Eight outputs of loads in flight per lane; no atomics.  The plain backward leaves the bits of the two
// gather forms (tests/test_pool_kernels.py holds the three to it); with `accumulate` this form starts its chain from the target's value,
// where the gather forms add the target last.
// Round 5: 32 channels per workgroup by default (half a wave adds; 50 KB for the 20 x 20 map).  Alone on the chip the 64-channel form is
// as fast (the add chain is latency-bound either way), but in the train step its 100 KB workgroups waited for a CU with that much LDS
// free while weight-gradient kernels of the side stream were resident: 200 us per call in the step's trace against 35 alone (r5m).
#define MP_SCATTER_CH 32
#define MP_SCATTER_THREADS 256
#define MP_SCATTER_MAX_LDS (152 * 1024)
template <int CH>
__global__ __launch_bounds__(MP_SCATTER_THREADS) void maxpool_bwd_scatter_kernel(int HW, int C, int HoWo, const int* argmax, const float* dy, long dy_ld_pix,
                                                                                 long dy_ld_img, float* dx, long dx_ld_pix, long dx_ld_img, int accumulate) {
    SGX_DYN_SMEM(float, tile);  // [HW][CH]
    constexpr int PP = MP_SCATTER_THREADS / CH;  // pixels per pass of the load / store phases (thread = (pixel slot, channel))
    const int groups = C / CH, ch = threadIdx.x % CH, ps = threadIdx.x / CH;
    const int img = blockIdx.x / groups, c = (blockIdx.x % groups) * CH + ch;
    float* const gx = dx + (long)img * dx_ld_img + c;
    // the slice's starting value: every thread, eight pixels of loads in flight (a lane's scatter below is a chain of ~1 us memory
    // round trips as it is: r4v measured 372 us per call with one wave doing everything, eight outputs at a time)
    for (int p0 = ps * 8; p0 < HW; p0 += 8 * PP) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (accumulate && p0 + u < HW) ? gx[(long)(p0 + u) * dx_ld_pix] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (p0 + u < HW) tile[(p0 + u) * CH + ch] = v[u];
    }
    __syncthreads();
    if (threadIdx.x < CH) {  // ONE (part of a) wave adds, in output order; lane = channel
        const int* const a = argmax + (long)img * HoWo * C + c;
        const float* const g = dy + (long)img * dy_ld_img + c;
        int o = 0;
        for (; o + 32 <= HoWo; o += 32) {
            int ix[32];
            float d[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) {
                ix[u] = a[(long)(o + u) * C];
                d[u] = g[(long)(o + u) * dy_ld_pix];
            }
#pragma unroll
            for (int u = 0; u < 32; ++u)
                if (ix[u] >= 0) tile[ix[u] * CH + ch] += d[u];  // (-1: a window that lies in the padding only)
        }
        for (; o < HoWo; ++o) {
            const int ix = a[(long)o * C];
            if (ix >= 0) tile[ix * CH + ch] += g[(long)o * dy_ld_pix];
        }
    }
    __syncthreads();
    for (int p = ps; p < HW; p += PP) gx[(long)p * dx_ld_pix] = tile[p * CH + ch];
}

// The kernel a backward launch runs: 0 the direct kernel, 1 the LDS tile, 2 the LDS scatter (tried first).
static int maxpool_bwd_form(int H, int W, int C, int k, int stride, int pad) {
    const int Ho = maxpool_out(H, k, stride, pad), Wo = maxpool_out(W, k, stride, pad);
    if (C % MP_SCATTER_CH == 0 && Ho > 0 && Wo > 0 && (long)H * W * MP_SCATTER_CH * 4 <= MP_SCATTER_MAX_LDS) return 2;
    if (stride == 1 && C % MP_CG == 0 && Ho > 0 && Wo > 0 && (long)H * W < 65536 && (long)Ho * Wo * MP_CG * 6 <= MP_TILE_MAX_LDS && k > 2) return 1;
    return 0;
}
extern "C" int32_t sgx_debug_maxpool_form(int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, int32_t backward) {
    SGX_CHECK_ARG(H > 0 && W > 0 && C > 0 && k > 0 && stride > 0 && pad >= 0, "debug_maxpool_form: bad args");
    return backward ? maxpool_bwd_form(H, W, C, k, stride, pad) : maxpool_fwd_form(H, W, C, k, stride, pad);
}

extern "C" int32_t sgx_maxpool_bwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, const int32_t* argmax,
                                   const float* dy, int64_t dy_ld_pix, int64_t dy_ld_img, float* dx, int64_t dx_ld_pix, int64_t dx_ld_img,
                                   int32_t accumulate, void* stream) {
    SGX_CHECK_ARG(argmax && dy && dx && C % 4 == 0, "maxpool_bwd: bad args");
    SGX_CHECK_ARG(pad >= 0 && 2 * pad <= k, "maxpool_bwd: pad %d must be at most half the window %d", pad, k);
    SGX_CHECK_ARG(dy_ld_pix % 4 == 0 && dy_ld_img % 4 == 0 && dx_ld_pix % 4 == 0 && dx_ld_img % 4 == 0 && SGX_ALIGNED16(dy) && SGX_ALIGNED16(dx),
                  "maxpool_bwd: strides and addresses must be multiples of 16 bytes");
    const int Ho = maxpool_out(H, k, stride, pad), Wo = maxpool_out(W, k, stride, pad);
    SGX_CHECK_ARG(Ho > 0 && Wo > 0, "maxpool_bwd: empty output");
    const int form = maxpool_bwd_form(H, W, C, k, stride, pad);
    if (form == 2) {
        const unsigned lds = (unsigned)((long)H * W * MP_SCATTER_CH * 4);
#ifndef SGX_EMU
        // dynamic LDS beyond 64 KB is opt-in per function AND per device: one flag bit per device ordinal
        static std::atomic<unsigned long long> raised{0ull};
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            if (hipFuncSetAttribute((const void*)maxpool_bwd_scatter_kernel<MP_SCATTER_CH>, hipFuncAttributeMaxDynamicSharedMemorySize, MP_SCATTER_MAX_LDS) != hipSuccess)
                SGX_FAIL(SGX_ERR_HIP, "maxpool_bwd: cannot raise the scatter kernel's dynamic LDS limit");
            raised.fetch_or(bit, std::memory_order_release);
        }
#endif
        SGX_LAUNCH(maxpool_bwd_scatter_kernel<MP_SCATTER_CH>, dim3((unsigned)(N * (C / MP_SCATTER_CH))), dim3(MP_SCATTER_THREADS), lds, stream, H * W, C, Ho * Wo, argmax, dy,
                   (long)dy_ld_pix, (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate);
        SGX_CHECK_LAUNCH("maxpool_bwd (scatter)");
        return SGX_OK;
    }
    if (form == 1) {
        SGX_LAUNCH(maxpool_bwd_tile_kernel, dim3((unsigned)(N * (C / MP_CG))), dim3(256), (unsigned)((long)Ho * Wo * MP_CG * 6), stream, H, W, C, k, pad, Ho, Wo,
                   argmax, dy, (long)dy_ld_pix, (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate);
        SGX_CHECK_LAUNCH("maxpool_bwd (tile)");
        return SGX_OK;
    }
    long n = (long)N * H * W * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(maxpool_bwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, H, W, C, k, stride, pad, Ho, Wo,
               argmax, dy, (long)dy_ld_pix, (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate);
    SGX_CHECK_LAUNCH("maxpool_bwd");
    return SGX_OK;
}

__global__ void avgpool_fwd_kernel(int N, int HW, int C, const float* x, long ld_pix, long ld_img, float* y) {
    const int C4 = C / 4;
    long n = (long)N * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        int img = (int)(i / C4);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = 0; p < HW; ++p) {
            float4 v = sgx_ld4(x + (long)img * ld_img + (long)p * ld_pix + c);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        float inv = 1.f / (float)HW;
        sgx_st4(y + (long)img * C + c, make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv));
    }
}
extern "C" int32_t sgx_avgpool_fwd(int32_t N, int32_t HW, int32_t C, const float* x, int64_t x_ld_pix, int64_t x_ld_img, float* y, void* stream) {
    SGX_CHECK_ARG(x && y && C % 4 == 0, "avgpool_fwd: bad args");
    SGX_CHECK_ARG(x_ld_pix % 4 == 0 && x_ld_img % 4 == 0 && SGX_ALIGNED16(x) && SGX_ALIGNED16(y), "avgpool_fwd: strides and addresses must be multiples of 16 bytes");
    long n = (long)N * (C / 4), blocks = (n + 63) / 64;
    SGX_LAUNCH(avgpool_fwd_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, N, HW, C, x, (long)x_ld_pix, (long)x_ld_img, y);
    SGX_CHECK_LAUNCH("avgpool_fwd");
    return SGX_OK;
}
__global__ void avgpool_bwd_kernel(int N, int HW, int C, const float* dy, float* dx, long ld_pix, long ld_img) {
    const int C4 = C / 4;
    long n = (long)N * HW * C4;
    float inv = 1.f / (float)HW;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) * 4;
        long t = i / C4;
        int p = (int)(t % HW);
        int img = (int)(t / HW);
        float4 d = sgx_ld4(dy + (long)img * C + c);
        sgx_st4(dx + (long)img * ld_img + (long)p * ld_pix + c, make_float4(d.x * inv, d.y * inv, d.z * inv, d.w * inv));
    }
}
extern "C" int32_t sgx_avgpool_bwd(int32_t N, int32_t HW, int32_t C, const float* dy, float* dx, int64_t dx_ld_pix, int64_t dx_ld_img, void* stream) {
    SGX_CHECK_ARG(dy && dx && C % 4 == 0, "avgpool_bwd: bad args");
    SGX_CHECK_ARG(dx_ld_pix % 4 == 0 && dx_ld_img % 4 == 0 && SGX_ALIGNED16(dy) && SGX_ALIGNED16(dx), "avgpool_bwd: strides and addresses must be multiples of 16 bytes");
    long n = (long)N * HW * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(avgpool_bwd_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, stream, N, HW, C, dy, dx, (long)dx_ld_pix,
               (long)dx_ld_img);
    SGX_CHECK_LAUNCH("avgpool_bwd");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// Depthwise 3x3 convolution, pad 1, stride 1 or 2 (MobileNetV2's nn.Conv2d(groups = channels)): per-channel stencils, no matrix work -
// memory-bound like the pooling kernels above.  Filter [3][3][C]: a lane reads the nine taps of its four channels as nine 16-byte loads.
//
// One geometry serves the three kernels.  A workgroup is CG channel groups (16 bytes each) x PL "columns"; a column is one output pixel
// column of a strip of TH output rows of one image.  Lane = (column, channel group), channel groups fastest: a wave reads whole contiguous
// pixel rows.  A thread walks its strip downwards and keeps the three input rows of the window in registers, so an input element is loaded
// by the threads of its (at most) three horizontal neighbours and once more per strip boundary - not nine times.  The rows the NEXT
// output row needs are requested before the current one is computed and stored.
// TH: eight rows, halved (down to two) until the launch has DW_MIN_THREADS threads - 7 x 7 x 960 at batch 64 runs 4 strips x 7 columns x
// 240 groups x 64 images = 430 080 threads (26 waves per CU); 112 x 112 x 32 at batch 64 keeps TH = 8 and has 802 816 (49 waves per CU).
// Every reduction (statistics rows, weight gradient) is per-workgroup partial rows folded in a fixed order: no atomics.
#define DW_THREADS 256
#define DW_MIN_THREADS 262144  // 256 CUs x 16 waves
struct DwGeom {
    int N, Hi, Wi, Ho, Wo, C, C4, CG, PL, TH, nstrips, ctiles;
    long items;                                // columns: N x nstrips x Wo
    long i_ld_pix, i_ld_img, o_ld_pix, o_ld_img;  // strides of the tensor the window walks / of the tensor indexed by output pixels
};
// Hi x Wi: the map the window walks, Ho x Wo: the map a column belongs to
// vec: channels per lane (4: the 3x3 kernels' float4 groups; 2: the 5x5 kernels' float2 groups - C4 then counts pairs)
static DwGeom dw_geom(int N, int Hi, int Wi, int Ho, int Wo, int C, long i_ld_pix, long i_ld_img, long o_ld_pix, long o_ld_img, long min_threads, int vec = 4) {
    DwGeom g;
    g.N = N; g.Hi = Hi; g.Wi = Wi; g.Ho = Ho; g.Wo = Wo; g.C = C; g.C4 = C / vec;
    g.ctiles = sgx_cdiv(g.C4, 64);
    g.CG = sgx_cdiv(g.C4, g.ctiles);  // (1296 channels: six strips of 54 groups, not five of 64 and one of 4)
    g.PL = DW_THREADS / g.CG;
    g.TH = 8;
    while (g.TH > 2 && (long)N * sgx_cdiv(Ho, g.TH) * Wo * g.C4 < min_threads) g.TH >>= 1;
    g.nstrips = sgx_cdiv(Ho, g.TH);
    g.items = (long)N * g.nstrips * Wo;
    g.i_ld_pix = i_ld_pix; g.i_ld_img = i_ld_img; g.o_ld_pix = o_ld_pix; g.o_ld_img = o_ld_img;
    return g;
}
struct DwCol {
    int img, strip, col;
};
__device__ __forceinline__ DwCol dw_column(const DwGeom& g, long item) {
    DwCol k;
    k.col = (int)(item % g.Wo);
    const long t = item / g.Wo;
    k.strip = (int)(t % g.nstrips);
    k.img = (int)(t / g.nstrips);
    return k;
}
// the three window columns wi0 .. wi0 + 2 of input row hi (zeros outside the map, or when !on)
__device__ __forceinline__ void dw_ldrow(const float* __restrict__ xb, const DwGeom& g, int hi, int wi0, bool on, float4 (&r)[3]) {
    const bool ok = on && hi >= 0 && hi < g.Hi;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int wi = wi0 + s;
        r[s] = (ok && wi >= 0 && wi < g.Wi) ? sgx_ld4(xb + ((long)hi * g.Wi + wi) * g.i_ld_pix) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void dw_fma(float4& a, const float4& x, const float4& w) {
    a.x = fmaf(x.x, w.x, a.x); a.y = fmaf(x.y, w.y, a.y); a.z = fmaf(x.z, w.z, a.z); a.w = fmaf(x.w, w.w, a.w);
}
__device__ __forceinline__ void dw_put(float* p, float4 v, int accumulate) {
    if (accumulate) {
        const float4 u = sgx_ld4(p);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    sgx_st4(p, v);
}
// per-workgroup partial row of `q`: the PL column lanes of a channel group meet in LDS and are added in lane order, in double
__device__ __forceinline__ void dw_fold_store(float4 (&red)[DW_THREADS], const DwGeom& g, int tid, int cg, int pl, bool lane_ok, float4 q, float* dst) {
    red[tid] = q;
    __syncthreads();
    if (lane_ok && pl == 0) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < g.PL; ++k) {
            const float4 a = red[k * g.CG + cg];
            s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
        }
        sgx_st4(dst, make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]));
    }
    __syncthreads();
}

// y = act(dwconv(x, w) + bias); flip: the taps in reverse order (the stride-1 data gradient is this kernel on dy); accumulate: y += ...;
// partials: [2][gridDim.x][C] sum / sum of squares of the value before bias and activation.
template <int ST>
__global__ __launch_bounds__(DW_THREADS) void dwconv_fwd_kernel(DwGeom g, const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y, int act, int flip, int accumulate,
                                                                float* __restrict__ partials) {
    __shared__ float4 red[DW_THREADS];
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c4 = blockIdx.y * g.CG + cg, c = c4 * 4;
    const long item = (long)blockIdx.x * g.PL + pl;
    const bool lane_ok = pl < g.PL && c4 < g.C4;
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    if (lane_ok && item < g.items) {
        const DwCol k = dw_column(g, item);
        float4 wt[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t] = sgx_ld4(w + (long)(flip ? 8 - t : t) * g.C + c);
        const float4 b = bias ? sgx_ld4(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* __restrict__ xb = x + (long)k.img * g.i_ld_img + c;
        float* __restrict__ yb = y + (long)k.img * g.o_ld_img + c;
        const int wi0 = k.col * ST - 1;
        const int ho0 = k.strip * g.TH, ho1 = min(g.Ho, ho0 + g.TH);
        float4 r0[3], r1[3], r2[3], n1[3], n2[3];
        dw_ldrow(xb, g, ho0 * ST - 1, wi0, true, r0);
        dw_ldrow(xb, g, ho0 * ST, wi0, true, r1);
        dw_ldrow(xb, g, ho0 * ST + 1, wi0, true, r2);
        for (int ho = ho0; ho < ho1; ++ho) {
            const bool more = ho + 1 < ho1;
            const int hn = (ho + 1) * ST - 1;  // first window row of the next output row
            if (ST == 2) dw_ldrow(xb, g, hn + 1, wi0, more, n1);
            dw_ldrow(xb, g, hn + 2, wi0, more, n2);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int s = 0; s < 3; ++s) dw_fma(v, r0[s], wt[s]);
#pragma unroll
            for (int s = 0; s < 3; ++s) dw_fma(v, r1[s], wt[3 + s]);
#pragma unroll
            for (int s = 0; s < 3; ++s) dw_fma(v, r2[s], wt[6 + s]);
            q0.x += v.x; q0.y += v.y; q0.z += v.z; q0.w += v.w;
            q1.x += v.x * v.x; q1.y += v.y * v.y; q1.z += v.z * v.z; q1.w += v.w * v.w;
            float* yp = yb + ((long)ho * g.Wo + k.col) * g.o_ld_pix;
            if (accumulate) {
                const float4 u = sgx_ld4(yp);
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            sgx_st4(yp, make_float4(sgx_act6(v.x, act), sgx_act6(v.y, act), sgx_act6(v.z, act), sgx_act6(v.w, act)));
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (ST == 1) { r0[s] = r1[s]; r1[s] = r2[s]; }
                else { r0[s] = r2[s]; r1[s] = n1[s]; }
                r2[s] = n2[s];
            }
        }
    }
    if (partials) {
        dw_fold_store(red, g, tid, cg, pl, lane_ok, q0, partials + (long)blockIdx.x * g.C + c);
        dw_fold_store(red, g, tid, cg, pl, lane_ok, q1, partials + ((long)gridDim.x + blockIdx.x) * g.C + c);
    }
}

// Data gradient at stride 2, gather form.  Column = (image, strip of TH input rows, input column wi).  dx(hi, wi) takes the taps whose
// output position exists: rows r with (hi + 1 - r) even, columns s with (wi + 1 - s) even.  Even wi: s = 1 at wo = wi / 2; odd wi: s = 2
// at wo = (wi - 1) / 2 and s = 0 at wo = (wi + 1) / 2 - so a thread reads one or two dy columns (A, B).  Even hi = 2k: r = 1 at ho = k;
// odd hi = 2k + 1: r = 2 at ho = k and r = 0 at ho = k + 1 - walking down, every dy row is loaded once per strip and used for three dx rows.
__global__ __launch_bounds__(DW_THREADS) void dwconv_bwd_data_s2_kernel(DwGeom g, const float* __restrict__ dy, const float* __restrict__ w,
                                                                        float* __restrict__ dx, int accumulate) {
    // here g.Hi x g.Wi is the dy map (the rows the window walks) and g.Ho x g.Wo the dx map (TH even: strips start at even rows)
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c4 = blockIdx.y * g.CG + cg, c = c4 * 4;
    const long item = (long)blockIdx.x * g.PL + pl;
    if (!(pl < g.PL && c4 < g.C4 && item < g.items)) return;
    const DwCol k = dw_column(g, item);
    const int wi = k.col, odd = wi & 1;
    const int colA = wi >> 1, colB = (wi + 1) >> 1, sA = odd ? 2 : 1;
    const bool vB = odd && colB < g.Wi;
    float4 wA[3], wB[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        wA[r] = sgx_ld4(w + (long)(r * 3 + sA) * g.C + c);
        wB[r] = sgx_ld4(w + (long)(r * 3) * g.C + c);
    }
    const float* __restrict__ gb = dy + (long)k.img * g.i_ld_img + c;
    float* __restrict__ xb = dx + (long)k.img * g.o_ld_img + c;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const int hi0 = k.strip * g.TH, hi1 = min(g.Ho, hi0 + g.TH);
    const float* pA = gb + (long)colA * g.i_ld_pix;
    const float* pB = gb + (long)colB * g.i_ld_pix;
    const long row_ld = (long)g.Wi * g.i_ld_pix;
    float* px = xb + (long)wi * g.o_ld_pix;
    const long xrow_ld = (long)g.Wo * g.o_ld_pix;
    int ho = hi0 >> 1;
    float4 aA = sgx_ld4(pA + ho * row_ld), aB = vB ? sgx_ld4(pB + ho * row_ld) : z;  // (row hi0 / 2 always exists)
    for (int hi = hi0; hi < hi1; hi += 2, ++ho) {
        const bool two = hi + 1 < hi1, nxt = two && ho + 1 < g.Hi;
        const float4 bA = nxt ? sgx_ld4(pA + (ho + 1) * row_ld) : z, bB = (nxt && vB) ? sgx_ld4(pB + (ho + 1) * row_ld) : z;
        float4 v = z;
        dw_fma(v, aA, wA[1]);
        dw_fma(v, aB, wB[1]);
        dw_put(px + hi * xrow_ld, v, accumulate);
        if (two) {
            float4 u = z;
            dw_fma(u, bA, wA[0]);
            dw_fma(u, bB, wB[0]);
            dw_fma(u, aA, wA[2]);
            dw_fma(u, aB, wB[2]);
            dw_put(px + (hi + 1) * xrow_ld, u, accumulate);
        }
        aA = bA; aB = bB;
    }
}

// Weight gradient, stage 1: a workgroup owns the columns [blockIdx.x * per_blk, ...) and leaves ONE partial row [9][C] of its channel strip:
// ws[blockIdx.x][tap][c] = sum over its pixels of dy * x(tap).  A thread walks its columns' strips with the forward kernel's window.
template <int ST>
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_kernel(DwGeom g, long per_blk, const float* __restrict__ x, const float* __restrict__ dy,
                                                                  float* __restrict__ ws) {
    __shared__ float4 red[DW_THREADS];
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c4 = blockIdx.y * g.CG + cg, c = c4 * 4;
    const bool lane_ok = pl < g.PL && c4 < g.C4;
    float4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane_ok) {
        const long i0 = (long)blockIdx.x * per_blk, i1 = i0 + per_blk < g.items ? i0 + per_blk : g.items;
        for (long item = i0 + pl; item < i1; item += g.PL) {
            const DwCol k = dw_column(g, item);
            const float* __restrict__ xb = x + (long)k.img * g.i_ld_img + c;
            const float* __restrict__ gb = dy + (long)k.img * g.o_ld_img + c;
            const int wi0 = k.col * ST - 1;
            const int ho0 = k.strip * g.TH, ho1 = min(g.Ho, ho0 + g.TH);
            float4 r0[3], r1[3], r2[3];
            dw_ldrow(xb, g, ho0 * ST - 1, wi0, true, r0);
            if (ST == 1) dw_ldrow(xb, g, ho0, wi0, true, r1);
            for (int ho = ho0; ho < ho1; ++ho) {
                if (ST == 2) dw_ldrow(xb, g, ho * 2, wi0, true, r1);
                dw_ldrow(xb, g, ho * ST + 1, wi0, true, r2);
                const float4 d = sgx_ld4(gb + ((long)ho * g.Wo + k.col) * g.o_ld_pix);
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    dw_fma(acc[s], r0[s], d);
                    dw_fma(acc[3 + s], r1[s], d);
                    dw_fma(acc[6 + s], r2[s], d);
                }
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (ST == 1) { r0[s] = r1[s]; r1[s] = r2[s]; }
                    else r0[s] = r2[s];
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) dw_fold_store(red, g, tid, cg, pl, lane_ok, acc[t], ws + ((long)blockIdx.x * 9 + t) * g.C + c);
}
// stage 2: dw[col] += sum over the nblk partial rows, in double, in a fixed order (64 row lanes x 4 column groups per workgroup: a lane adds
// its rows ascending, the lanes meet in LDS and are added in lane order)
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_fold_kernel(const float* __restrict__ ws, int nblk, int ncol, float* __restrict__ dw) {
    __shared__ double red[64][4][4];
    const int cgp = threadIdx.x & 3, rl = threadIdx.x >> 2;
    const int col = (blockIdx.x * 4 + cgp) * 4;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < ncol)
        for (int b = rl; b < nblk; b += 64) {
            const float4 v = sgx_ld4(ws + (long)b * ncol + col);
            a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[rl][cgp][j] = a[j];
    __syncthreads();
    if (rl == 0 && col < ncol) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 64; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] += red[k][cgp][j];
        const float4 u = sgx_ld4(dw + col);
        sgx_st4(dw + col, make_float4(u.x + (float)t[0], u.y + (float)t[1], u.z + (float)t[2], u.w + (float)t[3]));
    }
}

#define DW_ALIGNED(p) SGX_ALIGNED16(p)
static int32_t dw_check(const sgx_conv_desc* d, const char* what, int k = 3) {
    SGX_CHECK_ARG(d, "%s: null descriptor", what);
    SGX_CHECK_ARG(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0, "%s: bad dims N=%d H=%d W=%d C=%d", what, d->N, d->H, d->W, d->C);
    SGX_CHECK_ARG(d->C % 4 == 0, "%s: C=%d must be a multiple of 4 (16-byte channel groups)", what, d->C);
    SGX_CHECK_ARG(d->K == d->C, "%s: depthwise means K == C (one filter per channel), got K=%d C=%d", what, d->K, d->C);
    if (k == 3) SGX_CHECK_ARG(d->R == 3 && d->S == 3 && d->pad == 1, "%s: only the 3x3 pad-1 filter is built, got R=%d S=%d pad=%d", what, d->R, d->S, d->pad);
    else SGX_CHECK_ARG(d->R == k && d->S == k && d->pad == k / 2, "%s: the %dx%d pad-%d filter, got R=%d S=%d pad=%d", what, k, k, k / 2, d->R, d->S, d->pad);
    SGX_CHECK_ARG(d->stride == 1 || d->stride == 2, "%s: stride %d is not built (1 or 2)", what, d->stride);
    SGX_CHECK_ARG(d->Ho == (d->H - 1) / d->stride + 1 && d->Wo == (d->W - 1) / d->stride + 1, "%s: Ho/Wo do not match (H+2p-R)/s+1", what);
    SGX_CHECK_ARG(d->x_ld_pix >= d->C && d->y_ld_pix >= d->C && d->x_ld_pix % 4 == 0 && d->y_ld_pix % 4 == 0 && d->x_ld_img % 4 == 0 && d->y_ld_img % 4 == 0,
                  "%s: pixel / image strides must be multiples of 4 floats and at least C", what);
    SGX_CHECK_ARG((long)d->N * d->H * d->W < 0x7fffffffL, "%s: more than 2^31 pixels", what);
    return SGX_OK;
}
static DwGeom dw_fwd_geom(const sgx_conv_desc* d) {
    return dw_geom(d->N, d->H, d->W, d->Ho, d->Wo, d->C, d->x_ld_pix, d->x_ld_img, d->y_ld_pix, d->y_ld_img, DW_MIN_THREADS);
}
static dim3 dw_grid(const DwGeom& g) { return dim3((unsigned)sgx_cdiv(g.items, g.PL), (unsigned)g.ctiles); }

extern "C" int32_t sgx_dwconv3x3_stat_blocks(const sgx_conv_desc* d) {
    if (dw_check(d, "dwconv3x3_stat_blocks")) return 0;
    const DwGeom g = dw_fwd_geom(d);
    return (int32_t)sgx_cdiv(g.items, g.PL);
}
extern "C" int32_t sgx_dwconv3x3_fwd(const sgx_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int32_t act,
                                     float* stat_partials, void* stream) {
    int32_t rc = dw_check(d, "dwconv3x3_fwd");
    if (rc) return rc;
    SGX_CHECK_ARG(x && w && y, "dwconv3x3_fwd: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(w) && DW_ALIGNED(y) && DW_ALIGNED(bias) && DW_ALIGNED(stat_partials), "dwconv3x3_fwd: operands must be 16-byte aligned");
    SGX_CHECK_ACT4(act, "dwconv3x3_fwd");
    SGX_CHECK_ARG(!stat_partials || (!bias && act == SGX_ACT_NONE), "dwconv3x3_fwd: statistics rows go with the plain convolution (no bias, no activation)");
    const DwGeom g = dw_fwd_geom(d);
    if (d->stride == 1) SGX_LAUNCH(dwconv_fwd_kernel<1>, dw_grid(g), dim3(DW_THREADS), 0, stream, g, x, w, bias, y, act, 0, 0, stat_partials);
    else SGX_LAUNCH(dwconv_fwd_kernel<2>, dw_grid(g), dim3(DW_THREADS), 0, stream, g, x, w, bias, y, act, 0, 0, stat_partials);
    SGX_CHECK_LAUNCH("dwconv3x3_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_dwconv3x3_bwd_data(const sgx_conv_desc* d, const float* dy, const float* w, float* dx, int32_t accumulate, void* stream) {
    int32_t rc = dw_check(d, "dwconv3x3_bwd_data");
    if (rc) return rc;
    SGX_CHECK_ARG(dy && w && dx, "dwconv3x3_bwd_data: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(dy) && DW_ALIGNED(w) && DW_ALIGNED(dx), "dwconv3x3_bwd_data: operands must be 16-byte aligned");
    // columns are dx pixels; the window walks dy
    const DwGeom g = dw_geom(d->N, d->Ho, d->Wo, d->H, d->W, d->C, d->y_ld_pix, d->y_ld_img, d->x_ld_pix, d->x_ld_img, DW_MIN_THREADS);
    if (d->stride == 1) {  // a 3x3 pad-1 convolution of dy with the taps reversed
        SGX_LAUNCH(dwconv_fwd_kernel<1>, dw_grid(g), dim3(DW_THREADS), 0, stream, g, dy, w, (const float*)nullptr, dx, SGX_ACT_NONE, 1, accumulate ? 1 : 0,
                   (float*)nullptr);
    } else {
        SGX_LAUNCH(dwconv_bwd_data_s2_kernel, dw_grid(g), dim3(DW_THREADS), 0, stream, g, dy, w, dx, accumulate ? 1 : 0);
    }
    SGX_CHECK_LAUNCH("dwconv3x3_bwd_data");
    return SGX_OK;
}
// weight gradient: ~1024 workgroups (four per CU) unless the problem has fewer columns - every workgroup leaves a [9][C-strip] partial row,
// so more of them only adds traffic (7 x 7 x 960 at batch 64: 112 row blocks, 3.9 MB of partials beside 24 MB of operands)
#define DW_WGRAD_MIN_THREADS 65536
#define DW_WGRAD_BLOCKS 1024
static DwGeom dw_wgrad_geom(const sgx_conv_desc* d, int* nblk, long* per_blk) {
    const DwGeom g = dw_geom(d->N, d->H, d->W, d->Ho, d->Wo, d->C, d->x_ld_pix, d->x_ld_img, d->y_ld_pix, d->y_ld_img, DW_WGRAD_MIN_THREADS);
    long n = sgx_cdiv(g.items, g.PL);
    // (SGX_STRIDE_GRID is made for grid-stride kernels whose result does not depend on the workgroup count.  Here it is borrowed to cap the
    // row blocks at two on the host emulation - every emulated workgroup pays eighteen 256-thread barriers in the fold - and that DOES
    // change the partition of the sum: the weight gradient's bits differ between chip and emulation (each is deterministic), and the fold
    // kernel's loop over more than 64 rows runs on the chip only.)
    const long cap = SGX_STRIDE_GRID(sgx_cdiv(DW_WGRAD_BLOCKS, g.ctiles));
    if (n > cap) n = cap;
    *per_blk = (g.items + n - 1) / n;
    *nblk = sgx_cdiv(g.items, *per_blk);
    return g;
}
extern "C" int64_t sgx_dwconv3x3_bwd_weight_workspace(const sgx_conv_desc* d) {
    if (dw_check(d, "dwconv3x3_bwd_weight_workspace")) return 0;
    int nblk;
    long per_blk;
    dw_wgrad_geom(d, &nblk, &per_blk);
    return (int64_t)nblk * 9 * d->C * (int64_t)sizeof(float);
}
extern "C" int32_t sgx_dwconv3x3_bwd_weight(const sgx_conv_desc* d, const float* x, const float* dy, float* dw, void* ws, int64_t ws_bytes,
                                            void* stream) {
    int32_t rc = dw_check(d, "dwconv3x3_bwd_weight");
    if (rc) return rc;
    SGX_CHECK_ARG(x && dy && dw, "dwconv3x3_bwd_weight: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(dy) && DW_ALIGNED(dw), "dwconv3x3_bwd_weight: operands must be 16-byte aligned");
    int nblk;
    long per_blk;
    const DwGeom g = dw_wgrad_geom(d, &nblk, &per_blk);
    if (!ws || ws_bytes < (int64_t)nblk * 9 * d->C * (int64_t)sizeof(float) || ((uintptr_t)ws % 16) != 0)
        SGX_FAIL(SGX_ERR_WORKSPACE, "dwconv3x3_bwd_weight: workspace too small or unaligned (sgx_dwconv3x3_bwd_weight_workspace)");
    const dim3 grid((unsigned)nblk, (unsigned)g.ctiles);
    if (d->stride == 1) SGX_LAUNCH(dwconv_wgrad_kernel<1>, grid, dim3(DW_THREADS), 0, stream, g, per_blk, x, dy, (float*)ws);
    else SGX_LAUNCH(dwconv_wgrad_kernel<2>, grid, dim3(DW_THREADS), 0, stream, g, per_blk, x, dy, (float*)ws);
    SGX_CHECK_LAUNCH("dwconv3x3_bwd_weight");
    SGX_LAUNCH(dwconv_wgrad_fold_kernel, dim3((unsigned)sgx_cdiv(9L * d->C, 16)), dim3(DW_THREADS), 0, stream, (const float*)ws, nblk, 9 * d->C, dw);
    SGX_CHECK_LAUNCH("dwconv3x3_bwd_weight (fold)");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// Depthwise 5x5 convolution, pad 2, stride 1 or 2 (MobileNetV3's nn.Conv2d(C, C, 5, stride, 2, groups = C)).  Filter [5][5][C].
// The 3x3 scheme (window rows and taps in registers, one float4 channel group per lane) would need 25 + 25 float4s: 200 registers before
// any addressing.  Two forms of the forward are built (DESIGN.md 16.5 has the measurements that chose between them):
//   register window: the same geometry and walk with TWO channels per lane (float2 groups: 25 + 25 float2s, 100 registers; a wave still
//     reads contiguous pixel rows, 512 bytes per 64 lanes); also the stride-1 data gradient (reversed taps) and, with its 25 accumulators,
//     the weight gradient;
//   LDS patch: a workgroup owns a TH x TW tile of output pixels of CG float4 channel groups, stages the (TH * stride + 4) x (TW * stride + 4)
//     input patch once (zeros outside the map) and every lane reads its 25 window elements from LDS - each input element is fetched from
//     global memory once per workgroup; the taps stay in registers (25 float4s).
// The stride-2 data gradient is a gather over the taps of matching parity: three or two per axis.
#define DW5_K 5
#define DW5_TAPS 25
__device__ __forceinline__ float2 dw_ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }
__device__ __forceinline__ void dw_st2(float* p, float2 v) { *reinterpret_cast<float2*>(p) = v; }
__device__ __forceinline__ void dw_fma2(float2& a, const float2& x, const float2& w) {
    a.x = fmaf(x.x, w.x, a.x); a.y = fmaf(x.y, w.y, a.y);
}
// the five window columns wi0 .. wi0 + 4 of input row hi (zeros outside the map, or when !on)
__device__ __forceinline__ void dw5_ldrow(const float* __restrict__ xb, const DwGeom& g, int hi, int wi0, bool on, float2 (&r)[DW5_K]) {
    const bool ok = on && hi >= 0 && hi < g.Hi;
#pragma unroll
    for (int s = 0; s < DW5_K; ++s) {
        const int wi = wi0 + s;
        r[s] = (ok && wi >= 0 && wi < g.Wi) ? dw_ld2(xb + ((long)hi * g.Wi + wi) * g.i_ld_pix) : make_float2(0.f, 0.f);
    }
}
__device__ __forceinline__ void dw2_fold_store(float2 (&red)[DW_THREADS], const DwGeom& g, int tid, int cg, int pl, bool lane_ok, float2 q, float* dst) {
    red[tid] = q;
    __syncthreads();
    if (lane_ok && pl == 0) {
        double s[2] = {0.0, 0.0};
        for (int k = 0; k < g.PL; ++k) {
            const float2 a = red[k * g.CG + cg];
            s[0] += a.x; s[1] += a.y;
        }
        dw_st2(dst, make_float2((float)s[0], (float)s[1]));
    }
    __syncthreads();
}

// Register-window forward (see dwconv_fwd_kernel: the same arguments and walk; g.C4 counts channel PAIRS here).
template <int ST>
__global__ __launch_bounds__(DW_THREADS) void dwconv5_fwd_kernel(DwGeom g, const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ y, int act, int flip, int accumulate,
                                                                 float* __restrict__ partials) {
    __shared__ float2 red[DW_THREADS];
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c2 = blockIdx.y * g.CG + cg, c = c2 * 2;
    const long item = (long)blockIdx.x * g.PL + pl;
    const bool lane_ok = pl < g.PL && c2 < g.C4;
    float2 q0 = make_float2(0.f, 0.f), q1 = q0;
    if (lane_ok && item < g.items) {
        const DwCol k = dw_column(g, item);
        float2 wt[DW5_TAPS];
#pragma unroll
        for (int t = 0; t < DW5_TAPS; ++t) wt[t] = dw_ld2(w + (long)(flip ? DW5_TAPS - 1 - t : t) * g.C + c);
        const float2 b = bias ? dw_ld2(bias + c) : make_float2(0.f, 0.f);
        const float* __restrict__ xb = x + (long)k.img * g.i_ld_img + c;
        float* __restrict__ yb = y + (long)k.img * g.o_ld_img + c;
        const int wi0 = k.col * ST - 2;
        const int ho0 = k.strip * g.TH, ho1 = min(g.Ho, ho0 + g.TH);
        float2 r[DW5_K][DW5_K], nx[ST][DW5_K];
#pragma unroll
        for (int i = 0; i < DW5_K; ++i) dw5_ldrow(xb, g, ho0 * ST - 2 + i, wi0, true, r[i]);
        for (int ho = ho0; ho < ho1; ++ho) {
            const bool more = ho + 1 < ho1;
            const int hn = (ho + 1) * ST - 2;  // first window row of the next output row: its last ST rows are new
#pragma unroll
            for (int u = 0; u < ST; ++u) dw5_ldrow(xb, g, hn + DW5_K - ST + u, wi0, more, nx[u]);
            float2 v = make_float2(0.f, 0.f);
#pragma unroll
            for (int i = 0; i < DW5_K; ++i)
#pragma unroll
                for (int s = 0; s < DW5_K; ++s) dw_fma2(v, r[i][s], wt[i * DW5_K + s]);
            q0.x += v.x; q0.y += v.y;
            q1.x += v.x * v.x; q1.y += v.y * v.y;
            float* yp = yb + ((long)ho * g.Wo + k.col) * g.o_ld_pix;
            if (accumulate) {
                const float2 u = dw_ld2(yp);
                v.x += u.x; v.y += u.y;
            }
            v.x += b.x; v.y += b.y;
            dw_st2(yp, make_float2(sgx_act6(v.x, act), sgx_act6(v.y, act)));
#pragma unroll
            for (int s = 0; s < DW5_K; ++s) {
#pragma unroll
                for (int i = 0; i < DW5_K - ST; ++i) r[i][s] = r[i + ST][s];
#pragma unroll
                for (int u = 0; u < ST; ++u) r[DW5_K - ST + u][s] = nx[u][s];
            }
        }
    }
    if (partials) {
        dw2_fold_store(red, g, tid, cg, pl, lane_ok, q0, partials + (long)blockIdx.x * g.C + c);
        dw2_fold_store(red, g, tid, cg, pl, lane_ok, q1, partials + ((long)gridDim.x + blockIdx.x) * g.C + c);
    }
}

// LDS-patch forward.  Tile geometry: b carries the strides, extents and CG / PL / TH / nstrips / ctiles (C4 = float4 groups, lane = (pixel
// lane, channel group), channel groups fastest); TW output columns per tile, wtiles of them per row, patch PH x PW pixels.
struct Dw5Tile {
    DwGeom b;
    int TW, wtiles, PH, PW;
};
#define DW5_LDS_CG 8  // float4 channel groups per workgroup: 128 contiguous bytes per pixel, 12 x 20 x 128 B = 30 KB of patch
template <int ST>
__global__ __launch_bounds__(DW_THREADS) void dwconv5_fwd_lds_kernel(Dw5Tile t, const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, float* __restrict__ y, int act,
                                                                     float* __restrict__ partials) {
    SGX_DYN_SMEM(float, patch);  // [PH][PW][CG] float4
    __shared__ float4 red[DW_THREADS];
    const DwGeom& g = t.b;
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c4 = blockIdx.y * g.CG + cg, c = c4 * 4;
    const bool lane_ok = pl < g.PL && c4 < g.C4;
    const int wt_i = blockIdx.x % t.wtiles, rest = blockIdx.x / t.wtiles;
    const int strip = rest % g.nstrips, img = rest / g.nstrips;
    const int ho0 = strip * g.TH, wo0 = wt_i * t.TW;
    const int hi0 = ho0 * ST - 2, wi0 = wo0 * ST - 2;
    if (lane_ok) {
        const float* __restrict__ xb = x + (long)img * g.i_ld_img + c;
        for (int p = pl; p < t.PH * t.PW; p += g.PL) {
            const int hi = hi0 + p / t.PW, wi = wi0 + p % t.PW;
            const bool in = hi >= 0 && hi < g.Hi && wi >= 0 && wi < g.Wi;
            sgx_st4(patch + ((long)p * g.CG + cg) * 4, in ? sgx_ld4(xb + ((long)hi * g.Wi + wi) * g.i_ld_pix) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
    }
    __syncthreads();
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    if (lane_ok) {
        float4 wt[DW5_TAPS];
#pragma unroll
        for (int k = 0; k < DW5_TAPS; ++k) wt[k] = sgx_ld4(w + (long)k * g.C + c);
        const float4 b = bias ? sgx_ld4(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        float* __restrict__ yb = y + (long)img * g.o_ld_img + c;
        for (int o = pl; o < g.TH * t.TW; o += g.PL) {
            const int orow = o / t.TW, ocol = o % t.TW;
            const int ho = ho0 + orow, wo = wo0 + ocol;
            if (ho >= g.Ho || wo >= g.Wo) continue;
            const float* pp = patch + ((long)(orow * ST * t.PW + ocol * ST) * g.CG + cg) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < DW5_K; ++i)
#pragma unroll
                for (int s = 0; s < DW5_K; ++s) dw_fma(v, sgx_ld4(pp + (long)(i * t.PW + s) * g.CG * 4), wt[i * DW5_K + s]);
            q0.x += v.x; q0.y += v.y; q0.z += v.z; q0.w += v.w;
            q1.x += v.x * v.x; q1.y += v.y * v.y; q1.z += v.z * v.z; q1.w += v.w * v.w;
            v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            sgx_st4(yb + ((long)ho * g.Wo + wo) * g.o_ld_pix, make_float4(sgx_act6(v.x, act), sgx_act6(v.y, act), sgx_act6(v.z, act), sgx_act6(v.w, act)));
        }
    }
    if (partials) {
        dw_fold_store(red, g, tid, cg, pl, lane_ok, q0, partials + (long)blockIdx.x * g.C + c);
        dw_fold_store(red, g, tid, cg, pl, lane_ok, q1, partials + ((long)gridDim.x + blockIdx.x) * g.C + c);
    }
}

// Data gradient at stride 2, gather form.  Column = (image, strip of TH dx rows, dx column wi); g.Hi x g.Wi is the dy map, g.Ho x g.Wo the dx
// map (TH even: strips start at even rows).  dx(hi, wi) takes the taps (r, s) with ho = (hi + 2 - r) / 2, wo = (wi + 2 - s) / 2 whole:
// columns j = 0 .. 2 at wo = ((wi + 2) >> 1) - j with s = 2 j + (wi & 1) (odd wi has two); rows alike - the pair hi = 2 k, 2 k + 1 reads the dy
// rows k - 1, k, k + 1 (even: r = 4, 2, 0; odd: r = 3, 1): walking down, every dy row is loaded once per strip.
// the dy columns base, base - 1, base - 2 of row ho (zeros where the row or the column does not exist, or when !on)
__device__ __forceinline__ void dw5_ldrow_s2(const float* __restrict__ gb, const DwGeom& g, int ho, int base, unsigned cv, bool on, float2 (&a)[3]) {
    const bool ok = on && ho >= 0 && ho < g.Hi;
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = (ok && ((cv >> j) & 1u)) ? dw_ld2(gb + ((long)ho * g.Wi + (base - j)) * g.i_ld_pix) : make_float2(0.f, 0.f);
}
__global__ __launch_bounds__(DW_THREADS) void dwconv5_bwd_data_s2_kernel(DwGeom g, const float* __restrict__ dy, const float* __restrict__ w,
                                                                         float* __restrict__ dx, int accumulate) {
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c2 = blockIdx.y * g.CG + cg, c = c2 * 2;
    const long item = (long)blockIdx.x * g.PL + pl;
    if (!(pl < g.PL && c2 < g.C4 && item < g.items)) return;
    const DwCol k = dw_column(g, item);
    const int wi = k.col, po = wi & 1, base = (wi + 2) >> 1;
    const float2 z = make_float2(0.f, 0.f);
    unsigned cv = 0u;  // bit j: column j exists
    float2 wt[DW5_K][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int s = 2 * j + po;
        if (s < DW5_K && base - j >= 0 && base - j < g.Wi) cv |= 1u << j;
#pragma unroll
        for (int r = 0; r < DW5_K; ++r) wt[r][j] = s < DW5_K ? dw_ld2(w + (long)(r * DW5_K + s) * g.C + c) : z;
    }
    const float* __restrict__ gb = dy + (long)k.img * g.i_ld_img + c;
    float* px = dx + (long)k.img * g.o_ld_img + c + (long)wi * g.o_ld_pix;
    const long xrow_ld = (long)g.Wo * g.o_ld_pix;
    const int hi0 = k.strip * g.TH, hi1 = min(g.Ho, hi0 + g.TH);
    int kk = hi0 >> 1;
    float2 a0[3], a1[3], a2[3], nx[3];
    dw5_ldrow_s2(gb, g, kk - 1, base, cv, true, a0);
    dw5_ldrow_s2(gb, g, kk, base, cv, true, a1);
    dw5_ldrow_s2(gb, g, kk + 1, base, cv, true, a2);
    for (int hi = hi0; hi < hi1; hi += 2, ++kk) {
        const bool two = hi + 1 < hi1;
        dw5_ldrow_s2(gb, g, kk + 2, base, cv, hi + 2 < hi1, nx);
        float2 v = z;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dw_fma2(v, a2[j], wt[0][j]);
            dw_fma2(v, a1[j], wt[2][j]);
            dw_fma2(v, a0[j], wt[4][j]);
        }
        float* p0 = px + hi * xrow_ld;
        if (accumulate) {
            const float2 u = dw_ld2(p0);
            v.x += u.x; v.y += u.y;
        }
        dw_st2(p0, v);
        if (two) {
            float2 u = z;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dw_fma2(u, a2[j], wt[1][j]);
                dw_fma2(u, a1[j], wt[3][j]);
            }
            float* p1 = p0 + xrow_ld;
            if (accumulate) {
                const float2 o = dw_ld2(p1);
                u.x += o.x; u.y += o.y;
            }
            dw_st2(p1, u);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) { a0[j] = a1[j]; a1[j] = a2[j]; a2[j] = nx[j]; }
    }
}

// Weight gradient, stage 1 (see dwconv_wgrad_kernel): ONE partial row [25][C] per workgroup; the 25 accumulators of a lane's channel pair
// meet in LDS five taps (one filter row) at a time.  Stage 2 is dwconv_wgrad_fold_kernel over 25 * C columns.
template <int ST>
__global__ __launch_bounds__(DW_THREADS) void dwconv5_wgrad_kernel(DwGeom g, long per_blk, const float* __restrict__ x, const float* __restrict__ dy,
                                                                   float* __restrict__ ws) {
    __shared__ float2 red[DW5_K][DW_THREADS];
    const int tid = threadIdx.x, cg = tid % g.CG, pl = tid / g.CG;
    const int c2 = blockIdx.y * g.CG + cg, c = c2 * 2;
    const bool lane_ok = pl < g.PL && c2 < g.C4;
    float2 acc[DW5_TAPS];
#pragma unroll
    for (int t = 0; t < DW5_TAPS; ++t) acc[t] = make_float2(0.f, 0.f);
    if (lane_ok) {
        const long i0 = (long)blockIdx.x * per_blk, i1 = i0 + per_blk < g.items ? i0 + per_blk : g.items;
        for (long item = i0 + pl; item < i1; item += g.PL) {
            const DwCol k = dw_column(g, item);
            const float* __restrict__ xb = x + (long)k.img * g.i_ld_img + c;
            const float* __restrict__ gb = dy + (long)k.img * g.o_ld_img + c;
            const int wi0 = k.col * ST - 2;
            const int ho0 = k.strip * g.TH, ho1 = min(g.Ho, ho0 + g.TH);
            float2 r[DW5_K][DW5_K];
#pragma unroll
            for (int i = 0; i < DW5_K - ST; ++i) dw5_ldrow(xb, g, ho0 * ST - 2 + i, wi0, true, r[i]);
            for (int ho = ho0; ho < ho1; ++ho) {
#pragma unroll
                for (int u = 0; u < ST; ++u) dw5_ldrow(xb, g, ho * ST - 2 + DW5_K - ST + u, wi0, true, r[DW5_K - ST + u]);
                const float2 d = dw_ld2(gb + ((long)ho * g.Wo + k.col) * g.o_ld_pix);
#pragma unroll
                for (int i = 0; i < DW5_K; ++i)
#pragma unroll
                    for (int s = 0; s < DW5_K; ++s) dw_fma2(acc[i * DW5_K + s], r[i][s], d);
#pragma unroll
                for (int s = 0; s < DW5_K; ++s)
#pragma unroll
                    for (int i = 0; i < DW5_K - ST; ++i) r[i][s] = r[i + ST][s];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < DW5_K; ++i) {
#pragma unroll
        for (int s = 0; s < DW5_K; ++s) red[s][tid] = acc[i * DW5_K + s];
        __syncthreads();
        if (lane_ok)
            for (int s = pl; s < DW5_K; s += g.PL) {  // the column lanes share the five folds (each in lane order, in double)
                double t0 = 0.0, t1 = 0.0;
                for (int k = 0; k < g.PL; ++k) {
                    const float2 a = red[s][k * g.CG + cg];
                    t0 += a.x; t1 += a.y;
                }
                dw_st2(ws + ((long)blockIdx.x * DW5_TAPS + i * DW5_K + s) * g.C + c, make_float2((float)t0, (float)t1));
            }
        __syncthreads();
    }
}

// which forward runs: 0 the register window (the default: DESIGN.md 16.5), 1 the LDS patch - a measurement switch (tools/dwconv_bench.py)
static std::atomic<int> g_dw5_form{0};
extern "C" int32_t sgx_debug_set_dwconv5x5_form(int32_t form) {
    SGX_CHECK_ARG(form == 0 || form == 1, "debug_set_dwconv5x5_form: 0 (register window) or 1 (LDS patch), got %d", form);
    g_dw5_form = form;
    return SGX_OK;
}
static DwGeom dw5_fwd_geom(const sgx_conv_desc* d) {
    return dw_geom(d->N, d->H, d->W, d->Ho, d->Wo, d->C, d->x_ld_pix, d->x_ld_img, d->y_ld_pix, d->y_ld_img, DW_MIN_THREADS, 2);
}
static Dw5Tile dw5_tile(const sgx_conv_desc* d) {
    Dw5Tile t;
    DwGeom& g = t.b;
    g.N = d->N; g.Hi = d->H; g.Wi = d->W; g.Ho = d->Ho; g.Wo = d->Wo; g.C = d->C; g.C4 = d->C / 4;
    g.ctiles = sgx_cdiv(g.C4, DW5_LDS_CG);
    g.CG = sgx_cdiv(g.C4, g.ctiles);
    g.PL = DW_THREADS / g.CG;
    g.TH = d->stride == 1 ? 8 : 4;
    t.TW = d->stride == 1 ? 16 : 8;
    if (t.TW > g.Wo) t.TW = g.Wo;
    t.wtiles = sgx_cdiv(g.Wo, t.TW);
    while (g.TH > 2 && (long)d->N * sgx_cdiv(g.Ho, g.TH) * t.wtiles * g.ctiles * DW_THREADS < DW_MIN_THREADS) g.TH >>= 1;
    g.nstrips = sgx_cdiv(g.Ho, g.TH);
    g.items = (long)d->N * g.nstrips * t.wtiles;  // workgroups per channel tile
    t.PH = g.TH * d->stride + 4;
    t.PW = t.TW * d->stride + 4;
    g.i_ld_pix = d->x_ld_pix; g.i_ld_img = d->x_ld_img; g.o_ld_pix = d->y_ld_pix; g.o_ld_img = d->y_ld_img;
    return t;
}
static int32_t dw5_lds_ok(const Dw5Tile& t, const char* what) {
    SGX_CHECK_ARG(t.b.items < 0x7fffffffL && (long)t.PH * t.PW * t.b.CG * 16 <= 65536, "%s: tile outside the launch limits", what);
    return SGX_OK;
}

extern "C" int32_t sgx_dwconv5x5_stat_blocks(const sgx_conv_desc* d) {
    if (dw_check(d, "dwconv5x5_stat_blocks", 5)) return 0;
    if (g_dw5_form == 1) return (int32_t)dw5_tile(d).b.items;
    const DwGeom g = dw5_fwd_geom(d);
    return (int32_t)sgx_cdiv(g.items, g.PL);
}
extern "C" int32_t sgx_dwconv5x5_fwd(const sgx_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int32_t act,
                                     float* stat_partials, void* stream) {
    int32_t rc = dw_check(d, "dwconv5x5_fwd", 5);
    if (rc) return rc;
    SGX_CHECK_ARG(x && w && y, "dwconv5x5_fwd: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(w) && DW_ALIGNED(y) && DW_ALIGNED(bias) && DW_ALIGNED(stat_partials), "dwconv5x5_fwd: operands must be 16-byte aligned");
    SGX_CHECK_ACT4(act, "dwconv5x5_fwd");
    SGX_CHECK_ARG(!stat_partials || (!bias && act == SGX_ACT_NONE), "dwconv5x5_fwd: statistics rows go with the plain convolution (no bias, no activation)");
    if (g_dw5_form == 1) {
        const Dw5Tile t = dw5_tile(d);
        rc = dw5_lds_ok(t, "dwconv5x5_fwd");
        if (rc) return rc;
        const dim3 grid((unsigned)t.b.items, (unsigned)t.b.ctiles);
        const unsigned lds = (unsigned)((long)t.PH * t.PW * t.b.CG * 16);
        if (d->stride == 1) SGX_LAUNCH(dwconv5_fwd_lds_kernel<1>, grid, dim3(DW_THREADS), lds, stream, t, x, w, bias, y, act, stat_partials);
        else SGX_LAUNCH(dwconv5_fwd_lds_kernel<2>, grid, dim3(DW_THREADS), lds, stream, t, x, w, bias, y, act, stat_partials);
        SGX_CHECK_LAUNCH("dwconv5x5_fwd (LDS patch)");
        return SGX_OK;
    }
    const DwGeom g = dw5_fwd_geom(d);
    if (d->stride == 1) SGX_LAUNCH(dwconv5_fwd_kernel<1>, dw_grid(g), dim3(DW_THREADS), 0, stream, g, x, w, bias, y, act, 0, 0, stat_partials);
    else SGX_LAUNCH(dwconv5_fwd_kernel<2>, dw_grid(g), dim3(DW_THREADS), 0, stream, g, x, w, bias, y, act, 0, 0, stat_partials);
    SGX_CHECK_LAUNCH("dwconv5x5_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_dwconv5x5_bwd_data(const sgx_conv_desc* d, const float* dy, const float* w, float* dx, int32_t accumulate, void* stream) {
    int32_t rc = dw_check(d, "dwconv5x5_bwd_data", 5);
    if (rc) return rc;
    SGX_CHECK_ARG(dy && w && dx, "dwconv5x5_bwd_data: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(dy) && DW_ALIGNED(w) && DW_ALIGNED(dx), "dwconv5x5_bwd_data: operands must be 16-byte aligned");
    // columns are dx pixels; the window walks dy
    const DwGeom g = dw_geom(d->N, d->Ho, d->Wo, d->H, d->W, d->C, d->y_ld_pix, d->y_ld_img, d->x_ld_pix, d->x_ld_img, DW_MIN_THREADS, 2);
    if (d->stride == 1) {  // a 5x5 pad-2 convolution of dy with the taps reversed
        SGX_LAUNCH(dwconv5_fwd_kernel<1>, dw_grid(g), dim3(DW_THREADS), 0, stream, g, dy, w, (const float*)nullptr, dx, SGX_ACT_NONE, 1, accumulate ? 1 : 0,
                   (float*)nullptr);
    } else {
        SGX_LAUNCH(dwconv5_bwd_data_s2_kernel, dw_grid(g), dim3(DW_THREADS), 0, stream, g, dy, w, dx, accumulate ? 1 : 0);
    }
    SGX_CHECK_LAUNCH("dwconv5x5_bwd_data");
    return SGX_OK;
}
static DwGeom dw5_wgrad_geom(const sgx_conv_desc* d, int* nblk, long* per_blk) {
    const DwGeom g = dw_geom(d->N, d->H, d->W, d->Ho, d->Wo, d->C, d->x_ld_pix, d->x_ld_img, d->y_ld_pix, d->y_ld_img, DW_WGRAD_MIN_THREADS, 2);
    long n = sgx_cdiv(g.items, g.PL);
    const long cap = SGX_STRIDE_GRID(sgx_cdiv(DW_WGRAD_BLOCKS, g.ctiles));  // (see dw_wgrad_geom: two row blocks on the host emulation)
    if (n > cap) n = cap;
    *per_blk = (g.items + n - 1) / n;
    *nblk = sgx_cdiv(g.items, *per_blk);
    return g;
}
extern "C" int64_t sgx_dwconv5x5_bwd_weight_workspace(const sgx_conv_desc* d) {
    if (dw_check(d, "dwconv5x5_bwd_weight_workspace", 5)) return 0;
    int nblk;
    long per_blk;
    dw5_wgrad_geom(d, &nblk, &per_blk);
    return (int64_t)nblk * DW5_TAPS * d->C * (int64_t)sizeof(float);
}
extern "C" int32_t sgx_dwconv5x5_bwd_weight(const sgx_conv_desc* d, const float* x, const float* dy, float* dw, void* ws, int64_t ws_bytes,
                                            void* stream) {
    int32_t rc = dw_check(d, "dwconv5x5_bwd_weight", 5);
    if (rc) return rc;
    SGX_CHECK_ARG(x && dy && dw, "dwconv5x5_bwd_weight: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(dy) && DW_ALIGNED(dw), "dwconv5x5_bwd_weight: operands must be 16-byte aligned");
    int nblk;
    long per_blk;
    const DwGeom g = dw5_wgrad_geom(d, &nblk, &per_blk);
    if (!ws || ws_bytes < (int64_t)nblk * DW5_TAPS * d->C * (int64_t)sizeof(float) || ((uintptr_t)ws % 16) != 0)
        SGX_FAIL(SGX_ERR_WORKSPACE, "dwconv5x5_bwd_weight: workspace too small or unaligned (sgx_dwconv5x5_bwd_weight_workspace)");
    const dim3 grid((unsigned)nblk, (unsigned)g.ctiles);
    if (d->stride == 1) SGX_LAUNCH(dwconv5_wgrad_kernel<1>, grid, dim3(DW_THREADS), 0, stream, g, per_blk, x, dy, (float*)ws);
    else SGX_LAUNCH(dwconv5_wgrad_kernel<2>, grid, dim3(DW_THREADS), 0, stream, g, per_blk, x, dy, (float*)ws);
    SGX_CHECK_LAUNCH("dwconv5x5_bwd_weight");
    SGX_LAUNCH(dwconv_wgrad_fold_kernel, dim3((unsigned)sgx_cdiv((long)DW5_TAPS * d->C, 16)), dim3(DW_THREADS), 0, stream, (const float*)ws, nblk, DW5_TAPS * d->C, dw);
    SGX_CHECK_LAUNCH("dwconv5x5_bwd_weight (fold)");
    return SGX_OK;
}

// Grouped 3x3 convolution (1 < groups < C): MFMA tiles over an LDS patch; shares dw_check and the weight-gradient fold above.
#include "gconv.h"
