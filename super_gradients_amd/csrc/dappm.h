// DDRNet's DAPPM context module (segmentation_models/ddrnet.py): the pooling pyramid as ONE launch per direction and the size-based bilinear
// resize with addend and BatchNorm moments.  Included by pool.hip.  The map is tiny (1/64 resolution: 16 x 32 pixels at 1024 x 2048), so
// the step is a chain of dependent launches: these kernels exist to remove links, not to move bytes faster.
//   work split   a workgroup owns ONE IMAGE x ONE CHANNEL GROUP of CG = 4 / 8 / 16 floats; lane = (pixel lane, float4 channel lane), G = CG / 4
//                channel lanes innermost, 256 / G pixel lanes.  CG (dp_pick_cg): the widest group whose LDS fits and that still leaves
//                DP_FILL_WGS workgroups; the kernels that keep no per-image sum also cut the rows into tiles (gridDim.z) to reach that count.
//   pool fwd     x's plane slab -> LDS (x is read from HBM once; its moments are taken on the way), horizontal window sums of every level
//                -> LDS, vertical sums -> the pooled maps and their moments; the global level is x's own sum.  17 + 17 LDS reads per output
//                of the widest level instead of 289 global ones.
//   pool bwd     the pooled gradients of the image x channel group -> LDS; every input pixel gathers the windows that cover it (at most
//                ceil(k / s)^2 = 9 per level), adds the global level and up to two addends, and stores dx once.
//   resize fwd   the source map -> LDS; a lane owns a float4 of one output pixel: four LDS taps, + addend, one 16-byte store, moments of y.
//   resize bwd   separable gather: T[oh][wi] = sum_ow ww(ow, wi) dy[oh][ow] -> LDS, then dz[hi][wi] = sum_oh wh(oh, hi) T[oh][wi].
// No atomics anywhere: moments are reduced over a wave's pixel lanes by a fixed butterfly, over the four waves in wave order, and leave as
// ONE partial row per workgroup in the [2][nblk][C] layout sgx_bn_finalize / sgx_bn_reduce_sums read - two calls give the same bits.
// Source coordinates and weights of the resize are ATen's (upsample_bilinear2d, align_corners=False, a size given: scale = in / out in float),
// computed in ONE function both directions call.  No matrix instructions: there is no reduction over channels here.
#pragma once

#define DP_THREADS 256
#define DP_MAX_LEVELS 3
#define DP_MAX_K 17
#define DP_MAX_S 8
#define DP_MAX_LDS (80 * 1024)  // two workgroups per CU (160 KB); above 64 KB the kernel's dynamic limit is raised once per device
#define DP_RED_FLOATS 512       // reduction scratch: 8 quantities x 4 waves x 4 channel lanes x float4
#define DP_FILL_WGS 512         // two workgroups on each of the 256 CUs
#define DP_LD4(v) ((v) % 4 == 0)
#define DP_ALIGNED(p) (((uintptr_t)(p) % 16) == 0)

struct DpLevels {
    int n, glob;
    int k[DP_MAX_LEVELS], s[DP_MAX_LEVELS], Ho[DP_MAX_LEVELS], Wo[DP_MAX_LEVELS];
};

// The widest channel group (16 / 8 / 4 floats) that divides C, whose LDS (per_ch bytes per channel + fixed) fits DP_MAX_LDS and that leaves
// DP_FILL_WGS workgroups (`units` workgroups per channel group); when none fills the chip, the narrowest that fits; 0: not even 4 floats fit.
static int dp_pick_cg(int C, long units, long per_ch, long fixed) {
    int fit = 0;
    for (int cg = 16; cg >= 4; cg >>= 1) {
        if (C % cg || per_ch * cg + fixed > DP_MAX_LDS) continue;
        fit = cg;
        if ((long)(C / cg) * units >= DP_FILL_WGS) return cg;
    }
    return fit;
}
// row tiles (gridDim.z) that bring (C / cg) * N workgroups up to DP_FILL_WGS; -> rows per tile, *tiles = the count without empty tiles
static int dp_row_tiles(int rows, int C, int cg, int N, int* tiles) {
    long want = (DP_FILL_WGS + (long)(C / cg) * N - 1) / ((long)(C / cg) * N);
    if (want > rows) want = rows;
    const int per = (rows + (int)want - 1) / (int)want;
    *tiles = (rows + per - 1) / per;
    return per;
}
#ifndef SGX_EMU
template <typename KernelT>
static bool dp_raise_lds(KernelT kernel, std::atomic<unsigned long long>& raised) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DP_MAX_LDS) != hipSuccess) return false;
        raised.fetch_or(bit, std::memory_order_release);
    }
    return true;
}
#define DP_RAISE_LDS(kernel, what)                                                                              \
    do {                                                                                                        \
        static std::atomic<unsigned long long> raised_{0};                                                      \
        if (!dp_raise_lds(kernel, raised_)) SGX_FAIL(SGX_ERR_HIP, "%s: cannot raise the kernel's dynamic LDS limit", what); \
    } while (0)
#else
#define DP_RAISE_LDS(kernel, what) ((void)0)
#endif

__device__ __forceinline__ void dp_acc(float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
__device__ __forceinline__ void dp_acc_sq(float4& q, const float4& v) { q.x += v.x * v.x; q.y += v.y * v.y; q.z += v.z * v.z; q.w += v.w * v.w; }
__device__ __forceinline__ void dp_fma(float4& s, float k, const float4& v) { s.x += k * v.x; s.y += k * v.y; s.z += k * v.z; s.w += k * v.w; }
// Sum over the pixel lanes of this wave (the lanes G apart), a butterfly in fixed order; every lane of the wave calls it.  Lanes 0 .. G-1
// then leave the wave's sum of quantity q in red[q][wave][channel lane].
__device__ __forceinline__ void dp_wave_sum(float4 v, int G, int q, float* red) {
    for (int m = G; m < 64; m <<= 1) {
        v.x += __shfl_xor(v.x, m);
        v.y += __shfl_xor(v.y, m);
        v.z += __shfl_xor(v.z, m);
        v.w += __shfl_xor(v.w, m);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < G) sgx_st4(red + ((q * 4 + wave) * 4 + lane) * 4, v);
}
// the four waves' sums of quantity q for channel lane cl, in wave order (after a barrier)
__device__ __forceinline__ float4 dp_block_sum(const float* red, int q, int cl) {
    float4 s = sgx_ld4(red + ((q * 4 + 0) * 4 + cl) * 4);
    for (int w = 1; w < 4; ++w) dp_acc(s, sgx_ld4(red + ((q * 4 + w) * 4 + cl) * 4));
    return s;
}

// ---- pyramid forward: grid (C / CG, N), LDS = [H W][CG] slab + per level [H Wo_l][CG] horizontal sums + the reduction scratch -------------
// parts (may be NULL): [T][2][N][C], tensor order x, the window levels, the global level; this workgroup writes row blockIdx.y of each.
__global__ __launch_bounds__(DP_THREADS) void dappm_pool_fwd_kernel(int H, int W, int C, int CG, DpLevels lv, const float* __restrict__ x, long x_ld_pix,
                                                                    long x_ld_img, float* __restrict__ p0, float* __restrict__ p1, float* __restrict__ p2,
                                                                    float* __restrict__ pg, float* __restrict__ parts) {
    SGX_DYN_SMEM(float, smem);
    const int G = CG / 4, P = DP_THREADS / G, cl = threadIdx.x % G, pl = threadIdx.x / G;
    const int img = blockIdx.y, N = gridDim.y, c0 = blockIdx.x * CG + cl * 4, HW = H * W;
    float* slab = smem;
    float* red = smem + (long)HW * CG;
    float* hs = red + DP_RED_FLOATS;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 sx = zero, qx = zero;
    const float* xb = x + (long)img * x_ld_img + c0;
    for (int pix = pl; pix < HW; pix += P) {
        const float4 v = sgx_ld4(xb + (long)pix * x_ld_pix);
        sgx_st4(slab + pix * CG + cl * 4, v);
        dp_acc(sx, v);
        dp_acc_sq(qx, v);
    }
    __syncthreads();
    int hoff[DP_MAX_LEVELS];
    {
        int o = 0;
#pragma unroll
        for (int l = 0; l < DP_MAX_LEVELS; ++l) {
            hoff[l] = o;
            if (l < lv.n) o += H * lv.Wo[l] * CG;
        }
    }
#pragma unroll
    for (int l = 0; l < DP_MAX_LEVELS; ++l) {  // horizontal window sums (padding = stride: the window of column wo starts at (wo - 1) s)
        if (l >= lv.n) continue;
        const int k = lv.k[l], s = lv.s[l], Wo = lv.Wo[l];
        for (int i = pl; i < H * Wo; i += P) {
            const int h = i / Wo, wo = i - h * Wo, w0 = (wo - 1) * s;
            const int lo = w0 < 0 ? 0 : w0, hi = w0 + k < W ? w0 + k : W;
            float4 a = zero;
            for (int w = lo; w < hi; ++w) dp_acc(a, sgx_ld4(slab + (h * W + w) * CG + cl * 4));
            sgx_st4(hs + hoff[l] + i * CG + cl * 4, a);
        }
    }
    __syncthreads();
    float4 sm[DP_MAX_LEVELS], qm[DP_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < DP_MAX_LEVELS; ++l) {  // vertical sums, the divisor k^2 whatever the window's clipping (count_include_pad)
        sm[l] = qm[l] = zero;
        if (l >= lv.n) continue;
        const int k = lv.k[l], s = lv.s[l], Wo = lv.Wo[l], Ho = lv.Ho[l];
        const float div = (float)(k * k);
        float* pl_out = (l == 0 ? p0 : l == 1 ? p1 : p2) + (long)img * Ho * Wo * C + c0;
        for (int i = pl; i < Ho * Wo; i += P) {
            const int ho = i / Wo, wo = i - ho * Wo, h0 = (ho - 1) * s;
            const int lo = h0 < 0 ? 0 : h0, hi = h0 + k < H ? h0 + k : H;
            float4 a = zero;
            for (int h = lo; h < hi; ++h) dp_acc(a, sgx_ld4(hs + hoff[l] + (h * Wo + wo) * CG + cl * 4));
            a = make_float4(a.x / div, a.y / div, a.z / div, a.w / div);
            sgx_st4(pl_out + (long)i * C, a);
            dp_acc(sm[l], a);
            dp_acc_sq(qm[l], a);
        }
    }
    if (!parts && !lv.glob) return;  // (uniform over the workgroup)
    dp_wave_sum(sx, G, 0, red);
    dp_wave_sum(qx, G, 1, red);
#pragma unroll
    for (int l = 0; l < DP_MAX_LEVELS; ++l) {
        if (l >= lv.n) continue;
        dp_wave_sum(sm[l], G, 2 + 2 * l, red);
        dp_wave_sum(qm[l], G, 3 + 2 * l, red);
    }
    __syncthreads();
    const int T = 1 + lv.n + (lv.glob ? 1 : 0);
    if ((int)threadIdx.x >= T * G) return;
    const int t = threadIdx.x / G, c = blockIdx.x * CG + (threadIdx.x % G) * 4;
    float4 s, q;
    if (lv.glob && t == T - 1) {  // the global level: the mean of the plane, one value per (image, channel)
        s = dp_block_sum(red, 0, threadIdx.x % G);
        const float hw = (float)HW;
        s = make_float4(s.x / hw, s.y / hw, s.z / hw, s.w / hw);
        q = make_float4(s.x * s.x, s.y * s.y, s.z * s.z, s.w * s.w);
        sgx_st4(pg + (long)img * C + c, s);
    } else {
        s = dp_block_sum(red, 2 * t, threadIdx.x % G);
        q = dp_block_sum(red, 2 * t + 1, threadIdx.x % G);
    }
    if (parts) {
        float* row = parts + ((long)t * 2 * N + img) * C + c;
        sgx_st4(row, s);
        sgx_st4(row + (long)N * C, q);
    }
}

// ---- pyramid backward: grid (C / CG, N, row tiles), LDS = the pooled gradients of the image x channel group --------------------------------
__global__ __launch_bounds__(DP_THREADS) void dappm_pool_bwd_kernel(int H, int W, int C, int CG, DpLevels lv, int rows_per_tile, const float* __restrict__ d0,
                                                                    const float* __restrict__ d1, const float* __restrict__ d2, const float* __restrict__ dg,
                                                                    const float* __restrict__ a1, long a1_ld_pix, long a1_ld_img, const float* __restrict__ a2,
                                                                    long a2_ld_pix, long a2_ld_img, float* __restrict__ dx, long dx_ld_pix, long dx_ld_img,
                                                                    int accumulate) {
    SGX_DYN_SMEM(float, smem);
    const int G = CG / 4, P = DP_THREADS / G, cl = threadIdx.x % G, pl = threadIdx.x / G;
    const int img = blockIdx.y, c0 = blockIdx.x * CG + cl * 4;
    int off[DP_MAX_LEVELS];
    {
        int o = 0;
#pragma unroll
        for (int l = 0; l < DP_MAX_LEVELS; ++l) {
            off[l] = o;
            if (l >= lv.n) continue;
            const int np = lv.Ho[l] * lv.Wo[l];
            const float* src = (l == 0 ? d0 : l == 1 ? d1 : d2) + (long)img * np * C + c0;
            for (int i = pl; i < np; i += P) sgx_st4(smem + o + i * CG + cl * 4, sgx_ld4(src + (long)i * C));
            o += np * CG;
        }
    }
    __syncthreads();
    float4 base = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lv.glob) {
        const float4 g = sgx_ld4(dg + (long)img * C + c0);
        const float hw = (float)(H * W);
        base = make_float4(g.x / hw, g.y / hw, g.z / hw, g.w / hw);
    }
    const int r0 = blockIdx.z * rows_per_tile, r1 = r0 + rows_per_tile < H ? r0 + rows_per_tile : H;
    for (int i = r0 * W + pl; i < r1 * W; i += P) {
        const int h = i / W, w = i - h * W;
        float4 acc = base;
#pragma unroll
        for (int l = 0; l < DP_MAX_LEVELS; ++l) {
            if (l >= lv.n) continue;
            // windows (ho - 1) s <= h < (ho - 1) s + k:  ho in [ceil((h + s - k + 1) / s), (h + s) / s], clipped to the pooled map
            const int k = lv.k[l], s = lv.s[l], Ho = lv.Ho[l], Wo = lv.Wo[l];
            const int tl = h + s - k + 1, ul = w + s - k + 1;
            const int hlo = tl > 0 ? (tl + s - 1) / s : 0, hhi = (h + s) / s < Ho - 1 ? (h + s) / s : Ho - 1;
            const int wlo = ul > 0 ? (ul + s - 1) / s : 0, whi = (w + s) / s < Wo - 1 ? (w + s) / s : Wo - 1;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int ho = hlo; ho <= hhi; ++ho)
                for (int wo = wlo; wo <= whi; ++wo) dp_acc(a, sgx_ld4(smem + off[l] + (ho * Wo + wo) * CG + cl * 4));
            const float div = (float)(k * k);
            acc.x += a.x / div; acc.y += a.y / div; acc.z += a.z / div; acc.w += a.w / div;
        }
        if (a1) dp_acc(acc, sgx_ld4(a1 + (long)img * a1_ld_img + (long)i * a1_ld_pix + c0));
        if (a2) dp_acc(acc, sgx_ld4(a2 + (long)img * a2_ld_img + (long)i * a2_ld_pix + c0));
        float* xp = dx + (long)img * dx_ld_img + (long)i * dx_ld_pix + c0;
        if (accumulate) dp_acc(acc, sgx_ld4(xp));
        sgx_st4(xp, acc);
    }
}

// ---- size-based bilinear resize ---------------------------------------------------------------------------------------------------------
struct RsAxis {
    int in, out;
    float scale;  // ATen's area_pixel_compute_scale with a size given and align_corners=False: in / out, in float
};
static RsAxis rs_axis(int in, int out) {
    RsAxis a;
    a.in = in; a.out = out; a.scale = (float)in / (float)out;
    return a;
}
// output index o reads inputs i0 and i1 with weights 1 - l1 and l1 (ATen's compute_source_index_and_lambda)
__device__ __forceinline__ void rs_src(const RsAxis& a, int o, int& i0, int& i1, float& l1) {
    float s = a.scale * ((float)o + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > a.in - 1) i0 = a.in - 1;
    i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}
// the outputs [lo, hi] that can read input i: src(o) in (i - 1, i + 1), with a one-pixel guard; rs_weight decides membership exactly
__device__ __forceinline__ void rs_range(const RsAxis& a, int i, int& lo, int& hi) {
    const int l = (int)floorf(((float)i - 0.5f) / a.scale - 0.5f) - 1, h = (int)ceilf(((float)i + 1.5f) / a.scale - 0.5f) + 1;
    lo = l > 0 ? l : 0;
    hi = h < a.out - 1 ? h : a.out - 1;
}
// weight of input i in output o (0 outside the footprint; both taps when they coincide at the edge or on a one-pixel source)
__device__ __forceinline__ float rs_weight(const RsAxis& a, int o, int i) {
    int i0, i1;
    float l1;
    rs_src(a, o, i0, i1, l1);
    return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// forward: grid (C / CG, N, row tiles of y), LDS = the source map [Hi Wi][CG] + the reduction scratch; parts (may be NULL): [2][N tiles][C]
__global__ __launch_bounds__(DP_THREADS) void resize_bilinear_fwd_kernel(int C, int CG, RsAxis ah, RsAxis aw, int rows_per_tile, const float* __restrict__ z,
                                                                         long z_ld_pix, long z_ld_img, const float* __restrict__ addend, long a_ld_pix,
                                                                         long a_ld_img, float* __restrict__ y, long y_ld_pix, long y_ld_img,
                                                                         float* __restrict__ parts) {
    SGX_DYN_SMEM(float, smem);
    const int G = CG / 4, P = DP_THREADS / G, cl = threadIdx.x % G, pl = threadIdx.x / G;
    const int img = blockIdx.y, c0 = blockIdx.x * CG + cl * 4;
    float* red = smem;
    float* src = smem + DP_RED_FLOATS;
    const float* zb = z + (long)img * z_ld_img + c0;
    for (int i = pl; i < ah.in * aw.in; i += P) sgx_st4(src + i * CG + cl * 4, sgx_ld4(zb + (long)i * z_ld_pix));
    __syncthreads();
    float4 sy = make_float4(0.f, 0.f, 0.f, 0.f), qy = sy;
    const int r0 = blockIdx.z * rows_per_tile, r1 = r0 + rows_per_tile < ah.out ? r0 + rows_per_tile : ah.out;
    for (int i = r0 * aw.out + pl; i < r1 * aw.out; i += P) {
        const int oh = i / aw.out, ow = i - oh * aw.out;
        int h0, h1, w0, w1;
        float lh, lw;
        rs_src(ah, oh, h0, h1, lh);
        rs_src(aw, ow, w0, w1, lw);
        const float4 v00 = sgx_ld4(src + (h0 * aw.in + w0) * CG + cl * 4), v01 = sgx_ld4(src + (h0 * aw.in + w1) * CG + cl * 4);
        const float4 v10 = sgx_ld4(src + (h1 * aw.in + w0) * CG + cl * 4), v11 = sgx_ld4(src + (h1 * aw.in + w1) * CG + cl * 4);
        const float kh = 1.f - lh, kw = 1.f - lw;
        float4 o = make_float4(kh * (kw * v00.x + lw * v01.x) + lh * (kw * v10.x + lw * v11.x), kh * (kw * v00.y + lw * v01.y) + lh * (kw * v10.y + lw * v11.y),
                               kh * (kw * v00.z + lw * v01.z) + lh * (kw * v10.z + lw * v11.z), kh * (kw * v00.w + lw * v01.w) + lh * (kw * v10.w + lw * v11.w));
        if (addend) dp_acc(o, sgx_ld4(addend + (long)img * a_ld_img + (long)i * a_ld_pix + c0));
        sgx_st4(y + (long)img * y_ld_img + (long)i * y_ld_pix + c0, o);
        dp_acc(sy, o);
        dp_acc_sq(qy, o);
    }
    if (!parts) return;  // (uniform)
    dp_wave_sum(sy, G, 0, red);
    dp_wave_sum(qy, G, 1, red);
    __syncthreads();
    if ((int)threadIdx.x >= 2 * G) return;
    const int q = threadIdx.x / G, c = blockIdx.x * CG + (threadIdx.x % G) * 4;
    const long nblk = (long)gridDim.y * gridDim.z, blk = (long)img * gridDim.z + blockIdx.z;
    sgx_st4(parts + ((long)q * nblk + blk) * C + c, dp_block_sum(red, q, threadIdx.x % G));
}

// backward: grid (C / CG, N), LDS = T [Ho Wi][CG]
__global__ __launch_bounds__(DP_THREADS) void resize_bilinear_bwd_kernel(int C, int CG, RsAxis ah, RsAxis aw, const float* __restrict__ dy, long dy_ld_pix,
                                                                         long dy_ld_img, float* __restrict__ dz, long dz_ld_pix, long dz_ld_img, int accumulate) {
    SGX_DYN_SMEM(float, smem);
    const int G = CG / 4, P = DP_THREADS / G, cl = threadIdx.x % G, pl = threadIdx.x / G;
    const int img = blockIdx.y, c0 = blockIdx.x * CG + cl * 4;
    const float* db = dy + (long)img * dy_ld_img + c0;
    for (int i = pl; i < ah.out * aw.in; i += P) {  // along the rows of dy: the output columns whose two taps include source column wi
        const int oh = i / aw.in, wi = i - oh * aw.in;
        int lo, hi;
        rs_range(aw, wi, lo, hi);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ow = lo; ow <= hi; ++ow) {
            const float k = rs_weight(aw, ow, wi);
            if (k != 0.f) dp_fma(a, k, sgx_ld4(db + ((long)oh * aw.out + ow) * dy_ld_pix));
        }
        sgx_st4(smem + i * CG + cl * 4, a);
    }
    __syncthreads();
    for (int i = pl; i < ah.in * aw.in; i += P) {
        const int hi_ = i / aw.in, wi = i - hi_ * aw.in;
        int lo, hi;
        rs_range(ah, hi_, lo, hi);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int oh = lo; oh <= hi; ++oh) {
            const float k = rs_weight(ah, oh, hi_);
            if (k != 0.f) dp_fma(a, k, sgx_ld4(smem + (oh * aw.in + wi) * CG + cl * 4));
        }
        float* zp = dz + (long)img * dz_ld_img + (long)i * dz_ld_pix + c0;
        if (accumulate) dp_acc(a, sgx_ld4(zp));
        sgx_st4(zp, a);
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
// levels: nlev triples (kernel, stride, padding) on the host
static int32_t dp_levels(int H, int W, int nlev, const int32_t* levels, int glob, DpLevels* lv, const char* what) {
    SGX_CHECK_ARG(nlev >= 0 && nlev <= DP_MAX_LEVELS && (nlev == 0 || levels), "%s: %d window levels (at most %d)", what, nlev, DP_MAX_LEVELS);
    SGX_CHECK_ARG(nlev > 0 || glob, "%s: no level at all", what);
    memset(lv, 0, sizeof(*lv));
    lv->n = nlev;
    lv->glob = glob ? 1 : 0;
    for (int l = 0; l < nlev; ++l) {
        const int k = levels[3 * l], s = levels[3 * l + 1], p = levels[3 * l + 2];
        SGX_CHECK_ARG(s >= 1 && s <= DP_MAX_S && k >= 2 * s && k <= DP_MAX_K && p == s,
                      "%s: level %d (kernel %d, stride %d, padding %d): needs 1 <= stride <= %d, 2 stride <= kernel <= %d, padding == stride", what, l, k, s, p,
                      DP_MAX_S, DP_MAX_K);
        SGX_CHECK_ARG(H + 2 * p >= k && W + 2 * p >= k, "%s: level %d: the padded %d x %d map is smaller than the %d window", what, l, H, W, k);
        lv->k[l] = k; lv->s[l] = s;
        lv->Ho[l] = (H + 2 * p - k) / s + 1;
        lv->Wo[l] = (W + 2 * p - k) / s + 1;
    }
    return SGX_OK;
}
static int32_t dp_dims(int N, int H, int W, int C, const char* what) {
    SGX_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "%s: bad dims N=%d H=%d W=%d C=%d (C a multiple of 4)", what, N, H, W, C);
    SGX_CHECK_ARG(N <= 65535 && (long)H * W < (1L << 24), "%s: N=%d above 65535 or a plane of 2^24 pixels", what, N);
    return SGX_OK;
}

extern "C" int32_t sgx_dappm_pool_fwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t nlev, const int32_t* levels, int32_t has_global, const float* x,
                                      int64_t x_ld_pix, int64_t x_ld_img, float* p0, float* p1, float* p2, float* pg, float* partials, void* stream) {
    int32_t rc = dp_dims(N, H, W, C, "dappm_pool_fwd");
    if (rc) return rc;
    DpLevels lv;
    if ((rc = dp_levels(H, W, nlev, levels, has_global, &lv, "dappm_pool_fwd"))) return rc;
    float* const ps[DP_MAX_LEVELS] = {p0, p1, p2};
    for (int l = 0; l < nlev; ++l) SGX_CHECK_ARG(ps[l] && DP_ALIGNED(ps[l]), "dappm_pool_fwd: pooled map %d is NULL or not 16-byte aligned", l);
    SGX_CHECK_ARG(x && (!has_global || pg), "dappm_pool_fwd: null pointer");
    SGX_CHECK_ARG(DP_LD4(x_ld_pix) && DP_LD4(x_ld_img) && x_ld_pix >= C && DP_ALIGNED(x) && DP_ALIGNED(pg) && DP_ALIGNED(partials),
                  "dappm_pool_fwd: strides and addresses must be multiples of 16 bytes");
    long per_ch = (long)H * W * 4;
    for (int l = 0; l < nlev; ++l) per_ch += (long)H * lv.Wo[l] * 4;
    const int cg = dp_pick_cg(C, N, per_ch, DP_RED_FLOATS * 4);
    if (!cg)
        SGX_FAIL(SGX_ERR_UNSUPPORTED, "dappm_pool_fwd: a %d x %d plane needs %ld bytes of LDS per channel (limit %d for four): row tiling is not built", H, W,
                 per_ch, DP_MAX_LDS);
    const size_t smem = (size_t)per_ch * cg + DP_RED_FLOATS * 4;
    if (smem > 64 * 1024) DP_RAISE_LDS(dappm_pool_fwd_kernel, "dappm_pool_fwd");
    SGX_LAUNCH(dappm_pool_fwd_kernel, dim3((unsigned)(C / cg), (unsigned)N), dim3(DP_THREADS), smem, stream, H, W, C, cg, lv, x, (long)x_ld_pix, (long)x_ld_img,
               p0, p1, p2, pg, partials);
    SGX_CHECK_LAUNCH("dappm_pool_fwd");
    return SGX_OK;
}

extern "C" int32_t sgx_dappm_pool_bwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t nlev, const int32_t* levels, const float* d0, const float* d1,
                                      const float* d2, const float* dg, const float* a1, int64_t a1_ld_pix, int64_t a1_ld_img, const float* a2,
                                      int64_t a2_ld_pix, int64_t a2_ld_img, float* dx, int64_t dx_ld_pix, int64_t dx_ld_img, int32_t accumulate, void* stream) {
    int32_t rc = dp_dims(N, H, W, C, "dappm_pool_bwd");
    if (rc) return rc;
    DpLevels lv;
    if ((rc = dp_levels(H, W, nlev, levels, dg != NULL, &lv, "dappm_pool_bwd"))) return rc;
    const float* const ds[DP_MAX_LEVELS] = {d0, d1, d2};
    for (int l = 0; l < nlev; ++l) SGX_CHECK_ARG(ds[l] && DP_ALIGNED(ds[l]), "dappm_pool_bwd: pooled gradient %d is NULL or not 16-byte aligned", l);
    SGX_CHECK_ARG(dx && DP_LD4(dx_ld_pix) && DP_LD4(dx_ld_img) && dx_ld_pix >= C && DP_ALIGNED(dx) && DP_ALIGNED(dg) &&
                      (!a1 || (DP_LD4(a1_ld_pix) && DP_LD4(a1_ld_img) && a1_ld_pix >= C && DP_ALIGNED(a1))) &&
                      (!a2 || (DP_LD4(a2_ld_pix) && DP_LD4(a2_ld_img) && a2_ld_pix >= C && DP_ALIGNED(a2))),
                  "dappm_pool_bwd: null dx, or strides and addresses that are no multiples of 16 bytes");
    long per_ch = 0;
    for (int l = 0; l < nlev; ++l) per_ch += (long)lv.Ho[l] * lv.Wo[l] * 4;
    const int cg = dp_pick_cg(C, N, per_ch, 16);
    if (!cg) SGX_FAIL(SGX_ERR_UNSUPPORTED, "dappm_pool_bwd: the pooled gradients of a %d x %d plane need %ld bytes of LDS per channel", H, W, per_ch);
    int tiles;
    const int rows = dp_row_tiles(H, C, cg, N, &tiles);
    const size_t smem = (size_t)per_ch * cg + 16;
    if (smem > 64 * 1024) DP_RAISE_LDS(dappm_pool_bwd_kernel, "dappm_pool_bwd");
    SGX_LAUNCH(dappm_pool_bwd_kernel, dim3((unsigned)(C / cg), (unsigned)N, (unsigned)tiles), dim3(DP_THREADS), smem, stream, H, W, C, cg, lv, rows, d0, d1, d2,
               dg, a1, (long)a1_ld_pix, (long)a1_ld_img, a2, (long)a2_ld_pix, (long)a2_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate ? 1 : 0);
    SGX_CHECK_LAUNCH("dappm_pool_bwd");
    return SGX_OK;
}

static int32_t rs_check(int N, int Hi, int Wi, int Ho, int Wo, int C, const char* what) {
    SGX_CHECK_ARG(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0, "%s: bad dims N=%d %d x %d -> %d x %d C=%d (C a multiple of 4)", what, N,
                  Hi, Wi, Ho, Wo, C);
    SGX_CHECK_ARG(N <= 65535 && (long)Hi * Wi < (1L << 24) && (long)Ho * Wo < (1L << 24), "%s: N=%d above 65535 or a map of 2^24 pixels", what, N);
    return SGX_OK;
}
// geometry of a forward launch: channel-group width (0: the source does not fit LDS), rows of y per tile and the tile count
static int rs_fwd_geom(int N, int Hi, int Wi, int Ho, int C, int* rows, int* tiles) {
    const int cg = dp_pick_cg(C, (long)N * Ho, (long)Hi * Wi * 4, DP_RED_FLOATS * 4);
    if (cg) *rows = dp_row_tiles(Ho, C, cg, N, tiles);
    return cg;
}
extern "C" int32_t sgx_resize_bilinear_row_tiles(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t C) {
    int rows = 0, tiles = 0;
    if (N <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || C <= 0 || C % 4 || !rs_fwd_geom(N, Hi, Wi, Ho, C, &rows, &tiles)) return 0;
    return tiles;
}
extern "C" int32_t sgx_resize_bilinear_fwd(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t C, const float* z, int64_t z_ld_pix,
                                           int64_t z_ld_img, const float* addend, int64_t a_ld_pix, int64_t a_ld_img, float* y, int64_t y_ld_pix,
                                           int64_t y_ld_img, float* partials, void* stream) {
    int32_t rc = rs_check(N, Hi, Wi, Ho, Wo, C, "resize_bilinear_fwd");
    if (rc) return rc;
    SGX_CHECK_ARG(z && y && DP_LD4(z_ld_pix) && DP_LD4(z_ld_img) && DP_LD4(y_ld_pix) && DP_LD4(y_ld_img) && z_ld_pix >= C && y_ld_pix >= C && DP_ALIGNED(z) &&
                      DP_ALIGNED(y) && DP_ALIGNED(partials) && (!addend || (DP_LD4(a_ld_pix) && DP_LD4(a_ld_img) && a_ld_pix >= C && DP_ALIGNED(addend))),
                  "resize_bilinear_fwd: null pointer, or strides and addresses that are no multiples of 16 bytes");
    int rows = 0, tiles = 0;
    const int cg = rs_fwd_geom(N, Hi, Wi, Ho, C, &rows, &tiles);
    if (!cg) SGX_FAIL(SGX_ERR_UNSUPPORTED, "resize_bilinear_fwd: a %d x %d source map does not fit LDS", Hi, Wi);
    const size_t smem = (size_t)Hi * Wi * cg * 4 + DP_RED_FLOATS * 4;
    if (smem > 64 * 1024) DP_RAISE_LDS(resize_bilinear_fwd_kernel, "resize_bilinear_fwd");
    SGX_LAUNCH(resize_bilinear_fwd_kernel, dim3((unsigned)(C / cg), (unsigned)N, (unsigned)tiles), dim3(DP_THREADS), smem, stream, C, cg, rs_axis(Hi, Ho),
               rs_axis(Wi, Wo), rows, z, (long)z_ld_pix, (long)z_ld_img, addend, (long)a_ld_pix, (long)a_ld_img, y, (long)y_ld_pix, (long)y_ld_img, partials);
    SGX_CHECK_LAUNCH("resize_bilinear_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_resize_bilinear_bwd(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t C, const float* dy, int64_t dy_ld_pix,
                                           int64_t dy_ld_img, float* dz, int64_t dz_ld_pix, int64_t dz_ld_img, int32_t accumulate, void* stream) {
    int32_t rc = rs_check(N, Hi, Wi, Ho, Wo, C, "resize_bilinear_bwd");
    if (rc) return rc;
    SGX_CHECK_ARG(dy && dz && DP_LD4(dy_ld_pix) && DP_LD4(dy_ld_img) && DP_LD4(dz_ld_pix) && DP_LD4(dz_ld_img) && dy_ld_pix >= C && dz_ld_pix >= C &&
                      DP_ALIGNED(dy) && DP_ALIGNED(dz),
                  "resize_bilinear_bwd: null pointer, or strides and addresses that are no multiples of 16 bytes");
    const int cg = dp_pick_cg(C, N, (long)Ho * Wi * 4, 16);
    if (!cg) SGX_FAIL(SGX_ERR_UNSUPPORTED, "resize_bilinear_bwd: the %d x %d row sums do not fit LDS", Ho, Wi);
    const size_t smem = (size_t)Ho * Wi * cg * 4 + 16;
    if (smem > 64 * 1024) DP_RAISE_LDS(resize_bilinear_bwd_kernel, "resize_bilinear_bwd");
    SGX_LAUNCH(resize_bilinear_bwd_kernel, dim3((unsigned)(C / cg), (unsigned)N), dim3(DP_THREADS), smem, stream, C, cg, rs_axis(Hi, Ho), rs_axis(Wi, Wo), dy,
               (long)dy_ld_pix, (long)dy_ld_img, dz, (long)dz_ld_pix, (long)dz_ld_img, accumulate ? 1 : 0);
    SGX_CHECK_LAUNCH("resize_bilinear_bwd");
    return SGX_OK;
}
