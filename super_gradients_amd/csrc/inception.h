// GoogLeNet's pool-projection branch, MaxPool2d(3, stride 1, pad 1) -> 1x1 convolution, as ONE launch per pass: forward, data gradient, weight
// gradient.  Included by pool.hip behind gconv.h (GC_LD, gc_mfma, the fold kernel of the depthwise weight gradient).  Below them: the ceil-mode
// entry points of the plain max-pool.  Filter storage [Co][1][1][Ci]; Ci % 4 == 0, Co % 4 == 0; every operand may be a channel slice.
//
// P(x) is never stored.  A workgroup (four waves) owns 8 x TW pixels of ONE image (TW = 16, or 8 when the map is no wider than 8).  Per chunk
// of 16 input channels it stages the 10 x (TW + 2) patch in LDS (-inf outside the map), takes the maximum of three columns into a second array
// and the maximum of three rows of that back over the patch: the pooled tile, [pixel][GC_LD], which is the pixel operand of
// v_mfma_f32_16x16x4_f32 as gconv.h's patch is.  The maximum follows ATen: a later value replaces the running one when it is larger or a NaN.
//   forward          the filter chunk [Co tile][16] is the other operand; a lane ends with four consecutive output channels of one pixel.  One
//                    workgroup carries up to 128 output channels (x is read once for GoogLeNet's 32 .. 128); blockIdx.y walks wider filters.
//   weight gradient  dw[co][ci] += sum over pixels dy[p][co] * P(x)[p][ci]: the reduction index is the pixel.  A workgroup owns 16 input channels
//                    and up to 64 output channels, walks per_blk tiles and leaves a partial [Co][Ci] in the workspace; dwconv_wgrad_fold_kernel
//                    adds the partials to dw in a fixed order.
//   data gradient    a GATHER: the workgroup owns a dx tile.  It forms d_pooled = dy * W on the tile plus a one-pixel halo (reduction over Co on
//                    the matrix pipe), recomputes every halo pixel's arg-max from the x patch with a two-pixel halo (one byte per channel: the
//                    window position, ATen's first-maximum rule) and each dx pixel adds the up to nine d_pooled values whose window selected
//                    it, rows then columns ascending - the order of ATen's CPU backward.  The dy halo tile stays in LDS across the Ci chunks
//                    while the launch's LDS is within IC_DG_MAX_LDS (Co <= 156 on 8 x 16 tiles, Co <= 244 on 8 x 8); wider filters re-read dy
//                    per chunk in blocks of 64 channels.
// No atomics anywhere: every sum has a fixed order.
#pragma once

#define IC_TH 8
#define IC_NBMAX 8                    // 16-channel blocks of the forward's channel tile
#define IC_WG_KB 4                    // 16-channel blocks of dy per weight-gradient workgroup
#define IC_DG_MAX_LDS (152 * 1024)    // as MP_SCATTER_MAX_LDS
#define IC_DG_STREAM_KB 64            // dy channels per block of the data gradient's re-read route
struct IcGeom {
    int N, H, W, Ci, Co;
    int TW, twsh, tilesA, tilesB;
};
static IcGeom ic_geom(int N, int H, int W, int Ci, int Co) {
    IcGeom g;
    g.N = N; g.H = H; g.W = W; g.Ci = Ci; g.Co = Co;
    g.twsh = W > 8 ? 4 : 3;
    g.TW = 1 << g.twsh;
    g.tilesA = sgx_cdiv(H, IC_TH);
    g.tilesB = sgx_cdiv(W, g.TW);
    return g;
}

__device__ __forceinline__ float ic_max(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float4 ic_max4(float4 m, float4 v) { return make_float4(ic_max(m.x, v.x), ic_max(m.y, v.y), ic_max(m.z, v.z), ic_max(m.w, v.w)); }

// The pooled tile of the channels [c0, c0 + 16) at (a0, b0): patch [10 * (TW + 2)][GC_LD] in, the pooled [8 * TW][GC_LD] over its start out;
// rmax [10 * TW][GC_LD].  Channels beyond Ci and pixels beyond the map pool to 0.  The caller synchronises before reading the tile.
__device__ __forceinline__ void ic_stage_pooled(const IcGeom& g, float* patch, float* rmax, const float* __restrict__ xb, long ld_pix, int a0, int b0,
                                                int c0, int tid) {
    const int PW = g.TW + 2;
    const float ninf = -INFINITY;
    for (int i = tid; i < (IC_TH + 2) * PW * 4; i += GC_THREADS) {
        const int pix = i >> 2, q = (i & 3) * 4;
        const int hi = a0 - 1 + pix / PW, wi = b0 - 1 + pix % PW;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 + q < g.Ci) {
            const bool in = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
            v = in ? sgx_ld4(xb + ((long)hi * g.W + wi) * ld_pix + c0 + q) : make_float4(ninf, ninf, ninf, ninf);
        }
        sgx_st4(patch + pix * GC_LD + q, v);
    }
    __syncthreads();
    for (int i = tid; i < (IC_TH + 2) * g.TW * 4; i += GC_THREADS) {
        const int t = i >> 2, q = (i & 3) * 4;
        const float* p = patch + ((t >> g.twsh) * PW + (t & (g.TW - 1))) * GC_LD + q;
        sgx_st4(rmax + t * GC_LD + q, ic_max4(ic_max4(sgx_ld4(p), sgx_ld4(p + GC_LD)), sgx_ld4(p + 2 * GC_LD)));
    }
    __syncthreads();
    for (int i = tid; i < IC_TH * g.TW * 4; i += GC_THREADS) {
        const int p = i >> 2, q = (i & 3) * 4;
        const float* r = rmax + p * GC_LD + q;
        const bool in = a0 + (p >> g.twsh) < g.H && b0 + (p & (g.TW - 1)) < g.W;
        const float4 m = ic_max4(ic_max4(sgx_ld4(r), sgx_ld4(r + g.TW * GC_LD)), sgx_ld4(r + 2 * g.TW * GC_LD));
        sgx_st4(patch + p * GC_LD + q, in ? m : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}
__device__ __forceinline__ void ic_tile(const IcGeom& g, int t, int& img, int& a0, int& b0) {
    b0 = (t % g.tilesB) * g.TW;
    t /= g.tilesB;
    a0 = (t % g.tilesA) * IC_TH;
    img = t / g.tilesA;
}

// y = act(W * P(x) + bias); partials: [2][gridDim.x][Co] sum / sum of squares.  MT = TW / 8 position groups per wave, NB channel blocks.
template <int MT, int NB>
__global__ __launch_bounds__(GC_THREADS) void ic_fwd_kernel(IcGeom g, const float* __restrict__ x, long x_ld_pix, long x_ld_img,
                                                            const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
                                                            long y_ld_pix, long y_ld_img, int act, float* __restrict__ partials) {
    SGX_DYN_SMEM(float, smem);
    __shared__ float4 red[4][4];
    float* patch = smem;                                     // [10 * (TW + 2)][GC_LD]; the pooled tile after staging
    float* rmax = patch + (IC_TH + 2) * (g.TW + 2) * GC_LD;  // [10 * TW][GC_LD]
    float* fl = rmax + (IC_TH + 2) * g.TW * GC_LD;           // [NB * 16][GC_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    int img, a0, b0;
    ic_tile(g, blockIdx.x, img, a0, b0);
    const int cbase = blockIdx.y * (NB * 16);
    sgx_f32x4 acc[MT][NB];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mt][nb] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ xb = x + (long)img * x_ld_img;
    for (int rb = 0; rb < g.Ci; rb += 16) {
        __syncthreads();
        for (int i = tid; i < NB * 64; i += GC_THREADS) {
            const int q = (i & 3) * 4, o = i >> 2, co = cbase + o;
            const bool in = co < g.Co && rb + q < g.Ci;
            sgx_st4(fl + o * GC_LD + q, in ? sgx_ld4(w + (long)co * g.Ci + rb + q) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        ic_stage_pooled(g, patch, rmax, xb, x_ld_pix, a0, b0, rb, tid);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float bv[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) bv[mt] = patch[((wave * MT + mt) * 16 + li) * GC_LD + lj + 4 * ks];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (cbase + nb * 16 >= g.Co) continue;
                const float av = fl[(nb * 16 + li) * GC_LD + lj + 4 * ks];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nb] = gc_mfma(av, bv[mt], acc[mt][nb]);
            }
        }
    }
    // a lane holds channels cbase + nb * 16 + 4 lj .. + 3 of position li of its groups
    float4 q0[NB], q1[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) q0[nb] = q1[nb] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = (wave * MT + mt) * 16 + li;
        const int a = a0 + (p >> g.twsh), b = b0 + (p & (g.TW - 1));
        const bool pix_ok = a < g.H && b < g.W;
        float* yp = y + (long)img * y_ld_img + ((long)a * g.W + b) * y_ld_pix;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = cbase + nb * 16 + 4 * lj;
            if (!(pix_ok && c < g.Co)) continue;
            float4 v = make_float4(acc[mt][nb][0], acc[mt][nb][1], acc[mt][nb][2], acc[mt][nb][3]);
            if (partials) {
                q0[nb].x += v.x; q0[nb].y += v.y; q0[nb].z += v.z; q0[nb].w += v.w;
                q1[nb].x += v.x * v.x; q1[nb].y += v.y * v.y; q1[nb].z += v.z * v.z; q1[nb].w += v.w * v.w;
            }
            if (bias) {
                const float4 bb = sgx_ld4(bias + c);
                v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
            }
            sgx_st4(yp + c, make_float4(sgx_act(v.x, act), sgx_act(v.y, act), sgx_act(v.z, act), sgx_act(v.w, act)));
        }
    }
    if (partials) {  // the 16 position lanes in a fixed butterfly, then the four waves in order (as gconv_kernel)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float4 q = h ? q1[nb] : q0[nb];
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    q.x += __shfl_xor(q.x, m); q.y += __shfl_xor(q.y, m); q.z += __shfl_xor(q.z, m); q.w += __shfl_xor(q.w, m);
                }
                __syncthreads();
                if (li == 0) red[wave][lj] = q;
                __syncthreads();
                const int c = cbase + nb * 16 + 4 * tid;
                if (tid < 4 && c < g.Co) {
                    float4 s = red[0][tid];
#pragma unroll
                    for (int k = 1; k < 4; ++k) { s.x += red[k][tid].x; s.y += red[k][tid].y; s.z += red[k][tid].z; s.w += red[k][tid].w; }
                    sgx_st4(partials + ((long)h * gridDim.x + blockIdx.x) * g.Co + c, s);
                }
            }
    }
}

// Weight gradient, stage 1.  blockIdx.y = (block of 16 input channels, block of 64 output channels); the workgroup walks the tiles
// [blockIdx.x * per_blk, ...).  The dy tile [IC_WG_KB][MT * 64][GC_LD] lies over rmax, which is dead once the pooled tile stands.  The four waves
// take every fourth step of four pixels and meet in LDS in wave order.
template <int MT>
__global__ __launch_bounds__(GC_THREADS) void ic_wgrad_kernel(IcGeom g, int per_blk, int ntiles, const float* __restrict__ x, long x_ld_pix,
                                                              long x_ld_img, const float* __restrict__ dy, long dy_ld_pix, long dy_ld_img,
                                                              float* __restrict__ ws) {
    SGX_DYN_SMEM(float, smem);
    float* patch = smem;
    float* rmax = patch + (IC_TH + 2) * (g.TW + 2) * GC_LD;
    float* dyt = rmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    const int kpasses = (g.Co + IC_WG_KB * 16 - 1) / (IC_WG_KB * 16);
    const int cib = blockIdx.y / kpasses, k0 = (blockIdx.y % kpasses) * (IC_WG_KB * 16);
    sgx_f32x4 acc[IC_WG_KB];
#pragma unroll
    for (int kb = 0; kb < IC_WG_KB; ++kb) acc[kb] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    const int t_end = min(ntiles, (int)(blockIdx.x + 1) * per_blk);
    for (int tile = blockIdx.x * per_blk; tile < t_end; ++tile) {
        int img, a0, b0;
        ic_tile(g, tile, img, a0, b0);
        __syncthreads();
        ic_stage_pooled(g, patch, rmax, x + (long)img * x_ld_img, x_ld_pix, a0, b0, cib * 16, tid);
        __syncthreads();
        for (int i = tid; i < MT * 64 * IC_WG_KB * 4; i += GC_THREADS) {
            const int p = i >> 4, f = i & 15, kb = f >> 2, q = (f & 3) * 4;
            const int a = a0 + (p >> g.twsh), b = b0 + (p & (g.TW - 1)), co = k0 + kb * 16 + q;
            const bool in = a < g.H && b < g.W && co < g.Co;
            sgx_st4(dyt + (kb * MT * 64 + p) * GC_LD + q, in ? sgx_ld4(dy + (long)img * dy_ld_img + ((long)a * g.W + b) * dy_ld_pix + co) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        __syncthreads();
        for (int ks = wave; ks < MT * 16; ks += 4) {
            const int p = 4 * ks + lj;
            const float bv = patch[p * GC_LD + li];
#pragma unroll
            for (int kb = 0; kb < IC_WG_KB; ++kb) {
                if (k0 + kb * 16 >= g.Co) continue;
                acc[kb] = gc_mfma(dyt[(kb * MT * 64 + p) * GC_LD + li], bv, acc[kb]);
            }
        }
    }
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(smem);  // [4 waves][IC_WG_KB][64]
#pragma unroll
    for (int kb = 0; kb < IC_WG_KB; ++kb) red[(wave * IC_WG_KB + kb) * 64 + lane] = make_float4(acc[kb][0], acc[kb][1], acc[kb][2], acc[kb][3]);
    __syncthreads();
    float* out = ws + (long)blockIdx.x * g.Co * g.Ci;
    {
        const int kb = tid >> 6, l = tid & 63;  // IC_WG_KB * 64 == GC_THREADS
        float4 s = red[kb * 64 + l];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float4 u = red[(k * IC_WG_KB + kb) * 64 + l];
            s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        const float sv[4] = {s.x, s.y, s.z, s.w};
        const int ci = cib * 16 + (l & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = k0 + kb * 16 + 4 * (l >> 4) + r;
            if (co < g.Co && ci < g.Ci) out[(long)co * g.Ci + ci] = sv[r];
        }
    }
}

// Data gradient.  MTD 16-pixel groups of the halo tile per wave: 3 (8 x 16 tile: 10 x 18 = 180 of 192 pixels) or 2 (8 x 8: 100 of 128).
// LDS: dyb [MTD * 64][pitch] the dy halo tile (KB channels of it on the re-read route), wl [16][pitch] the filter chunk transposed, xp
// [12 * (TW + 4)][GC_LD] the x patch - d_pooled [MTD * 64][GC_LD] is written over it once the arg-max bytes stand -, amx [MTD * 64][4] words of
// four arg-max bytes.  pitch / 4 is odd: the 16 pixel rows x 4 reduction indices of an operand read fall into 64 different banks.
template <int MTD>
__global__ __launch_bounds__(GC_THREADS) void ic_dgrad_kernel(IcGeom g, int KB, int pitch, int resident, const float* __restrict__ dy, long dy_ld_pix,
                                                              long dy_ld_img, const float* __restrict__ w, const float* __restrict__ x, long x_ld_pix,
                                                              long x_ld_img, float* __restrict__ dx, long dx_ld_pix, long dx_ld_img, int accumulate) {
    constexpr int NPIX = MTD * 64;
    SGX_DYN_SMEM(float, smem);
    const int HW2 = g.TW + 2, XW = g.TW + 4, nhalo = (IC_TH + 2) * HW2;
    float* dyb = smem;
    float* wl = dyb + (long)NPIX * pitch;
    float* xp = wl + 16 * pitch;
    float* dpool = xp;
    unsigned* amx = reinterpret_cast<unsigned*>(xp + (IC_TH + 4) * XW * GC_LD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    int img, a0, b0;
    ic_tile(g, blockIdx.x, img, a0, b0);
    const float* __restrict__ xb = x + (long)img * x_ld_img;
    const float* __restrict__ dyi = dy + (long)img * dy_ld_img;
    for (int rb = 0; rb < g.Ci; rb += 16) {
        __syncthreads();
        for (int i = tid; i < (IC_TH + 4) * XW * 4; i += GC_THREADS) {
            const int pix = i >> 2, q = (i & 3) * 4;
            const int hi = a0 - 2 + pix / XW, wi = b0 - 2 + pix % XW;
            const bool in = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W && rb + q < g.Ci;
            sgx_st4(xp + pix * GC_LD + q, in ? sgx_ld4(xb + ((long)hi * g.W + wi) * x_ld_pix + rb + q) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        __syncthreads();
        // the window position (0 .. 8, row-major) every halo pixel's window selects, per channel; 0xff for a halo pixel outside the map
        for (int i = tid; i < nhalo * 4; i += GC_THREADS) {
            const int pix = i >> 2, qg = i & 3, pr = pix / HW2, pc = pix % HW2;
            const int hi = a0 - 1 + pr, wi = b0 - 1 + pc;
            unsigned word = 0xffffffffu;
            if (hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) {
                float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int code[4] = {-1, -1, -1, -1};
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int hh = hi - 1 + t / 3, ww = wi - 1 + t % 3;
                    if (hh < 0 || hh >= g.H || ww < 0 || ww >= g.W) continue;
                    const float4 v4 = sgx_ld4(xp + ((pr + t / 3) * XW + pc + t % 3) * GC_LD + qg * 4);
                    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                    for (int z = 0; z < 4; ++z)
                        if (v[z] > m[z] || v[z] != v[z] || code[z] < 0) { m[z] = v[z]; code[z] = t; }
                }
                word = (unsigned)code[0] | ((unsigned)code[1] << 8) | ((unsigned)code[2] << 16) | ((unsigned)code[3] << 24);
            }
            amx[pix * 4 + qg] = word;
        }
        __syncthreads();
        sgx_f32x4 acc[MTD];
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt) acc[mt] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < g.Co; k0 += KB) {
            const int kn = min(KB, g.Co - k0);
            if (k0) __syncthreads();
            for (int i = tid; i < kn * 4; i += GC_THREADS) {
                const int co = i >> 2, q = (i & 3) * 4;
                const float4 v = rb + q < g.Ci ? sgx_ld4(w + (long)(k0 + co) * g.Ci + rb + q) : make_float4(0.f, 0.f, 0.f, 0.f);
                float* d = wl + q * pitch + co;
                d[0] = v.x; d[pitch] = v.y; d[2 * pitch] = v.z; d[3 * pitch] = v.w;
            }
            if (!resident || rb == 0) {
                const int k4 = kn >> 2;
                for (int i = tid; i < NPIX * k4; i += GC_THREADS) {
                    const int pix = i / k4, f = i - pix * k4;
                    const int hi = a0 - 1 + pix / HW2, wi = b0 - 1 + pix % HW2;
                    const bool in = pix < nhalo && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                    sgx_st4(dyb + (long)pix * pitch + 4 * f, in ? sgx_ld4(dyi + ((long)hi * g.W + wi) * dy_ld_pix + k0 + 4 * f) : make_float4(0.f, 0.f, 0.f, 0.f));
                }
            }
            __syncthreads();
            for (int ks = 0; ks < (kn >> 2); ++ks) {
                const float av = wl[li * pitch + 4 * ks + lj];
#pragma unroll
                for (int mt = 0; mt < MTD; ++mt) acc[mt] = gc_mfma(av, dyb[(long)((wave * MTD + mt) * 16 + li) * pitch + 4 * ks + lj], acc[mt]);
            }
        }
        // a lane holds input channels rb + 4 lj .. + 3 of halo pixel li of its groups
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt)
            sgx_st4(dpool + ((wave * MTD + mt) * 16 + li) * GC_LD + 4 * lj, make_float4(acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]));
        __syncthreads();
        for (int i = tid; i < IC_TH * g.TW * 4; i += GC_THREADS) {
            const int p = i >> 2, qg = i & 3, a = p >> g.twsh, b = p & (g.TW - 1);
            const int hi = a0 + a, wi = b0 + b;
            if (hi >= g.H || wi >= g.W || rb + 4 * qg >= g.Ci) continue;
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {  // the window of halo pixel (a + t / 3, b + t % 3) holds this pixel at position 8 - t
                const int hp = (a + t / 3) * HW2 + b + t % 3;
                const unsigned word = amx[hp * 4 + qg];
                const float4 d4 = sgx_ld4(dpool + hp * GC_LD + 4 * qg);
                const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int z = 0; z < 4; ++z)
                    if (((word >> (8 * z)) & 0xffu) == (unsigned)(8 - t)) s[z] += d[z];
            }
            float* o = dx + (long)img * dx_ld_img + ((long)hi * g.W + wi) * dx_ld_pix + rb + 4 * qg;
            if (accumulate) {
                const float4 u = sgx_ld4(o);
                s[0] += u.x; s[1] += u.y; s[2] += u.z; s[3] += u.w;
            }
            sgx_st4(o, make_float4(s[0], s[1], s[2], s[3]));
        }
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------------
static int32_t ic_check(int N, int H, int W, int Ci, int Co, long a_pix, long a_img, int a_c, long b_pix, long b_img, int b_c, const char* what) {
    SGX_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0, "%s: bad dims N=%d H=%d W=%d Ci=%d Co=%d", what, N, H, W, Ci, Co);
    SGX_CHECK_ARG(Ci % 4 == 0 && Co % 4 == 0, "%s: Ci=%d and Co=%d must be multiples of 4 (16-byte channel groups)", what, Ci, Co);
    SGX_CHECK_ARG(a_pix >= a_c && b_pix >= b_c && a_pix % 4 == 0 && b_pix % 4 == 0 && a_img % 4 == 0 && b_img % 4 == 0,
                  "%s: pixel / image strides must be multiples of 4 floats and at least the channel count", what);
    SGX_CHECK_ARG((long)N * H * W < 0x7fffffffL && (long)Ci * Co < 0x7fffffffL, "%s: more than 2^31 pixels or filter elements", what);
    return SGX_OK;
}
static long ic_fwd_lds(const IcGeom& g, int nb) { return ((long)(IC_TH + 2) * (2 * g.TW + 2) + nb * 16) * GC_LD * 4; }

extern "C" int32_t sgx_pool3_conv1x1_stat_blocks(int32_t N, int32_t H, int32_t W) {
    if (N <= 0 || H <= 0 || W <= 0 || (long)N * H * W >= 0x7fffffffL) return 0;
    const IcGeom g = ic_geom(N, H, W, 4, 4);
    return N * g.tilesA * g.tilesB;
}
extern "C" int32_t sgx_pool3_conv1x1_fwd(int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co, const float* x, int64_t x_ld_pix, int64_t x_ld_img,
                                         const float* w, const float* bias, float* y, int64_t y_ld_pix, int64_t y_ld_img, int32_t act,
                                         float* stat_partials, void* stream) {
    int32_t rc = ic_check(N, H, W, Ci, Co, x_ld_pix, x_ld_img, Ci, y_ld_pix, y_ld_img, Co, "pool3_conv1x1_fwd");
    if (rc) return rc;
    SGX_CHECK_ARG(x && w && y, "pool3_conv1x1_fwd: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(w) && DW_ALIGNED(y) && DW_ALIGNED(bias) && DW_ALIGNED(stat_partials), "pool3_conv1x1_fwd: operands must be 16-byte aligned");
    SGX_CHECK_ACT3(act, "pool3_conv1x1_fwd");
    SGX_CHECK_ARG(!stat_partials || (!bias && act == SGX_ACT_NONE), "pool3_conv1x1_fwd: statistics rows go with the plain convolution (no bias, no activation)");
    const IcGeom g = ic_geom(N, H, W, Ci, Co);
    const int nb = Co <= 32 ? 2 : IC_NBMAX;
    const dim3 grid((unsigned)(N * g.tilesA * g.tilesB), (unsigned)sgx_cdiv(Co, nb * 16));
    const unsigned lds = (unsigned)ic_fwd_lds(g, nb);
#define IC_GO(MT_, NB_) SGX_LAUNCH((ic_fwd_kernel<MT_, NB_>), grid, dim3(GC_THREADS), lds, stream, g, x, (long)x_ld_pix, (long)x_ld_img, w, bias, y, (long)y_ld_pix, (long)y_ld_img, act, stat_partials)
    if (g.TW == 16) {
        if (nb == 2) IC_GO(2, 2);
        else IC_GO(2, IC_NBMAX);
    } else {
        if (nb == 2) IC_GO(1, 2);
        else IC_GO(1, IC_NBMAX);
    }
#undef IC_GO
    SGX_CHECK_LAUNCH("pool3_conv1x1_fwd");
    return SGX_OK;
}

// pitch of a [..][kb] operand tile of the data gradient: at least kb floats, pitch / 4 odd
static int ic_dg_pitch(int kb) { return (kb / 4) % 2 ? kb : kb + 4; }
static long ic_dg_lds(const IcGeom& g, int kb) {
    const int npix = g.TW == 16 ? 192 : 128;
    return ((long)(npix + 16) * ic_dg_pitch(kb) + (long)(IC_TH + 4) * (g.TW + 4) * GC_LD + npix * 4) * 4;
}
template <int MTD>
static int32_t ic_dg_raise_lds() {
#ifndef SGX_EMU
    // dynamic LDS beyond 64 KB is opt-in per function AND per device: one flag bit per device ordinal (as maxpool_bwd_scatter_kernel)
    static std::atomic<unsigned long long> raised{0ull};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute((const void*)ic_dgrad_kernel<MTD>, hipFuncAttributeMaxDynamicSharedMemorySize, IC_DG_MAX_LDS) != hipSuccess)
            SGX_FAIL(SGX_ERR_HIP, "pool3_conv1x1_bwd_data: cannot raise the kernel's dynamic LDS limit");
        raised.fetch_or(bit, std::memory_order_release);
    }
#endif
    return SGX_OK;
}
extern "C" int32_t sgx_pool3_conv1x1_bwd_data(int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co, const float* dy, int64_t dy_ld_pix,
                                              int64_t dy_ld_img, const float* w, const float* x, int64_t x_ld_pix, int64_t x_ld_img, float* dx,
                                              int64_t dx_ld_pix, int64_t dx_ld_img, int32_t accumulate, void* stream) {
    int32_t rc = ic_check(N, H, W, Ci, Co, x_ld_pix, x_ld_img, Ci, dy_ld_pix, dy_ld_img, Co, "pool3_conv1x1_bwd_data");
    if (rc) return rc;
    SGX_CHECK_ARG(dx_ld_pix >= Ci && dx_ld_pix % 4 == 0 && dx_ld_img % 4 == 0, "pool3_conv1x1_bwd_data: dx strides must be multiples of 4 floats and at least Ci");
    SGX_CHECK_ARG(dy && w && x && dx, "pool3_conv1x1_bwd_data: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(dy) && DW_ALIGNED(w) && DW_ALIGNED(x) && DW_ALIGNED(dx), "pool3_conv1x1_bwd_data: operands must be 16-byte aligned");
    const IcGeom g = ic_geom(N, H, W, Ci, Co);
    const int resident = ic_dg_lds(g, Co) <= IC_DG_MAX_LDS;
    const int kb = resident ? Co : IC_DG_STREAM_KB, pitch = ic_dg_pitch(kb);
    const unsigned lds = (unsigned)ic_dg_lds(g, kb);
    const dim3 grid((unsigned)(N * g.tilesA * g.tilesB));
    if (g.TW == 16) {
        if ((rc = ic_dg_raise_lds<3>())) return rc;
        SGX_LAUNCH(ic_dgrad_kernel<3>, grid, dim3(GC_THREADS), lds, stream, g, kb, pitch, resident, dy, (long)dy_ld_pix, (long)dy_ld_img, w, x, (long)x_ld_pix,
                   (long)x_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate ? 1 : 0);
    } else {
        if ((rc = ic_dg_raise_lds<2>())) return rc;
        SGX_LAUNCH(ic_dgrad_kernel<2>, grid, dim3(GC_THREADS), lds, stream, g, kb, pitch, resident, dy, (long)dy_ld_pix, (long)dy_ld_img, w, x, (long)x_ld_pix,
                   (long)x_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate ? 1 : 0);
    }
    SGX_CHECK_LAUNCH("pool3_conv1x1_bwd_data");
    return SGX_OK;
}

// weight gradient: ~1024 workgroups unless the problem has fewer tiles (every workgroup leaves a 16 x 64 partial)
static IcGeom ic_wgrad_geom(int N, int H, int W, int Ci, int Co, int* npairs, int* nsplit, int* per_blk, int* ntiles) {
    const IcGeom g = ic_geom(N, H, W, Ci, Co);
    *npairs = sgx_cdiv(Ci, 16) * sgx_cdiv(Co, IC_WG_KB * 16);
    *ntiles = N * g.tilesA * g.tilesB;
    long n = *ntiles;
    const long cap = SGX_STRIDE_GRID(sgx_cdiv(GC_WGRAD_BLOCKS, *npairs));  // (two splits on the host emulation, as gc_wgrad_geom)
    if (n > cap) n = cap;
    *per_blk = (int)((*ntiles + n - 1) / n);
    *nsplit = sgx_cdiv(*ntiles, *per_blk);
    return g;
}
extern "C" int64_t sgx_pool3_conv1x1_bwd_weight_workspace(int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co) {
    if (ic_check(N, H, W, Ci, Co, Ci, 0, Ci, Co, 0, Co, "pool3_conv1x1_bwd_weight_workspace")) return 0;
    int npairs, nsplit, per_blk, ntiles;
    ic_wgrad_geom(N, H, W, Ci, Co, &npairs, &nsplit, &per_blk, &ntiles);
    return (int64_t)nsplit * Ci * Co * (int64_t)sizeof(float);
}
extern "C" int32_t sgx_pool3_conv1x1_bwd_weight(int32_t N, int32_t H, int32_t W, int32_t Ci, int32_t Co, const float* x, int64_t x_ld_pix,
                                                int64_t x_ld_img, const float* dy, int64_t dy_ld_pix, int64_t dy_ld_img, float* dw, void* ws,
                                                int64_t ws_bytes, void* stream) {
    int32_t rc = ic_check(N, H, W, Ci, Co, x_ld_pix, x_ld_img, Ci, dy_ld_pix, dy_ld_img, Co, "pool3_conv1x1_bwd_weight");
    if (rc) return rc;
    SGX_CHECK_ARG(x && dy && dw, "pool3_conv1x1_bwd_weight: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(dy) && DW_ALIGNED(dw), "pool3_conv1x1_bwd_weight: operands must be 16-byte aligned");
    int npairs, nsplit, per_blk, ntiles;
    const IcGeom g = ic_wgrad_geom(N, H, W, Ci, Co, &npairs, &nsplit, &per_blk, &ntiles);
    const long ncol = (long)Ci * Co;
    if (!ws || ws_bytes < (int64_t)nsplit * ncol * (int64_t)sizeof(float) || ((uintptr_t)ws % 16) != 0)
        SGX_FAIL(SGX_ERR_WORKSPACE, "pool3_conv1x1_bwd_weight: workspace too small or unaligned (sgx_pool3_conv1x1_bwd_weight_workspace)");
    const int mt = g.TW / 8;
    const long lds = ((long)(IC_TH + 2) * (g.TW + 2) + (long)mt * 64 * IC_WG_KB) * GC_LD * 4;  // (the dy tile is larger than rmax and than the waves' meeting buffer)
    const dim3 grid((unsigned)nsplit, (unsigned)npairs);
    if (mt == 1) SGX_LAUNCH(ic_wgrad_kernel<1>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, per_blk, ntiles, x, (long)x_ld_pix, (long)x_ld_img, dy, (long)dy_ld_pix, (long)dy_ld_img, (float*)ws);
    else SGX_LAUNCH(ic_wgrad_kernel<2>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, per_blk, ntiles, x, (long)x_ld_pix, (long)x_ld_img, dy, (long)dy_ld_pix, (long)dy_ld_img, (float*)ws);
    SGX_CHECK_LAUNCH("pool3_conv1x1_bwd_weight");
    SGX_LAUNCH(dwconv_wgrad_fold_kernel, dim3((unsigned)sgx_cdiv(ncol, 16)), dim3(DW_THREADS), 0, stream, (const float*)ws, nsplit, (int)ncol, dw);
    SGX_CHECK_LAUNCH("pool3_conv1x1_bwd_weight (fold)");
    return SGX_OK;
}

// ---- ceil-mode max pooling: nn.MaxPool2d(ceil_mode=True) extents on the direct kernels, which take Ho / Wo and clip their windows at every
// edge.  The last window must start inside the map or its left / top padding.
// A padded map smaller than the window still has its one clipped window where ATen gives it one (in = 2, k = 3, stride 2); 0: empty.
static int maxpool_out_ceil(int in, int k, int stride, int pad) {
    const int num = in + 2 * pad - k + stride - 1;  // floor(num / stride), as ATen's div_rtn
    int o = (num >= 0 ? num / stride : -((-num + stride - 1) / stride)) + 1;
    if (o > 0 && (o - 1) * stride >= in + pad) --o;
    return o > 0 ? o : 0;
}
extern "C" int32_t sgx_maxpool_ceil_fwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, const float* x,
                                        int64_t x_ld_pix, int64_t x_ld_img, float* y, int64_t y_ld_pix, int64_t y_ld_img, int32_t* argmax,
                                        void* stream) {
    SGX_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && k > 0 && stride > 0, "maxpool_ceil_fwd: bad args");
    SGX_CHECK_ARG(pad >= 0 && 2 * pad <= k, "maxpool_ceil_fwd: pad %d must be at most half the window %d (F.max_pool2d's own rule)", pad, k);
    SGX_CHECK_ARG(x_ld_pix % 4 == 0 && x_ld_img % 4 == 0 && y_ld_pix % 4 == 0 && y_ld_img % 4 == 0 && SGX_ALIGNED16(x) && SGX_ALIGNED16(y),
                  "maxpool_ceil_fwd: strides and addresses must be multiples of 16 bytes");
    const int Ho = maxpool_out_ceil(H, k, stride, pad), Wo = maxpool_out_ceil(W, k, stride, pad);
    SGX_CHECK_ARG(Ho > 0 && Wo > 0, "maxpool_ceil_fwd: empty output");
    long n = (long)N * Ho * Wo * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(maxpool_fwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, H, W, C, k, stride, pad, Ho, Wo,
               x, (long)x_ld_pix, (long)x_ld_img, y, (long)y_ld_pix, (long)y_ld_img, argmax);
    SGX_CHECK_LAUNCH("maxpool_ceil_fwd");
    return SGX_OK;
}
extern "C" int32_t sgx_maxpool_ceil_bwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, const int32_t* argmax,
                                        const float* dy, int64_t dy_ld_pix, int64_t dy_ld_img, float* dx, int64_t dx_ld_pix, int64_t dx_ld_img,
                                        int32_t accumulate, void* stream) {
    SGX_CHECK_ARG(argmax && dy && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && k > 0 && stride > 0, "maxpool_ceil_bwd: bad args");
    SGX_CHECK_ARG(pad >= 0 && 2 * pad <= k, "maxpool_ceil_bwd: pad %d must be at most half the window %d", pad, k);
    SGX_CHECK_ARG(dy_ld_pix % 4 == 0 && dy_ld_img % 4 == 0 && dx_ld_pix % 4 == 0 && dx_ld_img % 4 == 0 && SGX_ALIGNED16(dy) && SGX_ALIGNED16(dx),
                  "maxpool_ceil_bwd: strides and addresses must be multiples of 16 bytes");
    const int Ho = maxpool_out_ceil(H, k, stride, pad), Wo = maxpool_out_ceil(W, k, stride, pad);
    SGX_CHECK_ARG(Ho > 0 && Wo > 0, "maxpool_ceil_bwd: empty output");
    long n = (long)N * H * W * (C / 4), blocks = (n + 255) / 256;
    SGX_LAUNCH(maxpool_bwd_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, N, H, W, C, k, stride, pad, Ho, Wo,
               argmax, dy, (long)dy_ld_pix, (long)dy_ld_img, dx, (long)dx_ld_pix, (long)dx_ld_img, accumulate ? 1 : 0);
    SGX_CHECK_LAUNCH("maxpool_ceil_bwd");
    return SGX_OK;
}
