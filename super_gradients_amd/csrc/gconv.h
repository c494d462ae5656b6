// Grouped 3x3 convolution, pad 1, stride 1 or 2, 1 < groups < C (RegNet's XBlock, ResNeXt's conv2): forward, data gradient, weight gradient.
// Included by pool.hip after the depthwise kernels (the weight gradient shares their fold kernel).  Filter storage [K][3][3][cg].
//
// One tiling for every cg in {4, 8, 16, 32, 64}: v_mfma_f32_16x16x4_f32 tiles of 16 output channels x 16 pixels, the filter as the A operand
// and the pixels as B, so a lane ends up with FOUR consecutive channels of one pixel (16-byte stores, float4 bias / statistics).
//   cg >= 16: the 16 output channels of a tile lie in one group; a workgroup owns the cg / 16 tiles of one group and reduces over that
//             group's 9 * cg inputs in chunks of 16 channels.
//   cg <  16: a tile spans 16 / cg groups; the staged filter block is block-diagonal (zeros where input and output channel are in
//             different groups), the reduction is the tile's own 16 channels.  A last tile that is only partly inside C is masked.
// A workgroup (four waves) owns TH x TW positions (MT * 64) of ONE image; the input patch of 16 channels is staged once per chunk in LDS
// (zeros outside the map), the filter three taps at a time; both with a row pitch of 20 floats: the 64 lanes of an operand read (16 rows x
// 4 reduction indices) then fall into 64 different banks.
// The launch is described by a list of taps (patch offset, filter tap), an input step IS and an output step OS - which makes the data
// gradient the same kernel: stride 1 is the reversed taps with the filter read transposed; stride 2 is four launches, one per parity class
// (dx rows 2a + ph, columns 2b + pw), each a gather over the one, two or four taps whose output position exists.  No scatter, no atomics.
#pragma once

#define GC_THREADS 256
#define GC_LD 20  // floats per staged 16-channel row
struct GcGeom {
    int N, Hi, Wi;            // the map the window walks
    int A, B;                 // rows / columns of the positions this launch computes
    int OS, oh0, ow0, Wout;   // position (a, b) is pixel (a * OS + oh0, b * OS + ow0) of a map Wout wide
    int IS, r0, c0;           // its window starts at (a * IS + r0, b * IS + c0)
    int PH, PW, TH, TW, twsh, tilesA, tilesB;
    int C, cg, nchunk, ntaps, transposed;
    int poff[9], ftap[9];     // per tap: pixel offset inside the patch, index of the filter tap
    long i_ld_pix, i_ld_img, o_ld_pix, o_ld_img;
};

__device__ __forceinline__ sgx_f32x4 gc_mfma(float a, float b, sgx_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the 16 channels [c0, c0 + 16) of the PH x PW patch at (hi0, wi0) of one image
__device__ __forceinline__ void gc_stage_patch(const GcGeom& g, float* patch, const float* __restrict__ xb, int hi0, int wi0, int c0, int tid) {
    for (int i = tid; i < g.PH * g.PW * 4; i += GC_THREADS) {
        const int pix = i >> 2, q = (i & 3) * 4;
        const int hi = hi0 + pix / g.PW, wi = wi0 + pix % g.PW;
        const bool in = hi >= 0 && hi < g.Hi && wi >= 0 && wi < g.Wi && c0 + q < g.C;
        sgx_st4(patch + pix * GC_LD + q, in ? sgx_ld4(xb + ((long)hi * g.Wi + wi) * g.i_ld_pix + c0 + q) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// out = act(sum over taps and the group's channels + bias) (+ out when accumulate); partials: [2][gridDim.x][C] sum / sum of squares
template <int MT, int NB>
__global__ __launch_bounds__(GC_THREADS) void gconv_kernel(GcGeom g, const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, int act, int accumulate,
                                                           float* __restrict__ partials) {
    SGX_DYN_SMEM(float, smem);
    __shared__ float4 red[4][4];
    float* patch = smem;                                  // [PH * PW][GC_LD]
    float* fl = smem + (long)g.PH * g.PW * GC_LD;         // [3][NB * 16][GC_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    int t = blockIdx.x;
    const int tb = t % g.tilesB;
    t /= g.tilesB;
    const int ta = t % g.tilesA, img = t / g.tilesA;
    const int a0 = ta * g.TH, b0 = tb * g.TW;
    const int cbase = blockIdx.y * (NB * 16);
    int ppix[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = (wave * MT + mt) * 16 + li;
        ppix[mt] = ((p >> g.twsh) * g.IS * g.PW + (p & (g.TW - 1)) * g.IS) * GC_LD + lj;
    }
    sgx_f32x4 acc[MT][NB];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mt][nb] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ xb = x + (long)img * g.i_ld_img;
    for (int ch = 0; ch < g.nchunk; ++ch) {
        const int rb = cbase + ch * 16;  // first reduction channel of the chunk
        __syncthreads();
        gc_stage_patch(g, patch, xb, a0 * g.IS + g.r0, b0 * g.IS + g.c0, rb, tid);
        for (int t0 = 0; t0 < g.ntaps; t0 += 3) {
            if (t0) __syncthreads();
            const int nt = min(3, g.ntaps - t0);
            for (int i = tid; i < nt * NB * 64; i += GC_THREADS) {
                const int q = (i & 3) * 4, o = (i >> 2) % (NB * 16), tl = (i >> 2) / (NB * 16);
                const int co = cbase + o, rc = rb + q, tap = g.ftap[t0 + tl];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (co < g.C && rc < g.C && co / g.cg == rc / g.cg) {
                    if (!g.transposed) {
                        v = sgx_ld4(w + ((long)co * 9 + tap) * g.cg + rc % g.cg);
                    } else {  // data gradient: the reduction runs over the filter's output channels
                        const float* p = w + ((long)rc * 9 + tap) * g.cg + co % g.cg;
                        const long ld = 9L * g.cg;
                        v = make_float4(p[0], p[ld], p[2 * ld], p[3 * ld]);
                    }
                }
                sgx_st4(fl + (tl * NB * 16 + o) * GC_LD + q, v);
            }
            __syncthreads();
            for (int tl = 0; tl < nt; ++tl) {
                const int po = g.poff[t0 + tl] * GC_LD;
                const float* fa = fl + (tl * NB * 16 + li) * GC_LD + lj;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    float bv[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) bv[mt] = patch[ppix[mt] + po + 4 * ks];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const float av = fa[nb * 16 * GC_LD + 4 * ks];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) acc[mt][nb] = gc_mfma(av, bv[mt], acc[mt][nb]);
                    }
                }
            }
        }
    }
    // a lane holds channels cbase + nb * 16 + 4 lj .. + 3 of position li of its tiles
    float4 q0[NB], q1[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) q0[nb] = q1[nb] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = (wave * MT + mt) * 16 + li;
        const int a = a0 + (p >> g.twsh), b = b0 + (p & (g.TW - 1));
        const bool pix_ok = a < g.A && b < g.B;
        float* yp = y + (long)img * g.o_ld_img + ((long)(a * g.OS + g.oh0) * g.Wout + (b * g.OS + g.ow0)) * g.o_ld_pix;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = cbase + nb * 16 + 4 * lj;
            if (!(pix_ok && c < g.C)) continue;
            float4 v = make_float4(acc[mt][nb][0], acc[mt][nb][1], acc[mt][nb][2], acc[mt][nb][3]);
            if (partials) {
                q0[nb].x += v.x; q0[nb].y += v.y; q0[nb].z += v.z; q0[nb].w += v.w;
                q1[nb].x += v.x * v.x; q1[nb].y += v.y * v.y; q1[nb].z += v.z * v.z; q1[nb].w += v.w * v.w;
            }
            if (accumulate) {
                const float4 u = sgx_ld4(yp + c);
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            if (bias) {
                const float4 bb = sgx_ld4(bias + c);
                v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
            }
            sgx_st4(yp + c, make_float4(sgx_act(v.x, act), sgx_act(v.y, act), sgx_act(v.z, act), sgx_act(v.w, act)));
        }
    }
    if (partials) {  // the 16 position lanes in a fixed butterfly, then the four waves in order
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
                if (tid < 4 && c < g.C) {
                    float4 s = red[0][tid];
#pragma unroll
                    for (int k = 1; k < 4; ++k) { s.x += red[k][tid].x; s.y += red[k][tid].y; s.z += red[k][tid].z; s.w += red[k][tid].w; }
                    sgx_st4(partials + ((long)h * gridDim.x + blockIdx.x) * g.C + c, s);
                }
            }
    }
}

// Weight gradient, stage 1.  A workgroup owns the tiles [blockIdx.x * per_blk, ...) and ONE pair of 16-channel blocks of a group (kb: filter
// output channels = dy channels, cib: input channels): per tap a 16 x 16 tile dw[k][ci] = sum over positions of dy[p][k] * x[p + tap][ci],
// the reduction index being the position.  The four waves take every fourth step of four positions and meet in LDS in wave order; the
// workgroup leaves its partial in ws[blockIdx.x] in the filter's own layout, which dwconv_wgrad_fold_kernel adds to dw in a fixed order.
template <int MT>
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_kernel(GcGeom g, int per_blk, int ntiles, const float* __restrict__ x,
                                                                 const float* __restrict__ dy, float* __restrict__ ws) {
    SGX_DYN_SMEM(float, smem);
    float* patch = smem;                               // [PH * PW][GC_LD]
    float* dyt = smem + (long)g.PH * g.PW * GC_LD;      // [MT * 64][GC_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    int kb, cib;
    if (g.cg < 16) {
        kb = cib = blockIdx.y;
    } else {
        const int nb = g.cg / 16, grp = blockIdx.y / (nb * nb), r = blockIdx.y % (nb * nb);
        kb = grp * nb + r / nb;
        cib = grp * nb + r % nb;
    }
    sgx_f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    const int t_end = min(ntiles, (int)(blockIdx.x + 1) * per_blk);
    for (int tile = blockIdx.x * per_blk; tile < t_end; ++tile) {
        int t = tile;
        const int tb = t % g.tilesB;
        t /= g.tilesB;
        const int ta = t % g.tilesA, img = t / g.tilesA;
        const int a0 = ta * g.TH, b0 = tb * g.TW;
        __syncthreads();
        gc_stage_patch(g, patch, x + (long)img * g.i_ld_img, a0 * g.IS + g.r0, b0 * g.IS + g.c0, cib * 16, tid);
        for (int i = tid; i < MT * 64 * 4; i += GC_THREADS) {
            const int p = i >> 2, q = (i & 3) * 4;
            const int a = a0 + (p >> g.twsh), b = b0 + (p & (g.TW - 1));
            const bool in = a < g.A && b < g.B && kb * 16 + q < g.C;
            sgx_st4(dyt + p * GC_LD + q, in ? sgx_ld4(dy + (long)img * g.o_ld_img + ((long)a * g.Wout + b) * g.o_ld_pix + kb * 16 + q) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        __syncthreads();
        for (int ks = wave; ks < MT * 16; ks += 4) {
            const int p = 4 * ks + lj;
            const float av = dyt[p * GC_LD + li];
            const float* pb = patch + ((p >> g.twsh) * g.IS * g.PW + (p & (g.TW - 1)) * g.IS) * GC_LD + li;
#pragma unroll
            for (int t9 = 0; t9 < 9; ++t9) acc[t9] = gc_mfma(av, pb[g.poff[t9] * GC_LD], acc[t9]);
        }
    }
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(smem);  // [4 waves][9][64]
#pragma unroll
    for (int t = 0; t < 9; ++t) red[(wave * 9 + t) * 64 + lane] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    __syncthreads();
    float* out = ws + (long)blockIdx.x * g.C * 9 * g.cg;
    for (int i = tid; i < 9 * 64; i += GC_THREADS) {
        const int t = i >> 6, l = i & 63;
        float4 s = red[t * 64 + l];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float4 u = red[(k * 9 + t) * 64 + l];
            s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        const float sv[4] = {s.x, s.y, s.z, s.w};
        const int ci = cib * 16 + (l & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kb * 16 + 4 * (l >> 4) + r;
            if (k < g.C && ci < g.C && k / g.cg == ci / g.cg) out[((long)k * 9 + t) * g.cg + ci % g.cg] = sv[r];
        }
    }
}

static int32_t gc_check(const sgx_conv_desc* d, int32_t groups, const char* what) {
    int32_t rc = dw_check(d, what);  // K == C, 3x3 pad 1, stride 1 or 2, strides, extents
    if (rc) return rc;
    SGX_CHECK_ARG(groups > 1 && d->C % groups == 0, "%s: groups=%d must be above 1 and divide C=%d", what, groups, d->C);
    const int cg = d->C / groups;
    SGX_CHECK_ARG(cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64, "%s: %d channels per group are not built (4, 8, 16, 32 or 64)", what, cg);
    return SGX_OK;
}
// tiles of A x B positions: 16 columns (8 for narrow maps), 64 positions per workgroup when the whole map has no more, else 128
static void gc_tiles(GcGeom& g, int A, int B) {
    g.A = A; g.B = B;
    g.twsh = B > 8 ? 4 : 3;
    g.TW = 1 << g.twsh;
    const int mt = (long)A * B > 64 ? 2 : 1;
    g.TH = mt * 64 / g.TW;
    g.tilesA = sgx_cdiv(A, g.TH);
    g.tilesB = sgx_cdiv(B, g.TW);
}
static void gc_channels(GcGeom& g, const sgx_conv_desc* d, int groups) {
    g.N = d->N; g.C = d->C; g.cg = d->C / groups;
    g.nchunk = g.cg < 16 ? 1 : g.cg / 16;
}
// forward geometry (also the weight gradient's): positions are output pixels, the window walks x
static GcGeom gc_fwd_geom(const sgx_conv_desc* d, int groups) {
    GcGeom g;
    gc_channels(g, d, groups);
    g.Hi = d->H; g.Wi = d->W;
    gc_tiles(g, d->Ho, d->Wo);
    g.OS = 1; g.oh0 = g.ow0 = 0; g.Wout = d->Wo;
    g.IS = d->stride; g.r0 = g.c0 = -1;
    g.PH = (g.TH - 1) * g.IS + 3; g.PW = (g.TW - 1) * g.IS + 3;
    g.ntaps = 9; g.transposed = 0;
    for (int t = 0; t < 9; ++t) { g.poff[t] = (t / 3) * g.PW + t % 3; g.ftap[t] = t; }
    g.i_ld_pix = d->x_ld_pix; g.i_ld_img = d->x_ld_img; g.o_ld_pix = d->y_ld_pix; g.o_ld_img = d->y_ld_img;
    return g;
}
static bool gc_tiles_fit(const sgx_conv_desc* d, int groups) {
    const GcGeom g = gc_fwd_geom(d, groups);
    return (long)g.N * g.tilesA * g.tilesB < 0x7fffffffL;
}
// data gradient: positions are the dx pixels (2a + ph, 2b + pw) at stride 2 (every pixel at stride 1), the window walks dy
static GcGeom gc_dgrad_geom(const sgx_conv_desc* d, int groups, int ph, int pw) {
    GcGeom g;
    gc_channels(g, d, groups);
    g.Hi = d->Ho; g.Wi = d->Wo;
    g.Wout = d->W; g.IS = 1; g.transposed = 1; g.ntaps = 0;
    int nr, nc, rr[3], dr[3], cc[3], dc[3];
    if (d->stride == 1) {
        gc_tiles(g, d->H, d->W);
        g.OS = 1; g.oh0 = g.ow0 = 0; g.r0 = g.c0 = -1;
        nr = nc = 3;
        for (int r = 0; r < 3; ++r) { rr[r] = cc[r] = r; dr[r] = dc[r] = 2 - r; }  // dy row = hi + 1 - r: patch row (1 - r) - r0
    } else {
        gc_tiles(g, (d->H - ph + 1) / 2, (d->W - pw + 1) / 2);
        g.OS = 2; g.oh0 = ph; g.ow0 = pw; g.r0 = g.c0 = 0;
        // even rows: tap 1 at ho = a; odd rows: tap 2 at ho = a and tap 0 at ho = a + 1
        nr = ph ? 2 : 1; rr[0] = ph ? 2 : 1; dr[0] = 0; rr[1] = 0; dr[1] = 1;
        nc = pw ? 2 : 1; cc[0] = pw ? 2 : 1; dc[0] = 0; cc[1] = 0; dc[1] = 1;
    }
    const int span_r = d->stride == 1 ? 2 : ph, span_c = d->stride == 1 ? 2 : pw;
    g.PH = g.TH + span_r; g.PW = g.TW + span_c;
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) {
            g.poff[g.ntaps] = dr[i] * g.PW + dc[j];
            g.ftap[g.ntaps++] = rr[i] * 3 + cc[j];
        }
    for (int t = g.ntaps; t < 9; ++t) g.poff[t] = g.ftap[t] = 0;
    g.i_ld_pix = d->y_ld_pix; g.i_ld_img = d->y_ld_img; g.o_ld_pix = d->x_ld_pix; g.o_ld_img = d->x_ld_img;
    return g;
}
static int32_t gc_launch(const GcGeom& g, const float* x, const float* w, const float* bias, float* y, int act, int accumulate, float* partials,
                         void* stream, const char* what) {
    const int nb = g.cg < 16 ? 1 : g.cg / 16, mt = g.TH * g.TW / 64;
    const long nblk = (long)g.N * g.tilesA * g.tilesB;
    const long lds = ((long)g.PH * g.PW + 3L * nb * 16) * GC_LD * 4;
    SGX_CHECK_ARG(nblk < 0x7fffffffL && lds <= 65536, "%s: tile outside the launch limits", what);
    const dim3 grid((unsigned)nblk, (unsigned)sgx_cdiv(g.C, nb * 16));
#define GC_GO(MT_, NB_) SGX_LAUNCH((gconv_kernel<MT_, NB_>), grid, dim3(GC_THREADS), (unsigned)lds, stream, g, x, w, bias, y, act, accumulate, partials)
    if (mt == 1) {
        if (nb == 1) GC_GO(1, 1);
        else if (nb == 2) GC_GO(1, 2);
        else GC_GO(1, 4);
    } else {
        if (nb == 1) GC_GO(2, 1);
        else if (nb == 2) GC_GO(2, 2);
        else GC_GO(2, 4);
    }
#undef GC_GO
    SGX_CHECK_LAUNCH(what);
    return SGX_OK;
}

extern "C" int32_t sgx_gconv3x3_stat_blocks(const sgx_conv_desc* d, int32_t groups) {
    if (gc_check(d, groups, "gconv3x3_stat_blocks") || !gc_tiles_fit(d, groups)) return 0;
    const GcGeom g = gc_fwd_geom(d, groups);
    return (int32_t)((long)g.N * g.tilesA * g.tilesB);
}
extern "C" int32_t sgx_gconv3x3_fwd(const sgx_conv_desc* d, int32_t groups, const float* x, const float* w, const float* bias, float* y, int32_t act,
                                    float* stat_partials, void* stream) {
    int32_t rc = gc_check(d, groups, "gconv3x3_fwd");
    if (rc) return rc;
    SGX_CHECK_ARG(x && w && y, "gconv3x3_fwd: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(w) && DW_ALIGNED(y) && DW_ALIGNED(bias) && DW_ALIGNED(stat_partials), "gconv3x3_fwd: operands must be 16-byte aligned");
    SGX_CHECK_ACT3(act, "gconv3x3_fwd");
    SGX_CHECK_ARG(!stat_partials || (!bias && act == SGX_ACT_NONE), "gconv3x3_fwd: statistics rows go with the plain convolution (no bias, no activation)");
    return gc_launch(gc_fwd_geom(d, groups), x, w, bias, y, act, 0, stat_partials, stream, "gconv3x3_fwd");
}
extern "C" int64_t sgx_gconv3x3_bwd_data_workspace(const sgx_conv_desc* d, int32_t groups) {
    (void)d; (void)groups;
    return 0;  // the filter is read transposed while it is staged
}
extern "C" int32_t sgx_gconv3x3_bwd_data(const sgx_conv_desc* d, int32_t groups, const float* dy, const float* w, float* dx, int32_t accumulate,
                                         void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    int32_t rc = gc_check(d, groups, "gconv3x3_bwd_data");
    if (rc) return rc;
    SGX_CHECK_ARG(dy && w && dx, "gconv3x3_bwd_data: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(dy) && DW_ALIGNED(w) && DW_ALIGNED(dx), "gconv3x3_bwd_data: operands must be 16-byte aligned");
    if (d->stride == 1) return gc_launch(gc_dgrad_geom(d, groups, 0, 0), dy, w, nullptr, dx, SGX_ACT_NONE, accumulate ? 1 : 0, nullptr, stream, "gconv3x3_bwd_data");
    for (int cls = 0; cls < 4; ++cls) {
        const GcGeom g = gc_dgrad_geom(d, groups, cls >> 1, cls & 1);
        if (g.A <= 0 || g.B <= 0) continue;  // (a map of one row has no odd rows)
        rc = gc_launch(g, dy, w, nullptr, dx, SGX_ACT_NONE, accumulate ? 1 : 0, nullptr, stream, "gconv3x3_bwd_data");
        if (rc) return rc;
    }
    return SGX_OK;
}
// weight gradient: ~1024 workgroups unless the problem has fewer tiles (every workgroup leaves a 9 x 16 x 16 partial)
#define GC_WGRAD_BLOCKS 1024
static GcGeom gc_wgrad_geom(const sgx_conv_desc* d, int groups, int* npairs, int* nsplit, int* per_blk, int* ntiles) {
    const GcGeom g = gc_fwd_geom(d, groups);
    const int nb = g.cg / 16;
    *npairs = g.cg < 16 ? sgx_cdiv(g.C, 16) : groups * nb * nb;
    *ntiles = g.N * g.tilesA * g.tilesB;  // (callers checked gc_tiles_fit)
    long n = *ntiles;
    const long cap = SGX_STRIDE_GRID(sgx_cdiv(GC_WGRAD_BLOCKS, *npairs));  // (two splits on the host emulation, as dw_wgrad_geom)
    if (n > cap) n = cap;
    *per_blk = (int)((*ntiles + n - 1) / n);
    *nsplit = sgx_cdiv(*ntiles, *per_blk);
    return g;
}
extern "C" int64_t sgx_gconv3x3_bwd_weight_workspace(const sgx_conv_desc* d, int32_t groups) {
    if (gc_check(d, groups, "gconv3x3_bwd_weight_workspace") || !gc_tiles_fit(d, groups)) return 0;
    int npairs, nsplit, per_blk, ntiles;
    const GcGeom g = gc_wgrad_geom(d, groups, &npairs, &nsplit, &per_blk, &ntiles);
    return (int64_t)nsplit * g.C * 9 * g.cg * (int64_t)sizeof(float);
}
extern "C" int32_t sgx_gconv3x3_bwd_weight(const sgx_conv_desc* d, int32_t groups, const float* x, const float* dy, float* dw, void* ws, int64_t ws_bytes,
                                           void* stream) {
    int32_t rc = gc_check(d, groups, "gconv3x3_bwd_weight");
    if (rc) return rc;
    SGX_CHECK_ARG(x && dy && dw, "gconv3x3_bwd_weight: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(dy) && DW_ALIGNED(dw), "gconv3x3_bwd_weight: operands must be 16-byte aligned");
    SGX_CHECK_ARG(gc_tiles_fit(d, groups), "gconv3x3_bwd_weight: more than 2^31 position tiles");
    int npairs, nsplit, per_blk, ntiles;
    const GcGeom g = gc_wgrad_geom(d, groups, &npairs, &nsplit, &per_blk, &ntiles);
    const long ncol = (long)g.C * 9 * g.cg;
    if (!ws || ws_bytes < (int64_t)nsplit * ncol * (int64_t)sizeof(float) || ((uintptr_t)ws % 16) != 0)
        SGX_FAIL(SGX_ERR_WORKSPACE, "gconv3x3_bwd_weight: workspace too small or unaligned (sgx_gconv3x3_bwd_weight_workspace)");
    const int mt = g.TH * g.TW / 64;
    long lds = ((long)g.PH * g.PW + mt * 64) * GC_LD * 4;
    if (lds < 4L * 9 * 64 * 16) lds = 4L * 9 * 64 * 16;  // the waves' accumulators meet in the same buffer
    SGX_CHECK_ARG(lds <= 65536 && ncol < 0x7fffffffL, "gconv3x3_bwd_weight: tile outside the launch limits");
    const dim3 grid((unsigned)nsplit, (unsigned)npairs);
    if (mt == 1) SGX_LAUNCH(gconv_wgrad_kernel<1>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, per_blk, ntiles, x, dy, (float*)ws);
    else SGX_LAUNCH(gconv_wgrad_kernel<2>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, per_blk, ntiles, x, dy, (float*)ws);
    SGX_CHECK_LAUNCH("gconv3x3_bwd_weight");
    SGX_LAUNCH(dwconv_wgrad_fold_kernel, dim3((unsigned)sgx_cdiv(ncol, 16)), dim3(DW_THREADS), 0, stream, (const float*)ws, nsplit, (int)ncol, dw);
    SGX_CHECK_LAUNCH("gconv3x3_bwd_weight (fold)");
    return SGX_OK;
}
