// Split-dilation grouped 3x3 convolution, stride 1, 16 channels per group (RegSeg's DBlock): forward, data gradient, weight gradient.
// Included by pool.hip behind gconv.h (its tiles, its MFMA operand mapping and LDS row pitch, the depthwise fold kernel).
//
// The C channels are cut into nsplit equal splits; split i is a grouped 3x3 convolution with pad = dilation = dil[i] and its own filter
// [C / nsplit][3][3][16].  ONE launch serves every split: blockIdx.y is a block of 16 output channels = one group, which lies in one split
// and so has one dilation; x and y are whole [N,H,W,C] tensors (or channel slices), no split or concat pass exists.
// Tiles are gconv's: a workgroup (four waves) owns TH x TW positions of one image, a wave MT tiles of 16 channels x 16 positions of
// v_mfma_f32_16x16x4_f32 with the filter as A and the pixels as B - a lane ends with four consecutive channels of one pixel.
// The group's whole filter (9 taps x 16 x 16) is staged once.  How the nine dilated taps reach LDS is chosen per split ON THE HOST:
//   halo    the (TH + 2d) x (TW + 2d) patch once, while it has at most DG_HALO_PIX pixels (the largest patch a gconv launch stages);
//   band    per filter row r the TH x (TW + 2d) band at row offset (r - 1) d: its three taps are the column offsets 0, d, 2d;
//   tiles   the band when d > TW: the columns between its taps are never read, so the three TH x TW tiles are staged side by side.
// The band is at most TH x 3 TW = 384 pixels, so every d fits.  Pixels outside the map are staged as zeros; a tap (a whole band) whose
// shifted tile lies outside the map is skipped - a 4 x 4 map at d = 14 runs the centre tap alone.
// The data gradient is the same kernel: the staged map is dy, the taps are reversed and the filter is read transposed (a gather).
#pragma once

#define DG_MAX_SPLITS 4
#define DG_HALO_PIX 561  // 17 x 33: gconv's stride-2 patch under an 8 x 16 tile
#define DG_FILTER (9 * 16 * GC_LD)  // floats of the staged filter
#define DG_FORM_HALO 0
#define DG_FORM_BAND 1
#define DG_FORM_TILES 2
struct DgGeom {
    int N, H, W, C, cs;  // cs: channels per split
    int TH, TW, twsh, tilesA, tilesB, transposed;
    int dil[DG_MAX_SPLITS], form[DG_MAX_SPLITS];
    long i_ld_pix, i_ld_img, o_ld_pix, o_ld_img;
};
struct DgPtrs {
    float* p[DG_MAX_SPLITS];
};
// what one workgroup needs of its split
struct DgSplit {
    int s, d, form, PH, PW, cstep;  // cstep: patch columns between two taps of a row
};
__device__ __forceinline__ DgSplit dg_split(const DgGeom& g, int cbase) {
    DgSplit sp;
    sp.s = cbase / g.cs;
    sp.d = g.dil[sp.s];
    sp.form = g.form[sp.s];
    sp.PH = sp.form == DG_FORM_HALO ? g.TH + 2 * sp.d : g.TH;
    sp.PW = sp.form == DG_FORM_TILES ? 3 * g.TW : g.TW + 2 * sp.d;
    sp.cstep = sp.form == DG_FORM_TILES ? g.TW : sp.d;
    return sp;
}
// the 16 channels [c0, c0 + 16) of the patch whose first row is map row hi0; its columns start at b0 - d (three tiles: at b0 + (k - 1) d)
__device__ __forceinline__ void dg_stage(const DgGeom& g, const DgSplit& sp, float* patch, const float* __restrict__ xb, int hi0, int b0, int c0, int tid) {
    for (int i = tid; i < sp.PH * sp.PW * 4; i += GC_THREADS) {
        const int pix = i >> 2, q = (i & 3) * 4;
        const int pr = pix / sp.PW, pq = pix - pr * sp.PW;
        const int hi = hi0 + pr;
        const int wi = sp.form == DG_FORM_TILES ? b0 + ((pq >> g.twsh) - 1) * sp.d + (pq & (g.TW - 1)) : b0 - sp.d + pq;
        const bool in = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
        sgx_st4(patch + pix * GC_LD + q, in ? sgx_ld4(xb + ((long)hi * g.W + wi) * g.i_ld_pix + c0 + q) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}
// does the tile [lo, lo + n) shifted by (k - 1) d meet [0, size)?
__device__ __forceinline__ bool dg_meets(int lo, int n, int k, int d, int size) { return lo + (k - 1) * d < size && lo + n - 1 + (k - 1) * d >= 0; }

// out = act(sum over the taps and the group's 16 channels + bias) (+ out when accumulate); partials: [2][gridDim.x][C] sum / sum of squares
template <int MT>
__global__ __launch_bounds__(GC_THREADS) void dgconv_kernel(DgGeom g, DgPtrs wp, const float* __restrict__ x, const float* __restrict__ bias,
                                                            float* __restrict__ y, int act, int accumulate, float* __restrict__ partials) {
    SGX_DYN_SMEM(float, smem);
    __shared__ float4 red[4][4];
    float* fl = smem;                // [9][16][GC_LD]
    float* patch = smem + DG_FILTER;  // [PH * PW][GC_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    int t = blockIdx.x;
    const int tb = t % g.tilesB;
    t /= g.tilesB;
    const int ta = t % g.tilesA, img = t / g.tilesA;
    const int a0 = ta * g.TH, b0 = tb * g.TW;
    const int th = min(g.TH, g.H - a0), tw = min(g.TW, g.W - b0);  // the part of the tile inside the map
    const int cbase = blockIdx.y * 16;
    const DgSplit sp = dg_split(g, cbase);
    const float* __restrict__ w = wp.p[sp.s] + (long)(cbase - sp.s * g.cs) * 144;
    for (int i = tid; i < 9 * 64; i += GC_THREADS) {
        const int q = (i & 3) * 4, o = (i >> 2) & 15, tap = i >> 6;
        float4 v;
        if (!g.transposed) {
            v = sgx_ld4(w + (o * 9 + tap) * 16 + q);
        } else {  // data gradient: the reduction runs over the filter's output channels
            const float* p = w + (q * 9 + tap) * 16 + o;
            v = make_float4(p[0], p[144], p[288], p[432]);
        }
        sgx_st4(fl + (tap * 16 + o) * GC_LD + q, v);
    }
    int ppix[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = (wave * MT + mt) * 16 + li;
        ppix[mt] = ((p >> g.twsh) * sp.PW + (p & (g.TW - 1))) * GC_LD + lj;
    }
    sgx_f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = sgx_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ xb = x + (long)img * g.i_ld_img;
    const int nstage = sp.form == DG_FORM_HALO ? 1 : 3;
    for (int st = 0; st < nstage; ++st) {
        const int r_lo = nstage == 1 ? 0 : st, r_hi = nstage == 1 ? 3 : st + 1;  // patch rows of taps this stage holds
        if (nstage == 3 && !dg_meets(a0, th, st, sp.d, g.H)) continue;            // (workgroup-uniform)
        __syncthreads();
        dg_stage(g, sp, patch, xb, a0 + (r_lo - 1) * sp.d, b0, cbase, tid);
        __syncthreads();
        for (int r = r_lo; r < r_hi; ++r) {
            if (!dg_meets(a0, th, r, sp.d, g.H)) continue;
            for (int c = 0; c < 3; ++c) {
                if (!dg_meets(b0, tw, c, sp.d, g.W)) continue;
                const int po = ((r - r_lo) * sp.d * sp.PW + c * sp.cstep) * GC_LD;
                const int tap = g.transposed ? 8 - (r * 3 + c) : r * 3 + c;
                const float* fa = fl + (tap * 16 + li) * GC_LD + lj;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const float av = fa[4 * ks];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt] = gc_mfma(av, patch[ppix[mt] + po + 4 * ks], acc[mt]);
                }
            }
        }
    }
    // a lane holds channels cbase + 4 lj .. + 3 of position li of its tiles
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    const int c = cbase + 4 * lj;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int p = (wave * MT + mt) * 16 + li;
        const int a = a0 + (p >> g.twsh), b = b0 + (p & (g.TW - 1));
        if (!(a < g.H && b < g.W)) continue;
        float* yp = y + (long)img * g.o_ld_img + ((long)a * g.W + b) * g.o_ld_pix + c;
        float4 v = make_float4(acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]);
        if (partials) {
            q0.x += v.x; q0.y += v.y; q0.z += v.z; q0.w += v.w;
            q1.x += v.x * v.x; q1.y += v.y * v.y; q1.z += v.z * v.z; q1.w += v.w * v.w;
        }
        if (accumulate) {
            const float4 u = sgx_ld4(yp);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        if (bias) {
            const float4 bb = sgx_ld4(bias + c);
            v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
        }
        sgx_st4(yp, make_float4(sgx_act(v.x, act), sgx_act(v.y, act), sgx_act(v.z, act), sgx_act(v.w, act)));
    }
    if (partials) {  // the 16 position lanes in a fixed butterfly, then the four waves in order
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 q = h ? q1 : q0;
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                q.x += __shfl_xor(q.x, m); q.y += __shfl_xor(q.y, m); q.z += __shfl_xor(q.z, m); q.w += __shfl_xor(q.w, m);
            }
            __syncthreads();
            if (li == 0) red[wave][lj] = q;
            __syncthreads();
            if (tid < 4) {
                float4 s = red[0][tid];
#pragma unroll
                for (int k = 1; k < 4; ++k) { s.x += red[k][tid].x; s.y += red[k][tid].y; s.z += red[k][tid].z; s.w += red[k][tid].w; }
                sgx_st4(partials + ((long)h * gridDim.x + blockIdx.x) * g.C + cbase + 4 * tid, s);
            }
        }
    }
}

// Weight gradient, stage 1.  A workgroup owns the tiles [blockIdx.x * per_blk, ...) and one group (blockIdx.y): per tap the 16 x 16 tile
// dw[k][ci] = sum over positions of dy[p][k] * x[p + (tap - 1) d][ci], the reduction index being the position; x is staged in the split's
// form (halo once per tile, bands one filter row at a time), dy once per tile.  The four waves take every fourth step of four positions
// and meet in LDS in wave order; the partial goes to ws[split][blockIdx.x] in the split filter's own layout for dwconv_wgrad_fold_kernel.
template <int MT>
__global__ __launch_bounds__(GC_THREADS) void dgconv_wgrad_kernel(DgGeom g, int per_blk, int ntiles, const float* __restrict__ x,
                                                                  const float* __restrict__ dy, float* __restrict__ ws) {
    SGX_DYN_SMEM(float, smem);
    float* dyt = smem;                         // [MT * 64][GC_LD]
    float* patch = smem + MT * 64 * GC_LD;     // [PH * PW][GC_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lj = lane >> 4;
    const int cbase = blockIdx.y * 16;
    const DgSplit sp = dg_split(g, cbase);
    const int nstage = sp.form == DG_FORM_HALO ? 1 : 3;
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
        const int th = min(g.TH, g.H - a0), tw = min(g.TW, g.W - b0);
        __syncthreads();
        for (int i = tid; i < MT * 64 * 4; i += GC_THREADS) {
            const int p = i >> 2, q = (i & 3) * 4;
            const int a = a0 + (p >> g.twsh), b = b0 + (p & (g.TW - 1));
            const bool in = a < g.H && b < g.W;
            sgx_st4(dyt + p * GC_LD + q, in ? sgx_ld4(dy + (long)img * g.o_ld_img + ((long)a * g.W + b) * g.o_ld_pix + cbase + q) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        for (int st = 0; st < nstage; ++st) {
            const int r_lo = nstage == 1 ? 0 : st;
            if (nstage == 3 && !dg_meets(a0, th, st, sp.d, g.H)) continue;
            if (st) __syncthreads();
            dg_stage(g, sp, patch, x + (long)img * g.i_ld_img, a0 + (r_lo - 1) * sp.d, b0, cbase, tid);
            __syncthreads();
            bool on[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) on[c] = dg_meets(b0, tw, c, sp.d, g.W);
            for (int ks = wave; ks < MT * 16; ks += 4) {
                const int p = 4 * ks + lj;
                const float av = dyt[p * GC_LD + li];
                const float* pb = patch + ((p >> g.twsh) * sp.PW + (p & (g.TW - 1))) * GC_LD + li;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    if (nstage == 3 ? r != st : !dg_meets(a0, th, r, sp.d, g.H)) continue;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (on[c]) acc[r * 3 + c] = gc_mfma(av, pb[((r - r_lo) * sp.d * sp.PW + c * sp.cstep) * GC_LD], acc[r * 3 + c]);
                }
            }
        }
    }
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(smem);  // [4 waves][9][64]
#pragma unroll
    for (int t = 0; t < 9; ++t) red[(wave * 9 + t) * 64 + lane] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    __syncthreads();
    // ws: [nsplit][gridDim.x][cs * 144]
    float* out = ws + ((long)sp.s * gridDim.x + blockIdx.x) * g.cs * 144 + (long)(cbase - sp.s * g.cs) * 144;
    for (int i = tid; i < 9 * 64; i += GC_THREADS) {
        const int t = i >> 6, l = i & 63;
        float4 s = red[t * 64 + l];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float4 u = red[(k * 9 + t) * 64 + l];
            s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
        const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) out[((4 * (l >> 4) + r) * 9 + t) * 16 + (l & 15)] = sv[r];
    }
}

static int32_t dg_check(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil, const char* what) {
    int32_t rc = dw_check(d, what);  // K == C, 3x3, the descriptor's pad 1 (= "same" extents: a split pads by its own dilation), strides
    if (rc) return rc;
    SGX_CHECK_ARG(d->stride == 1, "%s: stride %d is not built (the dilated kernels are stride 1)", what, d->stride);
    SGX_CHECK_ARG(cg == 16, "%s: %d channels per group are not built (16)", what, cg);
    SGX_CHECK_ARG(nsplit >= 1 && nsplit <= DG_MAX_SPLITS && d->C % nsplit == 0, "%s: %d splits must be 1 .. %d and divide C=%d", what, nsplit, DG_MAX_SPLITS, d->C);
    SGX_CHECK_ARG((d->C / nsplit) % cg == 0, "%s: %d channels per split are no multiple of the group width %d", what, d->C / nsplit, cg);
    SGX_CHECK_ARG(dil, "%s: null dilation list", what);
    for (int i = 0; i < nsplit; ++i) SGX_CHECK_ARG(dil[i] >= 1 && dil[i] <= 4096, "%s: dilation %d of split %d must be 1 .. 4096", what, dil[i], i);
    return SGX_OK;
}
static int dg_form(int TH, int TW, int d) {
    if ((long)(TH + 2 * d) * (TW + 2 * d) <= DG_HALO_PIX) return DG_FORM_HALO;
    return d > TW ? DG_FORM_TILES : DG_FORM_BAND;
}
// transposed: the data gradient (the staged map is dy, the stored one dx)
static DgGeom dg_geom(const sgx_conv_desc* d, int nsplit, const int32_t* dil, int transposed) {
    DgGeom g;
    GcGeom t;
    gc_tiles(t, d->H, d->W);
    g.N = d->N; g.H = d->H; g.W = d->W; g.C = d->C; g.cs = d->C / nsplit;
    g.TH = t.TH; g.TW = t.TW; g.twsh = t.twsh; g.tilesA = t.tilesA; g.tilesB = t.tilesB;
    g.transposed = transposed;
    for (int i = 0; i < DG_MAX_SPLITS; ++i) {
        g.dil[i] = i < nsplit ? dil[i] : 1;
        g.form[i] = dg_form(g.TH, g.TW, g.dil[i]);
    }
    g.i_ld_pix = transposed ? d->y_ld_pix : d->x_ld_pix; g.i_ld_img = transposed ? d->y_ld_img : d->x_ld_img;
    g.o_ld_pix = transposed ? d->x_ld_pix : d->y_ld_pix; g.o_ld_img = transposed ? d->x_ld_img : d->y_ld_img;
    return g;
}
// pixels of the largest patch any split of the launch stages
static long dg_patch_pix(const DgGeom& g, int nsplit) {
    long m = 0;
    for (int i = 0; i < nsplit; ++i) {
        const int dd = g.dil[i], f = g.form[i];
        const long pix = f == DG_FORM_HALO ? (long)(g.TH + 2 * dd) * (g.TW + 2 * dd) : (long)g.TH * (f == DG_FORM_TILES ? 3 * g.TW : g.TW + 2 * dd);
        if (pix > m) m = pix;
    }
    return m;
}
static int32_t dg_filters(DgPtrs& wp, const float* const* w, int nsplit, const char* what) {
    SGX_CHECK_ARG(w, "%s: null filter list", what);
    for (int i = 0; i < DG_MAX_SPLITS; ++i) {
        wp.p[i] = i < nsplit ? const_cast<float*>(w[i]) : nullptr;
        SGX_CHECK_ARG(i >= nsplit || (wp.p[i] && DW_ALIGNED(wp.p[i])), "%s: filter %d is null or not 16-byte aligned", what, i);
    }
    return SGX_OK;
}
static int32_t dg_launch(const DgGeom& g, int nsplit, const DgPtrs& wp, const float* x, const float* bias, float* y, int act, int accumulate,
                         float* partials, void* stream, const char* what) {
    const long nblk = (long)g.N * g.tilesA * g.tilesB;
    const long lds = (DG_FILTER + dg_patch_pix(g, nsplit) * GC_LD) * 4;
    SGX_CHECK_ARG(nblk < 0x7fffffffL && lds <= 65536, "%s: tile outside the launch limits", what);
    const dim3 grid((unsigned)nblk, (unsigned)(g.C / 16));
    if (g.TH * g.TW == 64) SGX_LAUNCH(dgconv_kernel<1>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, wp, x, bias, y, act, accumulate, partials);
    else SGX_LAUNCH(dgconv_kernel<2>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, wp, x, bias, y, act, accumulate, partials);
    SGX_CHECK_LAUNCH(what);
    return SGX_OK;
}

extern "C" int32_t sgx_debug_dgconv3x3_form(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil, int32_t split) {
    int32_t rc = dg_check(d, cg, nsplit, dil, "debug_dgconv3x3_form");
    if (rc) return rc;
    SGX_CHECK_ARG(split >= 0 && split < nsplit, "debug_dgconv3x3_form: split %d of %d", split, nsplit);
    return dg_geom(d, nsplit, dil, 0).form[split];
}
extern "C" int32_t sgx_dgconv3x3_stat_blocks(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil) {
    if (dg_check(d, cg, nsplit, dil, "dgconv3x3_stat_blocks")) return 0;
    const DgGeom g = dg_geom(d, nsplit, dil, 0);
    const long n = (long)g.N * g.tilesA * g.tilesB;
    return n < 0x7fffffffL ? (int32_t)n : 0;
}
extern "C" int32_t sgx_dgconv3x3_fwd(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil, const float* const* w, const float* x,
                                     const float* bias, float* y, int32_t act, float* stat_partials, void* stream) {
    int32_t rc = dg_check(d, cg, nsplit, dil, "dgconv3x3_fwd");
    if (rc) return rc;
    DgPtrs wp;
    if ((rc = dg_filters(wp, w, nsplit, "dgconv3x3_fwd"))) return rc;
    SGX_CHECK_ARG(x && y, "dgconv3x3_fwd: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(y) && DW_ALIGNED(bias) && DW_ALIGNED(stat_partials), "dgconv3x3_fwd: operands must be 16-byte aligned");
    SGX_CHECK_ACT3(act, "dgconv3x3_fwd");
    SGX_CHECK_ARG(!stat_partials || (!bias && act == SGX_ACT_NONE), "dgconv3x3_fwd: statistics rows go with the plain convolution (no bias, no activation)");
    return dg_launch(dg_geom(d, nsplit, dil, 0), nsplit, wp, x, bias, y, act, 0, stat_partials, stream, "dgconv3x3_fwd");
}
extern "C" int32_t sgx_dgconv3x3_bwd_data(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil, const float* dy, const float* const* w,
                                          float* dx, int32_t accumulate, void* stream) {
    int32_t rc = dg_check(d, cg, nsplit, dil, "dgconv3x3_bwd_data");
    if (rc) return rc;
    DgPtrs wp;
    if ((rc = dg_filters(wp, w, nsplit, "dgconv3x3_bwd_data"))) return rc;
    SGX_CHECK_ARG(dy && dx, "dgconv3x3_bwd_data: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(dy) && DW_ALIGNED(dx), "dgconv3x3_bwd_data: operands must be 16-byte aligned");
    return dg_launch(dg_geom(d, nsplit, dil, 1), nsplit, wp, dy, nullptr, dx, SGX_ACT_NONE, accumulate ? 1 : 0, nullptr, stream, "dgconv3x3_bwd_data");
}
// weight gradient: ~GC_WGRAD_BLOCKS workgroups unless the problem has fewer tiles (every workgroup leaves a 9 x 16 x 16 partial)
static DgGeom dg_wgrad_geom(const sgx_conv_desc* d, int nsplit, const int32_t* dil, int* nblk, int* per_blk, int* ntiles) {
    const DgGeom g = dg_geom(d, nsplit, dil, 0);
    const long tiles = (long)g.N * g.tilesA * g.tilesB;
    *ntiles = tiles < 0x7fffffffL ? (int)tiles : 0;
    long n = *ntiles;
    const long cap = SGX_STRIDE_GRID(sgx_cdiv(GC_WGRAD_BLOCKS, g.C / 16));  // (two workgroups per group on the host emulation, as gc_wgrad_geom)
    if (n > cap) n = cap;
    *per_blk = n ? (int)((*ntiles + n - 1) / n) : 1;
    *nblk = sgx_cdiv(*ntiles, *per_blk);
    return g;
}
extern "C" int64_t sgx_dgconv3x3_bwd_weight_workspace(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil) {
    if (dg_check(d, cg, nsplit, dil, "dgconv3x3_bwd_weight_workspace")) return 0;
    int nblk, per_blk, ntiles;
    const DgGeom g = dg_wgrad_geom(d, nsplit, dil, &nblk, &per_blk, &ntiles);
    return (int64_t)nblk * g.C * 144 * (int64_t)sizeof(float);
}
extern "C" int32_t sgx_dgconv3x3_bwd_weight(const sgx_conv_desc* d, int32_t cg, int32_t nsplit, const int32_t* dil, const float* x, const float* dy,
                                            float* const* dw, void* ws, int64_t ws_bytes, void* stream) {
    int32_t rc = dg_check(d, cg, nsplit, dil, "dgconv3x3_bwd_weight");
    if (rc) return rc;
    DgPtrs dp;
    if ((rc = dg_filters(dp, dw, nsplit, "dgconv3x3_bwd_weight"))) return rc;
    SGX_CHECK_ARG(x && dy, "dgconv3x3_bwd_weight: null pointer");
    SGX_CHECK_ARG(DW_ALIGNED(x) && DW_ALIGNED(dy), "dgconv3x3_bwd_weight: operands must be 16-byte aligned");
    int nblk, per_blk, ntiles;
    const DgGeom g = dg_wgrad_geom(d, nsplit, dil, &nblk, &per_blk, &ntiles);
    SGX_CHECK_ARG(ntiles > 0, "dgconv3x3_bwd_weight: more than 2^31 position tiles");
    const long ncol = (long)g.cs * 144;  // one split's filter
    if (!ws || ws_bytes < (int64_t)nblk * g.C * 144 * (int64_t)sizeof(float) || ((uintptr_t)ws % 16) != 0)
        SGX_FAIL(SGX_ERR_WORKSPACE, "dgconv3x3_bwd_weight: workspace too small or unaligned (sgx_dgconv3x3_bwd_weight_workspace)");
    const int mt = g.TH * g.TW / 64;
    long lds = ((long)mt * 64 + dg_patch_pix(g, nsplit)) * GC_LD * 4;
    if (lds < 4L * 9 * 64 * 16) lds = 4L * 9 * 64 * 16;  // the waves' accumulators meet in the same buffer
    SGX_CHECK_ARG(lds <= 65536 && ncol < 0x7fffffffL, "dgconv3x3_bwd_weight: tile outside the launch limits");
    const dim3 grid((unsigned)nblk, (unsigned)(g.C / 16));
    if (mt == 1) SGX_LAUNCH(dgconv_wgrad_kernel<1>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, per_blk, ntiles, x, dy, (float*)ws);
    else SGX_LAUNCH(dgconv_wgrad_kernel<2>, grid, dim3(GC_THREADS), (unsigned)lds, stream, g, per_blk, ntiles, x, dy, (float*)ws);
    SGX_CHECK_LAUNCH("dgconv3x3_bwd_weight");
    for (int s = 0; s < nsplit; ++s) {  // one fold per split: each has its own filter tensor
        SGX_LAUNCH(dwconv_wgrad_fold_kernel, dim3((unsigned)sgx_cdiv(ncol, 16)), dim3(DW_THREADS), 0, stream, (const float*)ws + (long)s * nblk * ncol, nblk, (int)ncol, dp.p[s]);
        SGX_CHECK_LAUNCH("dgconv3x3_bwd_weight (fold)");
    }
    return SGX_OK;
}
