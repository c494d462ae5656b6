// Per-pixel softmax cross-entropy and confusion counts over the class planes of an NCHW logit map (segmentation training).
// Included by loss.hip (after ce_reduce_kernel, which folds the cross-entropy's per-workgroup partial sums).
//
// The map is [N, C, P] with P = H * W contiguous floats per class plane.  LANES RUN ALONG THE PIXEL AXIS: a workgroup of SEG_THREADS lanes
// owns a chunk of SEG_CHUNK = SEG_THREADS * SEG_PIX consecutive pixels of ONE image and loops over the C planes, so every load and store of
// a wave is one contiguous run of a plane and the softmax of a pixel never leaves its lane (no cross-lane exchange per pixel, no NHWC copy).
//   VEC  (P % 4 == 0 and 16-byte aligned bases): a lane owns 4 ADJACENT pixels - one 16-byte load / store per plane, two per label quad.
//   !VEC (P % 4 != 0: the bases of planes >= 1 are not 16-byte aligned): a lane owns 4 pixels SEG_THREADS apart - coalesced 4-byte accesses.
// Pixels past P (the ragged last chunk) are dead: loaded as nothing, stored nowhere, labelled "no contribution"; their lanes stay in the
// kernel for the reductions and barriers.
#pragma once
#include <atomic>

#define SEG_THREADS 256
#define SEG_PIX 4
#define SEG_CHUNK (SEG_THREADS * SEG_PIX)
// seg_ce's two forms: C <= SEG_CE_REG_CAP keeps a lane's C x 4 logits in registers (128 value registers at the cap), anything wider streams
#define SEG_CE_REG_CAP 32
#define SEG_STREAM_PLANES 8    // planes whose loads a streaming loop issues before it uses the first
#define SEG_CONF_MAX_BINS 192  // (192 + 1) * 192 32-bit LDS counters = 148 224 bytes of the CU's 160 KB
#define SEG_CONF_WGS 2048      // confusion workgroups per launch: each zeroes and flushes one LDS matrix, so it strides over many chunks
#define SEG_MAX_P (1 << 30)    // pixel indices (chunk base + 3 * SEG_THREADS) stay in int
#define SEG_ALIGNED16(p) (((uintptr_t)(p) % 16) == 0)

struct alignas(16) seg_i64x2 {
    long long a, b;
};

// first pixel of this lane in chunk `chunk`; its others are i0 + 1, 2, 3 (VEC) or i0 + SEG_THREADS * k
template <bool VEC>
__device__ __forceinline__ int seg_first(int chunk) {
    return chunk * SEG_CHUNK + (VEC ? SEG_PIX * (int)threadIdx.x : (int)threadIdx.x);
}
template <bool VEC>
__device__ __forceinline__ void seg_ld(const float* plane, int i0, int P, float (&v)[SEG_PIX]) {
    if (VEC) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 < P) t = sgx_ld4(plane + i0);  // (P % 4 == 0: a quad is inside the plane or wholly past it)
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) {
            const int i = i0 + k * SEG_THREADS;
            v[k] = i < P ? plane[i] : 0.f;
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void seg_st(float* plane, int i0, int P, const float (&v)[SEG_PIX]) {
    if (VEC) {
        if (i0 < P) sgx_st4(plane + i0, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) {
            const int i = i0 + k * SEG_THREADS;
            if (i < P) plane[i] = v[k];
        }
    }
}
// the lane's four labels; live[k] = the pixel exists
template <bool VEC>
__device__ __forceinline__ void seg_ld_labels(const int64_t* lab, int i0, int P, long long (&y)[SEG_PIX], bool (&live)[SEG_PIX]) {
    if (VEC) {
        const bool in = i0 < P;
        seg_i64x2 lo = {0, 0}, hi = {0, 0};
        if (in) {
            lo = *reinterpret_cast<const seg_i64x2*>(lab + i0);
            hi = *reinterpret_cast<const seg_i64x2*>(lab + i0 + 2);
        }
        y[0] = lo.a; y[1] = lo.b; y[2] = hi.a; y[3] = hi.b;
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) live[k] = in;
    } else {
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) {
            const int i = i0 + k * SEG_THREADS;
            live[k] = i < P;
            y[k] = live[k] ? (long long)lab[i] : 0;
        }
    }
}
// class of each pixel, or -1 for "contributes nothing": dead, label == ignore_index, or a label outside [0, C) (a caller error the 2-D
// kernel treats as ignored too)
template <bool VEC>
__device__ __forceinline__ void seg_ce_classes(const int64_t* lab, int i0, int P, int C, int ignore_index, const float* weight, int (&cls)[SEG_PIX],
                                               float (&wy)[SEG_PIX]) {
    long long y[SEG_PIX];
    bool live[SEG_PIX];
    seg_ld_labels<VEC>(lab, i0, P, y, live);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        const bool use = live[k] && y[k] != (long long)ignore_index && y[k] >= 0 && y[k] < (long long)C;
        cls[k] = use ? (int)y[k] : -1;
        wy[k] = use ? (weight ? weight[cls[k]] : 1.f) : 0.f;
    }
}
// the workgroup's (numerator, denominator): xor butterflies inside each wave, then the four wave sums added in wave order by thread 0 -
// the same order in every run.  All threads call.
__device__ __forceinline__ void seg_block_sum2(float a, float b, float* out_a, float* out_b) {
    __shared__ float red[2][SEG_THREADS / 64];
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sa = red[0][0], sb = red[1][0];
        for (int w = 1; w < SEG_THREADS / 64; ++w) {
            sa += red[0][w];
            sb += red[1][w];
        }
        *out_a = sa;
        *out_b = sb;
    }
}

// ---------------------------------------------------------------------------------------------
// seg_ce, register-resident form (C <= SEG_CE_REG_CAP): the lane's C x 4 logits are loaded once - every load is issued before the first
// use - and max, exp-sum, log-sum-exp, the loss term and the C gradients all come from those registers.  The map is read once and the
// gradient written once.  The class loops are fully unrolled against the cap and guarded by the (wave-uniform) C, so x[][] is indexed by
// constants only and never touches scratch.
//   pixel loss  = w[y] * (lse - x[y]),  denominator term = w[y],  d numerator / d x[c] = w[y] * (softmax_c - [c == y])
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_reg_kernel(int C, int P, const float* logits, const int64_t* labels, const float* weight, int ignore_index,
                                                                 float* part_loss, float* part_den, float* dlogits) {
    const int n = blockIdx.y, i0 = seg_first<VEC>((int)blockIdx.x);
    const float* xin = logits + (long)n * C * P;
    float* gout = dlogits + (long)n * C * P;
    float x[SEG_CE_REG_CAP][SEG_PIX];
#pragma unroll
    for (int c = 0; c < SEG_CE_REG_CAP; ++c)
        if (c < C) seg_ld<VEC>(xin + (long)c * P, i0, P, x[c]);
    int cls[SEG_PIX];
    float wy[SEG_PIX], m[SEG_PIX], s[SEG_PIX], xy[SEG_PIX];
    seg_ce_classes<VEC>(labels + (long)n * P, i0, P, C, ignore_index, weight, cls, wy);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        m[k] = x[0][k];
        s[k] = 0.f;
        xy[k] = 0.f;
    }
#pragma unroll
    for (int c = 1; c < SEG_CE_REG_CAP; ++c)
        if (c < C)
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) m[k] = fmaxf(m[k], x[c][k]);
#pragma unroll
    for (int c = 0; c < SEG_CE_REG_CAP; ++c)
        if (c < C)
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) {
                if (c == cls[k]) xy[k] = x[c][k];
                x[c][k] = expf(x[c][k] - m[k]);  // from here on x holds the exponentials
                s[k] += x[c][k];
            }
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        if (cls[k] >= 0) {
            num += wy[k] * ((logf(s[k]) + m[k]) - xy[k]);
            den += wy[k];
        }
        s[k] = 1.f / s[k];
    }
#pragma unroll
    for (int c = 0; c < SEG_CE_REG_CAP; ++c)
        if (c < C) {
            float g[SEG_PIX];
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) g[k] = cls[k] >= 0 ? wy[k] * (x[c][k] * s[k] - (c == cls[k] ? 1.f : 0.f)) : 0.f;  // ignored pixel: zero in every plane
            seg_st<VEC>(gout + (long)c * P, i0, P, g);
        }
    const int wg = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    seg_block_sum2(num, den, part_loss + wg, part_den + wg);
}

// ---------------------------------------------------------------------------------------------
// seg_ce, streaming form (any C): pass 1 keeps an online maximum and a rescaled exp-sum per pixel while the planes stream by
// (SEG_STREAM_PLANES loads in flight), pass 2 re-reads the planes and writes the gradient.  The map is read twice, the gradient written once.
// exp arguments are clamped at 0 from above: m - m' and x - m' are <= 0 by construction, and the clamp turns the (-inf) - (-inf) = nan of a
// pixel whose planes so far are all -inf into exp(0), which the first finite plane then rescales by exp(-inf) = 0.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_stream_kernel(int C, int P, const float* logits, const int64_t* labels, const float* weight, int ignore_index,
                                                                    float* part_loss, float* part_den, float* dlogits) {
    const int n = blockIdx.y, i0 = seg_first<VEC>((int)blockIdx.x);
    const float* xin = logits + (long)n * C * P;
    float* gout = dlogits + (long)n * C * P;
    int cls[SEG_PIX];
    float wy[SEG_PIX], m[SEG_PIX], s[SEG_PIX], xy[SEG_PIX];
    seg_ce_classes<VEC>(labels + (long)n * P, i0, P, C, ignore_index, weight, cls, wy);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        m[k] = -INFINITY;
        s[k] = 0.f;
        xy[k] = 0.f;
    }
    for (int c0 = 0; c0 < C; c0 += SEG_STREAM_PLANES) {
        float t[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
        for (int j = 0; j < SEG_STREAM_PLANES; ++j)
            if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, t[j]);
#pragma unroll
        for (int j = 0; j < SEG_STREAM_PLANES; ++j)
            if (c0 + j < C)
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k) {
                    const float mn = fmaxf(m[k], t[j][k]);
                    s[k] = s[k] * expf(fminf(m[k] - mn, 0.f)) + expf(fminf(t[j][k] - mn, 0.f));
                    m[k] = mn;
                    if (c0 + j == cls[k]) xy[k] = t[j][k];
                }
    }
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        if (cls[k] >= 0) {
            num += wy[k] * ((logf(s[k]) + m[k]) - xy[k]);
            den += wy[k];
        }
        s[k] = 1.f / s[k];
    }
    for (int c0 = 0; c0 < C; c0 += SEG_STREAM_PLANES) {
        float t[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
        for (int j = 0; j < SEG_STREAM_PLANES; ++j)
            if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, t[j]);
#pragma unroll
        for (int j = 0; j < SEG_STREAM_PLANES; ++j)
            if (c0 + j < C) {
                float g[SEG_PIX];
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k)
                    g[k] = cls[k] >= 0 ? wy[k] * (expf(t[j][k] - m[k]) * s[k] - (c0 + j == cls[k] ? 1.f : 0.f)) : 0.f;
                seg_st<VEC>(gout + (long)(c0 + j) * P, i0, P, g);
            }
    }
    const int wg = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    seg_block_sum2(num, den, part_loss + wg, part_den + wg);
}

static bool seg_vec_ok(int P, const void* a, const void* b, const void* c) { return P % 4 == 0 && SEG_ALIGNED16(a) && SEG_ALIGNED16(b) && SEG_ALIGNED16(c); }

// number of per-workgroup partial sums of a seg_ce launch: the caller's loss buffer holds 2 * that + 2 floats
extern "C" int32_t sgx_seg_ce_blocks(int32_t N, int32_t P) { return N > 0 && P > 0 ? N * sgx_cdiv(P, SEG_CHUNK) : 0; }

// loss: 2 * sgx_seg_ce_blocks + 2 floats; loss[0] = the loss, loss[1] = 1 / denominator; dlogits [N,C,P] WITHOUT the 1 / denominator factor
extern "C" int32_t sgx_seg_ce_fwd_bwd(int32_t N, int32_t C, int32_t P, const float* logits, const int64_t* labels, const float* weight, int32_t ignore_index,
                                      int32_t reduction_sum, float* loss, float* dlogits, void* stream) {
    SGX_CHECK_ARG(logits && labels && loss && dlogits && N > 0 && C > 0 && P > 0, "seg_ce: bad args");
    SGX_CHECK_ARG(N <= 65535 && P <= SEG_MAX_P, "seg_ce: at most 65535 images of 2^30 pixels (got %d x %d)", N, P);
    const int chunks = sgx_cdiv(P, SEG_CHUNK);
    SGX_CHECK_ARG((long)N * chunks <= 0x7fffffffL / 2, "seg_ce: too many workgroups");
    const int nwg = N * chunks;
    float *pl = loss + 2, *pd = loss + 2 + nwg;
    const bool vec = seg_vec_ok(P, logits, dlogits, labels);
    const bool in_regs = C <= SEG_CE_REG_CAP;  // THE predicate between the two forms
    const dim3 grid((unsigned)chunks, (unsigned)N), block(SEG_THREADS);
    if (in_regs && vec) SGX_LAUNCH(seg_ce_reg_kernel<true>, grid, block, 0, stream, C, P, logits, labels, weight, ignore_index, pl, pd, dlogits);
    else if (in_regs) SGX_LAUNCH(seg_ce_reg_kernel<false>, grid, block, 0, stream, C, P, logits, labels, weight, ignore_index, pl, pd, dlogits);
    else if (vec) SGX_LAUNCH(seg_ce_stream_kernel<true>, grid, block, 0, stream, C, P, logits, labels, weight, ignore_index, pl, pd, dlogits);
    else SGX_LAUNCH(seg_ce_stream_kernel<false>, grid, block, 0, stream, C, P, logits, labels, weight, ignore_index, pl, pd, dlogits);
    SGX_CHECK_LAUNCH("seg_ce");
    SGX_LAUNCH(ce_reduce_kernel, dim3(1), dim3(256), 0, stream, (const float*)pl, (const float*)pd, nwg, reduction_sum, loss);
    SGX_CHECK_LAUNCH("seg_ce reduce");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------
// seg_confusion: per-pixel arg-max over the planes (strict >: the lowest class wins a tie; NaN is not handled) + the label -> integer counts.
// counts[nb + 1][nb] int64, row = label (row nb: a label outside [0, nb) that is not ignored), column = prediction.  Each workgroup counts
// into a private 32-bit LDS matrix with integer LDS atomics - a lane first merges equal neighbours among its own 4 pixels, label maps being
// piecewise constant - and flushes the non-zero cells with 64-bit integer global atomics once, after striding over its share of the chunks
// of one image (at most P <= 2^30 pixels: a 32-bit cell cannot wrap).  Integer addition only: exact and independent of the order.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_confusion_kernel(int C, int P, int chunks, const float* logits, const int64_t* labels, int nb, int nig,
                                                                    long long ig0, long long ig1, long long ig2, long long ig3, unsigned long long* counts) {
    SGX_DYN_SMEM(unsigned, hist);
    const int cells = (nb + 1) * nb;
    for (int i = threadIdx.x; i < cells; i += SEG_THREADS) hist[i] = 0u;
    __syncthreads();
    const int n = blockIdx.y;
    const float* xin = logits + (long)n * C * P;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += (int)gridDim.x) {
        const int i0 = seg_first<VEC>(chunk);
        float best[SEG_PIX];
        int arg[SEG_PIX] = {0, 0, 0, 0};
        seg_ld<VEC>(xin, i0, P, best);
        for (int c0 = 1; c0 < C; c0 += SEG_STREAM_PLANES) {
            float t[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, t[j]);
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C)
#pragma unroll
                    for (int k = 0; k < SEG_PIX; ++k)
                        if (t[j][k] > best[k]) {
                            best[k] = t[j][k];
                            arg[k] = c0 + j;
                        }
        }
        long long y[SEG_PIX];
        bool live[SEG_PIX];
        seg_ld_labels<VEC>(labels + (long)n * P, i0, P, y, live);
        int run_cell = -1;
        unsigned run = 0u;
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) {
            const bool ignored = (nig > 0 && y[k] == ig0) || (nig > 1 && y[k] == ig1) || (nig > 2 && y[k] == ig2) || (nig > 3 && y[k] == ig3);
            if (!live[k] || ignored) continue;
            const int row = (y[k] >= 0 && y[k] < (long long)nb) ? (int)y[k] : nb;
            const int cell = row * nb + arg[k];
            if (cell != run_cell) {
                if (run) atomicAdd(&hist[run_cell], run);
                run_cell = cell;
                run = 0u;
            }
            ++run;
        }
        if (run) atomicAdd(&hist[run_cell], run);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += SEG_THREADS) {
        const unsigned v = hist[i];
        if (v) atomicAdd(counts + i, (unsigned long long)v);
    }
}

// dynamic LDS beyond 64 KB is opt-in per function and per device (pool.hip's scatter kernel does the same): one flag bit per device ordinal
template <bool VEC>
static bool seg_confusion_raise_lds() {
#ifndef SGX_EMU
    static std::atomic<unsigned long long> raised{0ull};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute((const void*)seg_confusion_kernel<VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (SEG_CONF_MAX_BINS + 1) * SEG_CONF_MAX_BINS * 4) !=
            hipSuccess)
            return false;
        raised.fetch_or(bit, std::memory_order_release);
    }
#endif
    return true;
}

// counts [num_bins + 1][num_bins] int64 ACCUMULATES (the caller zeroes it); num_bins in [C, SEG_CONF_MAX_BINS]; the first n_ignore of the four
// ignore values are labels whose pixels are skipped entirely
extern "C" int32_t sgx_seg_confusion(int32_t N, int32_t C, int32_t P, const float* logits, const int64_t* labels, int32_t num_bins, int32_t n_ignore, int64_t ignore0,
                                     int64_t ignore1, int64_t ignore2, int64_t ignore3, int64_t* counts, void* stream) {
    SGX_CHECK_ARG(logits && labels && counts && N > 0 && C > 0 && P > 0, "seg_confusion: bad args");
    SGX_CHECK_ARG(N <= 65535 && P <= SEG_MAX_P, "seg_confusion: at most 65535 images of 2^30 pixels (got %d x %d)", N, P);
    SGX_CHECK_ARG(num_bins >= C && num_bins <= SEG_CONF_MAX_BINS, "seg_confusion: num_bins %d must lie in [C = %d, %d] (the workgroup's LDS matrix)", num_bins, C,
                  SEG_CONF_MAX_BINS);
    SGX_CHECK_ARG(n_ignore >= 0 && n_ignore <= 4, "seg_confusion: at most 4 ignore labels, got %d", n_ignore);
    const int chunks = sgx_cdiv(P, SEG_CHUNK);
    const int per_image = SEG_CONF_WGS / N > 0 ? SEG_CONF_WGS / N : 1;
    const dim3 grid((unsigned)(chunks < per_image ? chunks : per_image), (unsigned)N), block(SEG_THREADS);
    const unsigned lds = (unsigned)((num_bins + 1) * num_bins * 4);
    const bool vec = seg_vec_ok(P, logits, labels, labels);
    if (lds > 65536u && !(vec ? seg_confusion_raise_lds<true>() : seg_confusion_raise_lds<false>()))
        SGX_FAIL(SGX_ERR_HIP, "seg_confusion: cannot raise the kernel's dynamic LDS limit");
    if (vec)
        SGX_LAUNCH(seg_confusion_kernel<true>, grid, block, lds, stream, C, P, chunks, logits, labels, num_bins, n_ignore, (long long)ignore0, (long long)ignore1,
                   (long long)ignore2, (long long)ignore3, (unsigned long long*)counts);
    else
        SGX_LAUNCH(seg_confusion_kernel<false>, grid, block, lds, stream, C, P, chunks, logits, labels, num_bins, n_ignore, (long long)ignore0, (long long)ignore1,
                   (long long)ignore2, (long long)ignore3, (unsigned long long*)counts);
    SGX_CHECK_LAUNCH("seg_confusion");
    return SGX_OK;
}
