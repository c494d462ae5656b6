// Region ("structure") losses over the class planes of an NCHW map: Dice, IoU, their generalized forms and BCE + Dice (the
// reference's AbstarctSegmentationStructureLoss.forward).  Included by loss.hip after seg_ohem.h: segloss.h's lane-along-pixel geometry
// (seg_first / seg_ld / seg_st / seg_ld_labels), its VEC / scalar split and its fixed-order sums.
//
//   p = act(x), act = softmax over C | sigmoid | identity;  v = the pixel is valid;  t = the one-hot (or dense) target
//   per (n, c):  I = sum v t p,  S = sum v p,  T = sum t,  D = S + T (Dice) or S + T - I (IoU)
//   per group g (a class over the batch, or an image over its classes):  loss_g = 1 - (k I_g w_g + smooth) / (D_g w_g + eps + smooth)
//
// A call is the MOMENT pass and the FINALIZE step in forward and the GRADIENT pass in backward:
//   moment    a workgroup owns ONE image and strides over its chunks.  A lane keeps its own running S_c and I_c for every class across all
//             of its chunks (2 C registers; the register form, softmax and C <= SEG_STRUCT_REG_CAP) and the workgroup reduces them ONCE, at
//             its end: xor butterflies inside a wave, the waves added in wave order.  Wider maps and the other activations stream the planes
//             (an online max / rescaled-sum sweep for softmax, then the sweep that forms p_c); there a wave folds each plane's quad sums by a
//             butterfly and lane 0 keeps the wave's running sums in LDS.  T is an integer: an LDS histogram, integer atomics, flushed exactly.
//             Each workgroup writes one row {S[C], I[C], T[C]} of partials.  No float atomic anywhere.
//   finalize  one workgroup: folds the rows in index order in fp64, forms the group sums, weights, losses, the reduced loss and a table of
//             {a, b} per (n, c) with  d result / d p = v (a t + b (1 - [IoU] t)).  Nothing is read back.
//   gradient  one chunk per workgroup: reloads the logits and the labels, recomputes p, reads the image's row of the table and the upstream
//             gradient from device memory, and writes dx once, already scaled.
// A dense target with sigmoid / identity makes every (n, c) plane independent: N * C one-class images (4 float sums per lane, one of them
// the BCE-with-logits term when that is fused in).
#pragma once

#define SEG_STRUCT_REG_CAP 21   // register form: 4 C logits + 2 C running sums per lane (126 value registers at the cap; VOC's 21 classes fit)
#define SEG_STRUCT_WGS 1536     // moment workgroups per launch (6 per CU: whole rounds at 1, 2, 3 or 6 resident workgroups per CU)
#define SEG_STRUCT_MAX_C 1024   // label form: 36 C bytes of LDS (histogram + 4 waves x 2 C sums)
#define SEG_STRUCT_ACT(flags) ((flags) & SGX_SEG_STRUCT_ACT_MASK)

// channel of each of the lane's pixels, or -1: dead, label == ignore_index, or a channel outside [0, C).  The reference builds C + 1 one-hot
// channels and deletes channel ignore_index: a label above it moves down by one.
template <bool VEC>
__device__ __forceinline__ void seg_struct_classes(const int64_t* lab, int i0, int P, int C, int has_ignore, int ignore_index, int (&cls)[SEG_PIX]) {
    long long y[SEG_PIX];
    bool live[SEG_PIX];
    seg_ld_labels<VEC>(lab, i0, P, y, live);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        const long long ch = y[k] - ((has_ignore && y[k] > (long long)ignore_index) ? 1 : 0);
        const bool use = live[k] && !(has_ignore && y[k] == (long long)ignore_index) && ch >= 0 && ch < (long long)C;
        cls[k] = use ? (int)ch : -1;
    }
}
// the lane's valid pixels into the workgroup's LDS histogram; equal neighbours merged first (label maps are piecewise constant)
__device__ __forceinline__ void seg_struct_count(unsigned* hist, const int (&cls)[SEG_PIX]) {
    int run_c = -1;
    unsigned run = 0u;
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        if (cls[k] < 0) continue;
        if (cls[k] != run_c) {
            if (run) atomicAdd(&hist[run_c], run);
            run_c = cls[k];
            run = 0u;
        }
        ++run;
    }
    if (run) atomicAdd(&hist[run_c], run);
}
__device__ __forceinline__ float seg_struct_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float seg_struct_wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// the workgroup's row: the 4 waves' sums added in wave order, then the counts.  red = [4][2 C] floats behind hist[C]
__device__ __forceinline__ void seg_struct_flush_row(const unsigned* hist, const float* red, int C, unsigned* row) {
    for (int j = threadIdx.x; j < 2 * C; j += SEG_THREADS) {
        float r = red[j];
        for (int w = 1; w < SEG_THREADS / 64; ++w) r += red[w * 2 * C + j];
        row[j] = __float_as_uint(r);
    }
    for (int c = threadIdx.x; c < C; c += SEG_THREADS) row[2 * C + c] = hist[c];
}

// ---------------------------------------------------------------------------------------------
// Moment pass, register form (softmax, C <= SEG_STRUCT_REG_CAP): a chunk's C x 4 logits are loaded once, every load issued before the first
// use.  The class loops are unrolled against the cap and guarded by the wave-uniform C: x, acc_s and acc_i are indexed by constants only.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_moment_reg_kernel(int C, int P, int chunks, const float* logits, const int64_t* labels, int has_ignore,
                                                                            int ignore_index, unsigned* part) {
    SGX_DYN_SMEM(unsigned, hist);
    float* red = reinterpret_cast<float*>(hist + C);
    for (int c = threadIdx.x; c < C; c += SEG_THREADS) hist[c] = 0u;
    __syncthreads();
    const int n = blockIdx.y;
    const float* xin = logits + (long)n * C * P;
    float acc_s[SEG_STRUCT_REG_CAP], acc_i[SEG_STRUCT_REG_CAP];
#pragma unroll
    for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c) acc_s[c] = acc_i[c] = 0.f;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += (int)gridDim.x) {
        const int i0 = seg_first<VEC>(chunk);
        float x[SEG_STRUCT_REG_CAP][SEG_PIX];
#pragma unroll
        for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
            if (c < C) seg_ld<VEC>(xin + (long)c * P, i0, P, x[c]);
        int cls[SEG_PIX];
        seg_struct_classes<VEC>(labels + (long)n * P, i0, P, C, has_ignore, ignore_index, cls);
        float m[SEG_PIX], s[SEG_PIX];
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) {
            m[k] = x[0][k];
            s[k] = 0.f;
        }
        int c_max = C, c_exp = C, c_acc = C;
        SEG_OHEM_OPAQUE(c_max);
        SEG_OHEM_OPAQUE(c_exp);
        SEG_OHEM_OPAQUE(c_acc);
#pragma unroll
        for (int c = 1; c < SEG_STRUCT_REG_CAP; ++c)
            if (c < c_max)
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k) m[k] = fmaxf(m[k], x[c][k]);
#pragma unroll
        for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
            if (c < c_exp)
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k) {
                    x[c][k] = expf(x[c][k] - m[k]);
                    s[k] += x[c][k];
                }
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) s[k] = cls[k] >= 0 ? 1.f / s[k] : 0.f;  // an invalid pixel adds nothing to either sum
#pragma unroll
        for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
            if (c < c_acc)
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k) {
                    const float p = x[c][k] * s[k];
                    acc_s[c] += p;
                    if (c == cls[k]) acc_i[c] += p;
                }
        seg_struct_count(hist, cls);
    }
    int c_red = C;
    SEG_OHEM_OPAQUE(c_red);
#pragma unroll
    for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
        if (c < c_red) {
            const float a = seg_struct_wave_sum(acc_s[c]), b = seg_struct_wave_sum(acc_i[c]);
            if ((threadIdx.x & 63) == 0) {
                red[(threadIdx.x >> 6) * 2 * C + c] = a;
                red[(threadIdx.x >> 6) * 2 * C + C + c] = b;
            }
        }
    __syncthreads();
    seg_struct_flush_row(hist, red, C, part + (long)(blockIdx.y * gridDim.x + blockIdx.x) * 3 * C);
}

// ---------------------------------------------------------------------------------------------
// Moment pass, streaming form (any C <= SEG_STRUCT_MAX_C, any activation).  Softmax: seg_ohem_stream_stats' online sweep, then the sweep that
// forms p_c (the map is read twice); sigmoid and identity need the second sweep alone.  A plane's quad sums are folded across the wave at
// once and lane 0 adds them to the wave's running sums in LDS (a slot has one writer: no atomic, a fixed order).
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_moment_stream_kernel(int C, int P, int chunks, const float* logits, const int64_t* labels, int act,
                                                                               int has_ignore, int ignore_index, unsigned* part) {
    SGX_DYN_SMEM(unsigned, hist);
    float* red = reinterpret_cast<float*>(hist + C);
    for (int c = threadIdx.x; c < 9 * C; c += SEG_THREADS) hist[c] = 0u;  // (the counts and the 4 x 2 C running sums: 0.f is all-zero bits)
    __syncthreads();
    const int n = blockIdx.y;
    const float* xin = logits + (long)n * C * P;
    float* mine = red + (threadIdx.x >> 6) * 2 * C;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += (int)gridDim.x) {
        const int i0 = seg_first<VEC>(chunk);
        int cls[SEG_PIX];
        seg_struct_classes<VEC>(labels + (long)n * P, i0, P, C, has_ignore, ignore_index, cls);
        float m[SEG_PIX] = {0.f, 0.f, 0.f, 0.f}, s[SEG_PIX] = {1.f, 1.f, 1.f, 1.f}, xy[SEG_PIX];
        if (act == SGX_SEG_STRUCT_SOFTMAX) {
            seg_ohem_stream_stats<VEC>(xin, i0, P, C, cls, m, s, xy);
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) s[k] = 1.f / s[k];
        }
        for (int c0 = 0; c0 < C; c0 += SEG_STREAM_PLANES) {
            float t[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, t[j]);
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) {
                    float sv = 0.f, iv = 0.f;
#pragma unroll
                    for (int k = 0; k < SEG_PIX; ++k) {
                        float p = act == SGX_SEG_STRUCT_SOFTMAX ? expf(t[j][k] - m[k]) * s[k] : (act == SGX_SEG_STRUCT_SIGMOID ? seg_struct_sigmoid(t[j][k]) : t[j][k]);
                        p = cls[k] >= 0 ? p : 0.f;
                        sv += p;
                        if (c0 + j == cls[k]) iv += p;
                    }
                    sv = seg_struct_wave_sum(sv);
                    iv = seg_struct_wave_sum(iv);
                    if ((threadIdx.x & 63) == 0) {
                        mine[c0 + j] += sv;
                        mine[C + c0 + j] += iv;
                    }
                }
        }
        seg_struct_count(hist, cls);
    }
    __syncthreads();
    seg_struct_flush_row(hist, red, C, part + (long)(blockIdx.y * gridDim.x + blockIdx.x) * 3 * C);
}

// the lane's four target values of a dense plane, as floats
template <bool VEC, bool TI64>
__device__ __forceinline__ void seg_struct_ld_target(const void* plane, int i0, int P, float (&t)[SEG_PIX]) {
    if (TI64) {
        long long y[SEG_PIX];
        bool live[SEG_PIX];
        seg_ld_labels<VEC>(static_cast<const int64_t*>(plane), i0, P, y, live);
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) t[k] = (float)y[k];
    } else {
        seg_ld<VEC>(static_cast<const float*>(plane), i0, P, t);
    }
}
// ---------------------------------------------------------------------------------------------
// Moment pass of a dense target (sigmoid / identity): blockIdx.y is the (n, c) plane, a one-class image.  Per lane sum t, sum p, sum t p and,
// with the BCE term, sum of max(x, 0) - x t + log1p(exp(-|x|)); one reduction at the workgroup's end -> a row of 4 floats.
// ---------------------------------------------------------------------------------------------
template <bool VEC, bool TI64>
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_dense_moment_kernel(int P, int chunks, const float* x, const void* target, int act, int bce, float* part) {
    __shared__ float red[4][SEG_THREADS / 64];
    const long plane = blockIdx.y;
    const float* xin = x + plane * P;
    const void* tin = TI64 ? (const void*)(static_cast<const int64_t*>(target) + plane * P) : (const void*)(static_cast<const float*>(target) + plane * P);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int chunk = blockIdx.x; chunk < chunks; chunk += (int)gridDim.x) {
        const int i0 = seg_first<VEC>(chunk);
        float xv[SEG_PIX], tv[SEG_PIX];
        seg_ld<VEC>(xin, i0, P, xv);
        seg_struct_ld_target<VEC, TI64>(tin, i0, P, tv);
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k)
            if (seg_ohem_live<VEC>(i0, P, k)) {
                const float p = act == SGX_SEG_STRUCT_SIGMOID ? seg_struct_sigmoid(xv[k]) : xv[k];
                acc[0] += tv[k];
                acc[1] += p;
                acc[2] += tv[k] * p;
                if (bce) acc[3] += (fmaxf(xv[k], 0.f) - xv[k] * tv[k]) + log1pf(expf(-fabsf(xv[k])));
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = seg_struct_wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float r = red[threadIdx.x][0];
        for (int w = 1; w < SEG_THREADS / 64; ++w) r += red[threadIdx.x][w];
        part[(long)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// Finalize (one workgroup).  mom [N C][4] = {I, D, T, BCE sum} and grp [G][3] = {weighted loss_g, a_g, b_g} are fp64 scratch in the workspace.
//   w_g = 1 / T_g^2 (inf -> 0) when generalized, else 1;  num = k I_g w_g + smooth;  den = D_g w_g + eps + smooth;  loss_g = 1 - num / den
//   r_g = d result / d loss_g = class weight x (1 / G for "mean") x w_dice;   a_g = -k w_g r_g / den;   b_g = num w_g r_g / den^2
// coef [2 N C + 1]: {a, b} of every (n, c) - expanded, the gradient pass does not know which axis was grouped - then w_bce / (N C P).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_final_kernel(int N, int C, int P, int rows, int flags, double smooth, double eps, double w_bce, double w_dice,
                                                                       const float* weight, const unsigned* part, double* mom, double* grp, float* loss, float* coef) {
    const bool dense = (flags & (SGX_SEG_STRUCT_DENSE_F32 | SGX_SEG_STRUCT_DENSE_I64)) != 0, iou = (flags & SGX_SEG_STRUCT_IOU) != 0;
    const bool over_n = (flags & SGX_SEG_STRUCT_OVER_BATCHES) != 0;
    const int NC = N * C, G = over_n ? N : C, M = over_n ? C : N;
    for (int e = threadIdx.x; e < NC; e += SEG_THREADS) {
        double I = 0.0, S = 0.0, T = 0.0, B = 0.0;
        if (dense) {
            const float* row = reinterpret_cast<const float*>(part) + (long)e * rows * 4;
            for (int j = 0; j < rows; ++j, row += 4) {
                T += (double)row[0];
                S += (double)row[1];
                I += (double)row[2];
                B += (double)row[3];
            }
        } else {
            const int n = e / C, c = e % C;
            const unsigned* row = part + (long)n * rows * 3 * C;
            unsigned long long cnt = 0ull;
            for (int j = 0; j < rows; ++j, row += 3 * C) {
                S += (double)__uint_as_float(row[c]);
                I += (double)__uint_as_float(row[C + c]);
                cnt += row[2 * C + c];
            }
            T = (double)cnt;
        }
        mom[4 * e] = I;
        mom[4 * e + 1] = iou ? (S + T) - I : S + T;
        mom[4 * e + 2] = T;
        mom[4 * e + 3] = B;
    }
    __syncthreads();
    const double k = iou ? 1.0 : 2.0;
    for (int g = threadIdx.x; g < G; g += SEG_THREADS) {
        double I = 0.0, D = 0.0, T = 0.0;
        for (int j = 0; j < M; ++j) {
            const int e = over_n ? g * C + j : j * C + g;
            I += mom[4 * e];
            D += mom[4 * e + 1];
            T += mom[4 * e + 2];
        }
        const double w = (flags & SGX_SEG_STRUCT_GENERALIZED) ? (T * T > 0.0 ? 1.0 / (T * T) : 0.0) : 1.0;
        const double num = k * I * w + smooth, den = D * w + eps + smooth;
        const double cw = weight ? (double)weight[g] : 1.0;
        const double r = cw * ((flags & (SGX_SEG_STRUCT_SUM | SGX_SEG_STRUCT_NONE)) ? 1.0 : 1.0 / (double)G) * w_dice;
        grp[3 * g] = cw * (1.0 - num / den);
        grp[3 * g + 1] = -k * w * r / den;
        grp[3 * g + 2] = num * w * r / (den * den);
        if (flags & SGX_SEG_STRUCT_NONE) loss[g] = (float)(w_dice * grp[3 * g]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NC; e += SEG_THREADS) {
        const int g = over_n ? e / C : e % C;
        coef[2 * e] = (float)grp[3 * g + 1];
        coef[2 * e + 1] = (float)grp[3 * g + 2];
    }
    if (threadIdx.x == 0) {
        const double npix = (double)NC * (double)P;
        coef[2 * NC] = (float)(w_bce / npix);
        if (!(flags & SGX_SEG_STRUCT_NONE)) {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += grp[3 * g];
            double out = w_dice * ((flags & SGX_SEG_STRUCT_SUM) ? s : s / (double)G);
            if (flags & SGX_SEG_STRUCT_BCE) {
                double b = 0.0;
                for (int e = 0; e < NC; ++e) b += mom[4 * e + 3];
                out += w_bce * (b / npix);
            }
            loss[0] = (float)out;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Gradient pass over labels.  With q_c = b_c + [c == y] e_c, e = a - [IoU] b, both already times the upstream gradient of the (n, c) group:
//   softmax : dx_c = p_c (q_c - sum_j p_j q_j)      sigmoid : dx_c = q_c p_c (1 - p_c)      identity : dx_c = q_c
// and zero in every plane of an invalid pixel.  The image's coefficients are wave-uniform loads.  up = grad_out[n * gs_n + c * gs_c].
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void seg_struct_coef(const float* coef, const float* up, int n, int c, int C, int iou, int gs_n, int gs_c, float& b, float& e) {
    const float g = up[n * gs_n + c * gs_c], a = coef[2 * (n * C + c)] * g;
    b = coef[2 * (n * C + c) + 1] * g;
    e = iou ? a - b : a;
}
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_grad_reg_kernel(int C, int P, const float* logits, const int64_t* labels, int has_ignore, int ignore_index,
                                                                          int iou, const float* coef, const float* up, int gs_n, int gs_c, float* dx) {
    const int n = blockIdx.y, i0 = seg_first<VEC>((int)blockIdx.x);
    const float* xin = logits + (long)n * C * P;
    float* gout = dx + (long)n * C * P;
    float x[SEG_STRUCT_REG_CAP][SEG_PIX];
#pragma unroll
    for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
        if (c < C) seg_ld<VEC>(xin + (long)c * P, i0, P, x[c]);
    int cls[SEG_PIX];
    seg_struct_classes<VEC>(labels + (long)n * P, i0, P, C, has_ignore, ignore_index, cls);
    float m[SEG_PIX], s[SEG_PIX], dot[SEG_PIX];
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        m[k] = x[0][k];
        s[k] = 0.f;
        dot[k] = 0.f;
    }
    int c_max = C, c_exp = C, c_dot = C, c_out = C;
    SEG_OHEM_OPAQUE(c_max);
    SEG_OHEM_OPAQUE(c_exp);
    SEG_OHEM_OPAQUE(c_dot);
    SEG_OHEM_OPAQUE(c_out);
#pragma unroll
    for (int c = 1; c < SEG_STRUCT_REG_CAP; ++c)
        if (c < c_max)
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) m[k] = fmaxf(m[k], x[c][k]);
#pragma unroll
    for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
        if (c < c_exp)
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) {
                x[c][k] = expf(x[c][k] - m[k]);
                s[k] += x[c][k];
            }
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) s[k] = 1.f / s[k];
#pragma unroll
    for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
        if (c < c_dot) {
            float b, e;
            seg_struct_coef(coef, up, n, c, C, iou, gs_n, gs_c, b, e);
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) {
                x[c][k] *= s[k];  // from here on x holds the probabilities
                dot[k] += x[c][k] * (c == cls[k] ? b + e : b);
            }
        }
#pragma unroll
    for (int c = 0; c < SEG_STRUCT_REG_CAP; ++c)
        if (c < c_out) {
            float b, e, g[SEG_PIX];
            seg_struct_coef(coef, up, n, c, C, iou, gs_n, gs_c, b, e);
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) g[k] = cls[k] >= 0 ? x[c][k] * ((c == cls[k] ? b + e : b) - dot[k]) : 0.f;
            seg_st<VEC>(gout + (long)c * P, i0, P, g);
        }
}
template <bool VEC>
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_grad_stream_kernel(int C, int P, const float* logits, const int64_t* labels, int act, int has_ignore,
                                                                             int ignore_index, int iou, const float* coef, const float* up, int gs_n, int gs_c,
                                                                             float* dx) {
    const int n = blockIdx.y, i0 = seg_first<VEC>((int)blockIdx.x);
    const float* xin = logits + (long)n * C * P;
    float* gout = dx + (long)n * C * P;
    int cls[SEG_PIX];
    seg_struct_classes<VEC>(labels + (long)n * P, i0, P, C, has_ignore, ignore_index, cls);
    float m[SEG_PIX], s[SEG_PIX], dot[SEG_PIX];
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        m[k] = -INFINITY;
        s[k] = 0.f;
        dot[k] = 0.f;
    }
    if (act == SGX_SEG_STRUCT_SOFTMAX) {
        // sum_j p_j q_j = (sum_j e^(x_j - m) q_j) / s: the numerator is rescaled with s while the planes stream by
        for (int c0 = 0; c0 < C; c0 += SEG_STREAM_PLANES) {
            float t[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, t[j]);
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) {
                    float b, e;
                    seg_struct_coef(coef, up, n, c0 + j, C, iou, gs_n, gs_c, b, e);
#pragma unroll
                    for (int k = 0; k < SEG_PIX; ++k) {
                        const float mn = fmaxf(m[k], t[j][k]);
                        const float r = expf(fminf(m[k] - mn, 0.f)), ex = expf(fminf(t[j][k] - mn, 0.f));
                        s[k] = s[k] * r + ex;
                        dot[k] = dot[k] * r + ex * (c0 + j == cls[k] ? b + e : b);
                        m[k] = mn;
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) {
            s[k] = 1.f / s[k];
            dot[k] *= s[k];
        }
    }
    for (int c0 = 0; c0 < C; c0 += SEG_STREAM_PLANES) {
        float t[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
        for (int j = 0; j < SEG_STREAM_PLANES; ++j)
            if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, t[j]);
#pragma unroll
        for (int j = 0; j < SEG_STREAM_PLANES; ++j)
            if (c0 + j < C) {
                float b, e, g[SEG_PIX];
                seg_struct_coef(coef, up, n, c0 + j, C, iou, gs_n, gs_c, b, e);
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k) {
                    const float q = c0 + j == cls[k] ? b + e : b;
                    float d;
                    if (act == SGX_SEG_STRUCT_SOFTMAX) {
                        d = (expf(t[j][k] - m[k]) * s[k]) * (q - dot[k]);
                    } else if (act == SGX_SEG_STRUCT_SIGMOID) {
                        const float p = seg_struct_sigmoid(t[j][k]);
                        d = q * (p * (1.f - p));
                    } else {
                        d = q;
                    }
                    g[k] = cls[k] >= 0 ? d : 0.f;
                }
                seg_st<VEC>(gout + (long)(c0 + j) * P, i0, P, g);
            }
    }
}
// Gradient pass of a dense target: dx = (a t + b (1 - [IoU] t)) act'(x) + c_bce (sigmoid(x) - t), everything times the upstream gradient
template <bool VEC, bool TI64>
__global__ __launch_bounds__(SEG_THREADS) void seg_struct_dense_grad_kernel(int C, int P, const float* x, const void* target, int act, int iou, int bce,
                                                                            const float* coef, const float* c_bce, const float* up, int gs_n, int gs_c, float* dx) {
    const long plane = blockIdx.y;
    const int n = (int)(plane / C), c = (int)(plane % C), i0 = seg_first<VEC>((int)blockIdx.x);
    const float g = up[n * gs_n + c * gs_c], a = coef[2 * plane] * g, b = coef[2 * plane + 1] * g;
    const float cb = bce ? c_bce[0] * up[0] : 0.f;
    const void* tin = TI64 ? (const void*)(static_cast<const int64_t*>(target) + plane * P) : (const void*)(static_cast<const float*>(target) + plane * P);
    float xv[SEG_PIX], tv[SEG_PIX], d[SEG_PIX];
    seg_ld<VEC>(x + plane * P, i0, P, xv);
    seg_struct_ld_target<VEC, TI64>(tin, i0, P, tv);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        const float q = a * tv[k] + b * (iou ? 1.f - tv[k] : 1.f);
        const float sg = (bce || act == SGX_SEG_STRUCT_SIGMOID) ? seg_struct_sigmoid(xv[k]) : 0.f;
        d[k] = act == SGX_SEG_STRUCT_SIGMOID ? q * (sg * (1.f - sg)) : q;
        if (bce) d[k] += cb * (sg - tv[k]);
    }
    seg_st<VEC>(dx + plane * P, i0, P, d);
}

struct seg_struct_ws {
    int rows;  // partial rows per image (labels) or per (n, c) plane (dense): the moment grid's x extent
    long mom, grp, total;
};
static bool seg_struct_dense(int flags) { return (flags & (SGX_SEG_STRUCT_DENSE_F32 | SGX_SEG_STRUCT_DENSE_I64)) != 0; }
// the cap and the grid are functions of the shape alone
static seg_struct_ws seg_struct_layout(int N, int C, int P, int flags) {
    const long images = seg_struct_dense(flags) ? (long)N * C : N;
    const int chunks = sgx_cdiv(P, SEG_CHUNK), cap = SEG_STRUCT_WGS / images > 0 ? (int)(SEG_STRUCT_WGS / images) : 1;
    seg_struct_ws w;
    w.rows = chunks < cap ? chunks : cap;
    const long part = seg_struct_dense(flags) ? images * w.rows * 16 : images * w.rows * 12L * C;
    w.mom = (part + 15) / 16 * 16;
    w.grp = w.mom + 32L * N * C;
    w.total = w.grp + 24L * (N > C ? N : C);
    return w;
}
static bool seg_struct_flags_ok(int flags) {
    const int act = SEG_STRUCT_ACT(flags);
    if (act > SGX_SEG_STRUCT_IDENTITY) return false;
    if ((flags & SGX_SEG_STRUCT_DENSE_F32) && (flags & SGX_SEG_STRUCT_DENSE_I64)) return false;
    if ((flags & SGX_SEG_STRUCT_SUM) && (flags & SGX_SEG_STRUCT_NONE)) return false;
    if (seg_struct_dense(flags)) return act != SGX_SEG_STRUCT_SOFTMAX && !(flags & SGX_SEG_STRUCT_HAS_IGNORE);
    return !(flags & SGX_SEG_STRUCT_BCE);
}
#define SEG_STRUCT_CHECK_SHAPE(what)                                                                                                             \
    SGX_CHECK_ARG(N > 0 && C > 0 && P > 0 && seg_struct_flags_ok(flags), what ": bad shape or flags (%d x %d x %d, flags 0x%x)", N, C, P, flags); \
    SGX_CHECK_ARG(N <= 65535 && P <= SEG_MAX_P, what ": at most 65535 images of 2^30 pixels (got %d x %d)", N, P);                               \
    SGX_CHECK_ARG(seg_struct_dense(flags) ? (long)N * C <= 65535 : C <= SEG_STRUCT_MAX_C,                                                        \
                  what ": at most %d classes with labels, at most 65535 planes with a dense target (got %d x %d)", SEG_STRUCT_MAX_C, N, C)

extern "C" int64_t sgx_seg_struct_ws_bytes(int32_t N, int32_t C, int32_t P, int32_t flags) {
    return N > 0 && C > 0 && P > 0 ? seg_struct_layout(N, C, P, flags).total : 0;
}

#define SEG_STRUCT_LAUNCH2(kernel, a, b, grid, lds, ...)                                             \
    do {                                                                                             \
        if ((a) && (b)) SGX_LAUNCH((kernel<true, true>), grid, block, lds, stream, __VA_ARGS__);     \
        else if (a) SGX_LAUNCH((kernel<true, false>), grid, block, lds, stream, __VA_ARGS__);        \
        else if (b) SGX_LAUNCH((kernel<false, true>), grid, block, lds, stream, __VA_ARGS__);        \
        else SGX_LAUNCH((kernel<false, false>), grid, block, lds, stream, __VA_ARGS__);              \
    } while (0)
#define SEG_STRUCT_LAUNCH1(kernel, a, grid, lds, ...)                                    \
    do {                                                                                 \
        if (a) SGX_LAUNCH((kernel<true>), grid, block, lds, stream, __VA_ARGS__);        \
        else SGX_LAUNCH((kernel<false>), grid, block, lds, stream, __VA_ARGS__);         \
    } while (0)

// loss: one float, or G floats with SGX_SEG_STRUCT_NONE; coef: 2 N C + 1 floats for the backward call; ws: sgx_seg_struct_ws_bytes, 16-byte aligned
extern "C" int32_t sgx_seg_struct_fwd(int32_t N, int32_t C, int32_t P, const float* x, const void* target, int32_t flags, int32_t ignore_index, double smooth,
                                      double eps, double w_bce, double w_dice, const float* weight, void* ws, int64_t ws_bytes, float* loss, float* coef,
                                      void* stream) {
    SGX_CHECK_ARG(x && target && ws && loss && coef, "seg_struct_fwd: bad args");
    SEG_STRUCT_CHECK_SHAPE("seg_struct_fwd");
    SGX_CHECK_ARG(!(weight && (flags & (SGX_SEG_STRUCT_OVER_BATCHES | SGX_SEG_STRUCT_GENERALIZED))), "seg_struct_fwd: class weights need classes as groups");
    SGX_CHECK_ARG(!(flags & SGX_SEG_STRUCT_BCE) || !(flags & (SGX_SEG_STRUCT_SUM | SGX_SEG_STRUCT_NONE)), "seg_struct_fwd: the BCE term goes with the mean reduction");
    const seg_struct_ws o = seg_struct_layout(N, C, P, flags);
    SGX_CHECK_ARG(ws_bytes >= o.total && SEG_ALIGNED16(ws), "seg_struct_fwd: workspace of %ld bytes, 16-byte aligned, needed (got %ld)", o.total, (long)ws_bytes);
    char* base = (char*)ws;
    const int chunks = sgx_cdiv(P, SEG_CHUNK), act = SEG_STRUCT_ACT(flags), has_ignore = (flags & SGX_SEG_STRUCT_HAS_IGNORE) != 0;
    const dim3 block(SEG_THREADS);
    if (seg_struct_dense(flags)) {
        const dim3 grid((unsigned)o.rows, (unsigned)(N * C));
        const bool vec = seg_vec_ok(P, x, target, target), ti64 = (flags & SGX_SEG_STRUCT_DENSE_I64) != 0;
        SEG_STRUCT_LAUNCH2(seg_struct_dense_moment_kernel, vec, ti64, grid, 0, P, chunks, x, target, act, (int)((flags & SGX_SEG_STRUCT_BCE) != 0), (float*)base);
    } else {
        const dim3 grid((unsigned)o.rows, (unsigned)N);
        const bool vec = seg_vec_ok(P, x, target, target);
        const unsigned lds = 36u * (unsigned)C;
        const int64_t* labels = (const int64_t*)target;
        if (act == SGX_SEG_STRUCT_SOFTMAX && C <= SEG_STRUCT_REG_CAP)  // THE predicate between the two forms
            SEG_STRUCT_LAUNCH1(seg_struct_moment_reg_kernel, vec, grid, lds, C, P, chunks, x, labels, has_ignore, ignore_index, (unsigned*)base);
        else
            SEG_STRUCT_LAUNCH1(seg_struct_moment_stream_kernel, vec, grid, lds, C, P, chunks, x, labels, act, has_ignore, ignore_index, (unsigned*)base);
    }
    SGX_CHECK_LAUNCH("seg_struct_fwd moment pass");
    SGX_LAUNCH(seg_struct_final_kernel, dim3(1), block, 0, stream, N, C, P, o.rows, flags, smooth, eps, w_bce, w_dice, weight, (const unsigned*)base,
               (double*)(base + o.mom), (double*)(base + o.grp), loss, coef);
    SGX_CHECK_LAUNCH("seg_struct_fwd finalize");
    return SGX_OK;
}

// grad_out: the upstream gradient on the device, one float or G floats with SGX_SEG_STRUCT_NONE; dx [N, C, P] = d result / d x, already scaled
extern "C" int32_t sgx_seg_struct_bwd(int32_t N, int32_t C, int32_t P, const float* x, const void* target, int32_t flags, int32_t ignore_index, const float* coef,
                                      const float* grad_out, float* dx, void* stream) {
    SGX_CHECK_ARG(x && target && coef && grad_out && dx, "seg_struct_bwd: bad args");
    SEG_STRUCT_CHECK_SHAPE("seg_struct_bwd");
    const int chunks = sgx_cdiv(P, SEG_CHUNK), act = SEG_STRUCT_ACT(flags), has_ignore = (flags & SGX_SEG_STRUCT_HAS_IGNORE) != 0;
    const int iou = (flags & SGX_SEG_STRUCT_IOU) != 0, none = (flags & SGX_SEG_STRUCT_NONE) != 0, over_n = (flags & SGX_SEG_STRUCT_OVER_BATCHES) != 0;
    const int gs_n = none && over_n ? 1 : 0, gs_c = none && !over_n ? 1 : 0;
    const dim3 block(SEG_THREADS);
    if (seg_struct_dense(flags)) {
        SGX_CHECK_ARG((long)N * C * chunks <= 0x7fffffffL, "seg_struct_bwd: too many workgroups");
        const dim3 grid((unsigned)chunks, (unsigned)(N * C));
        const bool vec = seg_vec_ok(P, x, target, dx), ti64 = (flags & SGX_SEG_STRUCT_DENSE_I64) != 0;
        SEG_STRUCT_LAUNCH2(seg_struct_dense_grad_kernel, vec, ti64, grid, 0, C, P, x, target, act, iou, (int)((flags & SGX_SEG_STRUCT_BCE) != 0), coef,
                           coef + 2L * N * C, grad_out, gs_n, gs_c, dx);
    } else {
        SGX_CHECK_ARG((long)N * chunks <= 0x7fffffffL, "seg_struct_bwd: too many workgroups");
        const dim3 grid((unsigned)chunks, (unsigned)N);
        const bool vec = seg_vec_ok(P, x, target, dx);
        const int64_t* labels = (const int64_t*)target;
        if (act == SGX_SEG_STRUCT_SOFTMAX && C <= SEG_STRUCT_REG_CAP)
            SEG_STRUCT_LAUNCH1(seg_struct_grad_reg_kernel, vec, grid, 0, C, P, x, labels, has_ignore, ignore_index, iou, coef, grad_out, gs_n, gs_c, dx);
        else
            SEG_STRUCT_LAUNCH1(seg_struct_grad_stream_kernel, vec, grid, 0, C, P, x, labels, act, has_ignore, ignore_index, iou, coef, grad_out, gs_n, gs_c, dx);
    }
    SGX_CHECK_LAUNCH("seg_struct_bwd");
    return SGX_OK;
}
