// Online hard example mining over the per-pixel cross-entropy of an NCHW logit map (OhemCELoss, DDRNetLoss, ShelfNetOHEMLoss).
// Included by loss.hip after segloss.h: same lane-along-pixel geometry (seg_first / seg_ld / seg_st / seg_ce_classes), same VEC / scalar split,
// same register / streaming split at SEG_CE_REG_CAP.
//
// The reference sorts the N * P pixel losses and reads loss[num_mining] back to the host.  Here nothing is sorted and nothing is read back:
//   l_i  = cross-entropy of pixel i (0 for an ignored pixel; -inf = "not in the set" when ignored pixels are excluded)
//   BAR    branch (more than num_mining losses above thresh = -log(threshold)): mean of the l > thresh
//   TOP-K  branch: mean of the num_mining largest, found by a RADIX SELECT of the rank num_mining - 1 over the order-preserving 32-bit key of
//          the float, digits of 11 + 11 + 10 bits from the top: one histogram per level, one scan of its bins from the top per level.
// The branch is taken on the device: every launch after the first select step reads the record and returns at once when it has nothing to do.
// Counting is integer (LDS atomics, flushed with 64-bit global atomics), every float reduction has a fixed order: results repeat bit for bit.
//   launches: zero -> pixel pass (l, partials, level-0 histogram) -> select 0 -> refine 1 -> select 1 -> refine 2 -> select 2 -> sum -> final -> gradient
#pragma once

#define SEG_OHEM_BINS 2048       // bins of a level's histogram (11 bits; the last level uses 1024 of them)
#define SEG_OHEM_WGS 1024        // workgroups of a pass that streams l alone (refine, sum): each strides over its share of the quads
#define SEG_OHEM_REC_BYTES 256   // the record's slot at the head of the workspace
// workspace: [record | 3 histograms (u64) | sum-pass partials (f64) | pixel-pass partials: set, gt (u32), sum (f32), nwg words each | l], l on a
// 16-byte boundary.  Everything before l sits at a fixed offset: the pixel pass takes the base alone (its scalar registers are short:
// the 32 plane guards of the register form live in them).
#define SEG_OHEM_OFF_HIST SEG_OHEM_REC_BYTES
#define SEG_OHEM_OFF_PART_L (SEG_OHEM_OFF_HIST + 3L * SEG_OHEM_BINS * 8)
#define SEG_OHEM_OFF_PART (SEG_OHEM_OFF_PART_L + SEG_OHEM_WGS * 8L)
#define SEG_OHEM_OFF_L(nwg) ((SEG_OHEM_OFF_PART + 12L * (nwg) + 15) / 16 * 16)
enum { SEG_OHEM_NONE = 0, SEG_OHEM_BAR = 1, SEG_OHEM_TOPK = 2, SEG_OHEM_NAN = 3 };

struct seg_ohem_rec {
    unsigned long long num_pixels, num_mining, cnt_gt;  // the set's size, int(mining_percent * num_pixels) capped at num_pixels - 1, #{l > thresh}
    unsigned long long rank, c_gt, c_eq;                // TOP-K: rank left inside the prefix bin; #{key > the bin}; after the last level #{l == t}
    double sum_thresh;                                  // sum of the l > thresh
    unsigned prefix;                                    // key bits decided so far
    int branch;
    float t_eff, w_gt, w_eq;                            // the gradient pass's weights: w_gt on l > t_eff, w_eq on l == t_eff
};
static_assert(sizeof(seg_ohem_rec) <= SEG_OHEM_REC_BYTES, "the record outgrew its slot");

// order-preserving image of a float: negatives flipped, the sign bit set on the others (lse - x_y can round to a tiny negative)
__device__ __forceinline__ unsigned seg_ohem_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float seg_ohem_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// digit of level `level` and the bits above it
__device__ __forceinline__ unsigned seg_ohem_digit(unsigned key, int level) { return level == 0 ? key >> 21 : (level == 1 ? (key >> 10) & 2047u : key & 1023u); }
__device__ __forceinline__ bool seg_ohem_match(unsigned key, int level, unsigned prefix) {
    return level == 0 || (level == 1 ? key >> 21 : key >> 10) == prefix;
}
__device__ __forceinline__ void seg_ohem_count(unsigned* hist, float v, int level, unsigned prefix) {
    const unsigned key = seg_ohem_key(v);
    if (v != -INFINITY && seg_ohem_match(key, level, prefix)) atomicAdd(&hist[seg_ohem_digit(key, level)], 1u);
}
__device__ __forceinline__ void seg_ohem_hist_flush(const unsigned* hist, unsigned long long* out) {
    for (int i = threadIdx.x; i < SEG_OHEM_BINS; i += SEG_THREADS) {
        const unsigned v = hist[i];
        if (v) atomicAdd(out + i, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_zero_kernel(unsigned long long* p, int n) {
    for (int i = (int)(blockIdx.x * SEG_THREADS + threadIdx.x); i < n; i += (int)(gridDim.x * SEG_THREADS)) p[i] = 0ull;
}

// max and exp-sum of each of the lane's pixels and the logit of its class, planes streamed SEG_STREAM_PLANES at a time (seg_ce_stream_kernel's pass 1)
template <bool VEC>
__device__ __forceinline__ void seg_ohem_stream_stats(const float* xin, int i0, int P, int C, const int (&cls)[SEG_PIX], float (&m)[SEG_PIX], float (&s)[SEG_PIX],
                                                      float (&xy)[SEG_PIX]) {
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
}
// The class loops below are unrolled against the cap and guarded by the wave-uniform C.  Left alone, the compiler keeps the 32 guards of the
// load loop as 64-bit lane masks for the loops after it - 64 scalar registers, which with the pixel pass's other scalars spills.  A copy of C
// it cannot see through makes each later loop compare again where it needs the guard.
#ifdef SGX_EMU
#define SEG_OHEM_OPAQUE(c) ((void)0)
#else
#define SEG_OHEM_OPAQUE(c) asm volatile("" : "+s"(c))
#endif
// the same from registers (C <= SEG_CE_REG_CAP): every load issued before the first use; x holds the exponentials afterwards
template <bool VEC>
__device__ __forceinline__ void seg_ohem_reg_stats(const float* xin, int i0, int P, int C, const int (&cls)[SEG_PIX], float (&x)[SEG_CE_REG_CAP][SEG_PIX],
                                                   float (&m)[SEG_PIX], float (&s)[SEG_PIX], float (&xy)[SEG_PIX]) {
#pragma unroll
    for (int c = 0; c < SEG_CE_REG_CAP; ++c)
        if (c < C) seg_ld<VEC>(xin + (long)c * P, i0, P, x[c]);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        m[k] = x[0][k];
        s[k] = 0.f;
        xy[k] = 0.f;
    }
    int c_max = C, c_exp = C;
    SEG_OHEM_OPAQUE(c_max);
    SEG_OHEM_OPAQUE(c_exp);
#pragma unroll
    for (int c = 1; c < SEG_CE_REG_CAP; ++c)
        if (c < c_max)
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) m[k] = fmaxf(m[k], x[c][k]);
#pragma unroll
    for (int c = 0; c < SEG_CE_REG_CAP; ++c)
        if (c < c_exp)
#pragma unroll
            for (int k = 0; k < SEG_PIX; ++k) {
                if (c == cls[k]) xy[k] = x[c][k];
                x[c][k] = expf(x[c][k] - m[k]);
                s[k] += x[c][k];
            }
}
template <bool VEC>
__device__ __forceinline__ bool seg_ohem_live(int i0, int P, int k) {
    return (VEC ? i0 : i0 + k * SEG_THREADS) < P;
}

// ---------------------------------------------------------------------------------------------
// Pixel pass: the planes once -> l[N * P], the workgroup's (set size, #{l > thresh}, sum of the l > thresh) and the level-0 histogram.
// The float partial: xor butterflies inside each wave, then the wave sums in wave order (seg_block_sum2's order); the counts are integers.
// ---------------------------------------------------------------------------------------------
template <bool VEC, bool REG>
__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_pixel_kernel(int C, int P, const float* logits, const int64_t* labels, int ignore_index, int exclude,
                                                                     float thresh, char* ws) {
    __shared__ unsigned hist[SEG_OHEM_BINS];
    __shared__ float red_s[SEG_THREADS / 64];
    __shared__ unsigned red_n[2][SEG_THREADS / 64];
    const int n = blockIdx.y, i0 = seg_first<VEC>((int)blockIdx.x);
    const float* xin = logits + (long)n * C * P;
    int cls[SEG_PIX];
    float wy[SEG_PIX], m[SEG_PIX], s[SEG_PIX], xy[SEG_PIX];
    seg_ce_classes<VEC>(labels + (long)n * P, i0, P, C, ignore_index, nullptr, cls, wy);
    if (REG) {
        float x[SEG_CE_REG_CAP][SEG_PIX];
        seg_ohem_reg_stats<VEC>(xin, i0, P, C, cls, x, m, s, xy);
    } else {
        seg_ohem_stream_stats<VEC>(xin, i0, P, C, cls, m, s, xy);
    }
    for (int i = threadIdx.x; i < SEG_OHEM_BINS; i += SEG_THREADS) hist[i] = 0u;  // (after the planes: nothing of theirs is live across the barrier but m, s, xy)
    __syncthreads();
    float lv[SEG_PIX], sum = 0.f;
    unsigned nset = 0u, ngt = 0u;
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        // a label outside [0, C) that is not ignore_index (a caller error) counts as ignored, as in seg_ce
        lv[k] = cls[k] >= 0 ? (logf(s[k]) + m[k]) - xy[k] : (exclude ? -INFINITY : 0.f);
        if (seg_ohem_live<VEC>(i0, P, k) && (cls[k] >= 0 || !exclude)) {
            ++nset;
            if (lv[k] > thresh) {
                ++ngt;
                sum += lv[k];
            }
            seg_ohem_count(hist, lv[k], 0, 0u);
        }
    }
    const int nwg = (int)(gridDim.x * gridDim.y);
    seg_st<VEC>(reinterpret_cast<float*>(ws + SEG_OHEM_OFF_L(nwg)) + (long)n * P, i0, P, lv);
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        nset += __shfl_xor(nset, off);
        ngt += __shfl_xor(ngt, off);
    }
    if ((threadIdx.x & 63) == 0) {
        red_s[threadIdx.x >> 6] = sum;
        red_n[0][threadIdx.x >> 6] = nset;
        red_n[1][threadIdx.x >> 6] = ngt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float fs = red_s[0];
        unsigned a = red_n[0][0], b = red_n[1][0];
        for (int w = 1; w < SEG_THREADS / 64; ++w) {
            fs += red_s[w];
            a += red_n[0][w];
            b += red_n[1][w];
        }
        const int wg = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        unsigned* part = reinterpret_cast<unsigned*>(ws + SEG_OHEM_OFF_PART);
        part[wg] = a;
        part[nwg + wg] = b;
        part[2 * nwg + wg] = __float_as_uint(fs);
    }
    seg_ohem_hist_flush(hist, reinterpret_cast<unsigned long long*>(ws + SEG_OHEM_OFF_HIST));
}

// ---------------------------------------------------------------------------------------------
// Select step (one workgroup).  Level 0 first folds the pixel pass's partials in index order (fp64, strided then a fixed tree) and takes the
// branch.  In the TOP-K branch every level scans its histogram from the top bin down: a thread sums its run of adjacent bins, an inclusive
// scan over the 256 thread sums finds the one thread whose run holds the rank, and that thread walks its run.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_select_kernel(int level, seg_ohem_rec* rec, const unsigned long long* hist, const unsigned* part_set,
                                                                      const unsigned* part_gt, const float* part_sum, int nwg, float thresh, double mining_percent) {
    __shared__ unsigned long long sc[2][SEG_THREADS];
    __shared__ double sd[SEG_THREADS];
    __shared__ unsigned long long sh_rank;
    __shared__ int sh_branch;
    const int tid = threadIdx.x;
    if (level == 0) {
        unsigned long long a = 0ull, b = 0ull;
        double s = 0.0;
        for (int i = tid; i < nwg; i += SEG_THREADS) {
            a += part_set[i];
            b += part_gt[i];
            s += (double)part_sum[i];
        }
        sc[0][tid] = a;
        sc[1][tid] = b;
        sd[tid] = s;
        __syncthreads();
        for (int w = SEG_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                sc[0][tid] += sc[0][tid + w];
                sc[1][tid] += sc[1][tid + w];
                sd[tid] += sd[tid + w];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const unsigned long long np = sc[0][0], gt = sc[1][0];
            unsigned long long nm = (unsigned long long)(mining_percent * (double)np);  // int(mining_percent * num_pixels): truncation
            if (np && nm > np - 1) nm = np - 1;
            const int branch = np == 0 ? SEG_OHEM_NONE : (gt > nm ? SEG_OHEM_BAR : (nm == 0 ? SEG_OHEM_NAN : SEG_OHEM_TOPK));
            rec->num_pixels = np;
            rec->num_mining = nm;
            rec->cnt_gt = gt;
            rec->sum_thresh = sd[0];
            rec->branch = branch;
            sh_branch = branch;
            sh_rank = branch == SEG_OHEM_TOPK ? nm - 1 : 0ull;  // the num_mining-th largest has rank num_mining - 1 from the top
        }
        __syncthreads();
    }
    const int branch = level == 0 ? sh_branch : rec->branch;
    if (branch != SEG_OHEM_TOPK) return;
    const unsigned long long rank = level == 0 ? sh_rank : rec->rank;
    const int bins = level == 2 ? 1024 : SEG_OHEM_BINS, per = bins / SEG_THREADS, hi = bins - 1 - tid * per;
    const unsigned long long* h = hist + (long)level * SEG_OHEM_BINS;
    unsigned long long mine = 0ull;
    for (int j = 0; j < per; ++j) mine += h[hi - j];
    __syncthreads();  // (level 0: the fold's last reads of sc)
    sc[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < SEG_THREADS; off <<= 1) {  // inclusive scan, thread 0 = the top bins
        sc[cur ^ 1][tid] = sc[cur][tid] + (tid >= off ? sc[cur][tid - off] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long incl = sc[cur][tid];
    unsigned long long above = incl - mine;
    if (above <= rank && rank < incl) {
        for (int j = 0; j < per; ++j) {
            const unsigned long long c = h[hi - j];
            if (rank < above + c) {
                rec->prefix = ((level == 0 ? 0u : rec->prefix) << (level == 2 ? 10 : 11)) | (unsigned)(hi - j);
                rec->rank = rank - above;
                rec->c_gt = (level == 0 ? 0ull : rec->c_gt) + above;
                rec->c_eq = c;  // (the count of one key after the last level)
                break;
            }
            above += c;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Refine pass (levels 1 and 2): l alone, 16-byte loads, a bounded grid striding over the quads; histogram of the level's digit among the
// keys whose higher bits equal the prefix.  The few elements past the last whole quad go to workgroup 0.  (A workgroup's 32-bit LDS bin
// cannot wrap: its share of the at most 2^46 elements is under 2^32 for any map that fits a device.)  Level 0 is counted by the pixel pass:
// measured against a refine pass of its own, the fused form was 14 - 17 us faster per call at 16 x 19 x 1024 x 2048.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_refine_kernel(int level, const seg_ohem_rec* rec, const float* l, long n, unsigned long long* hist_out) {
    if (rec->branch != SEG_OHEM_TOPK) return;
    __shared__ unsigned hist[SEG_OHEM_BINS];
    for (int i = threadIdx.x; i < SEG_OHEM_BINS; i += SEG_THREADS) hist[i] = 0u;
    __syncthreads();
    const unsigned prefix = rec->prefix;
    const long quads = n / 4;
    for (long q = (long)blockIdx.x * SEG_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * SEG_THREADS) {
        const float4 v = sgx_ld4(l + 4 * q);
        seg_ohem_count(hist, v.x, level, prefix);
        seg_ohem_count(hist, v.y, level, prefix);
        seg_ohem_count(hist, v.z, level, prefix);
        seg_ohem_count(hist, v.w, level, prefix);
    }
    if (blockIdx.x == 0 && 4 * quads + (long)threadIdx.x < n) seg_ohem_count(hist, l[4 * quads + threadIdx.x], level, prefix);
    __syncthreads();
    seg_ohem_hist_flush(hist, hist_out + (long)level * SEG_OHEM_BINS);
}

// Sum pass (TOP-K only): the workgroup's sum of the l > t in fp64 - per lane in its stride order, xor butterflies, wave order.
__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_sum_kernel(const seg_ohem_rec* rec, const float* l, long n, double* part) {
    if (rec->branch != SEG_OHEM_TOPK) return;
    __shared__ double red[SEG_THREADS / 64];
    const float t = seg_ohem_unkey(rec->prefix);
    const long quads = n / 4;
    double s = 0.0;
    for (long q = (long)blockIdx.x * SEG_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * SEG_THREADS) {
        const float4 v = sgx_ld4(l + 4 * q);
        s += (double)(v.x > t ? v.x : 0.f);
        s += (double)(v.y > t ? v.y : 0.f);
        s += (double)(v.z > t ? v.z : 0.f);
        s += (double)(v.w > t ? v.w : 0.f);
    }
    if (blockIdx.x == 0 && 4 * quads + (long)threadIdx.x < n) {
        const float v = l[4 * quads + threadIdx.x];
        s += (double)(v > t ? v : 0.f);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < SEG_THREADS / 64; ++w) r += red[w];
        part[blockIdx.x] = r;
    }
}

// Final step (one workgroup): the loss and the gradient pass's weights.
//   BAR   : sum / cnt_gt, weight 1 / cnt_gt above thresh          TOP-K: (sum_{l>t} + (k - c_gt) t) / k, weight 1 / k above t and the rest of the
//   NONE  : 0 (empty set), no weight                                      k shared by the c_eq pixels equal to t (symmetric in a tie)
//   NAN   : nan (the mean of no pixel), no weight
__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_final_kernel(seg_ohem_rec* rec, const double* part, int nparts, float thresh, float* loss) {
    __shared__ double sd[SEG_THREADS];
    const int tid = threadIdx.x, branch = rec->branch;
    double s = 0.0;
    if (branch == SEG_OHEM_TOPK)
        for (int i = tid; i < nparts; i += SEG_THREADS) s += part[i];
    sd[tid] = s;
    __syncthreads();
    for (int w = SEG_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) sd[tid] += sd[tid + w];
        __syncthreads();
    }
    if (tid != 0) return;
    float t = INFINITY, w_gt = 0.f, w_eq = 0.f, out = 0.f;
    if (branch == SEG_OHEM_BAR) {
        t = thresh;
        out = (float)(rec->sum_thresh / (double)rec->cnt_gt);
        w_gt = (float)(1.0 / (double)rec->cnt_gt);
    } else if (branch == SEG_OHEM_NAN) {
        out = __uint_as_float(0x7fc00000u);
    } else if (branch == SEG_OHEM_TOPK) {
        const double k = (double)rec->num_mining, at_t = (double)(rec->num_mining - rec->c_gt);
        t = seg_ohem_unkey(rec->prefix);
        out = (float)((sd[0] + at_t * (double)t) / k);
        w_gt = (float)(1.0 / k);
        w_eq = (float)(at_t / ((double)rec->c_eq * k));
    }
    rec->t_eff = t;
    rec->w_gt = w_gt;
    rec->w_eq = w_eq;
    loss[0] = out;
}

// ---------------------------------------------------------------------------------------------
// Gradient pass: weight of each pixel from l and the record.  A workgroup whose chunk holds no selected pixel (wave ballots, or-ed through
// LDS: the same answer in every lane) writes its zeros without loading a label or a plane; the others recompute the softmax from the planes.
// ---------------------------------------------------------------------------------------------
template <bool VEC, bool REG>
__global__ __launch_bounds__(SEG_THREADS) void seg_ohem_grad_kernel(int C, int P, const float* logits, const int64_t* labels, int ignore_index, const float* l,
                                                                    const seg_ohem_rec* rec, float* dlogits) {
    __shared__ int any_wave[SEG_THREADS / 64];
    const int n = blockIdx.y, i0 = seg_first<VEC>((int)blockIdx.x);
    const float* xin = logits + (long)n * C * P;
    float* gout = dlogits + (long)n * C * P;
    const float t = rec->t_eff, w_gt = rec->w_gt, w_eq = rec->w_eq;
    float lv[SEG_PIX], w[SEG_PIX];
    seg_ld<VEC>(l + (long)n * P, i0, P, lv);
    bool any = false;
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k) {
        w[k] = seg_ohem_live<VEC>(i0, P, k) ? (lv[k] > t ? w_gt : (lv[k] == t ? w_eq : 0.f)) : 0.f;
        any = any || w[k] != 0.f;
    }
    const unsigned long long ballot = __ballot(any);
    if ((threadIdx.x & 63) == 0) any_wave[threadIdx.x >> 6] = ballot != 0ull;
    __syncthreads();
    bool active = false;
    for (int i = 0; i < SEG_THREADS / 64; ++i) active = active || any_wave[i];
    if (!active) {
        const float z[SEG_PIX] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) seg_st<VEC>(gout + (long)c * P, i0, P, z);
        return;
    }
    int cls[SEG_PIX];
    float wy[SEG_PIX], m[SEG_PIX], s[SEG_PIX], xy[SEG_PIX];
    seg_ce_classes<VEC>(labels + (long)n * P, i0, P, C, ignore_index, nullptr, cls, wy);
#pragma unroll
    for (int k = 0; k < SEG_PIX; ++k)
        if (cls[k] < 0) w[k] = 0.f;  // an ignored pixel that takes part with loss 0 can sit at the bar: still zero in every plane
    if (REG) {
        float x[SEG_CE_REG_CAP][SEG_PIX];
        seg_ohem_reg_stats<VEC>(xin, i0, P, C, cls, x, m, s, xy);
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) s[k] = 1.f / s[k];
#pragma unroll
        for (int c = 0; c < SEG_CE_REG_CAP; ++c)
            if (c < C) {
                float g[SEG_PIX];
#pragma unroll
                for (int k = 0; k < SEG_PIX; ++k) g[k] = w[k] != 0.f ? w[k] * (x[c][k] * s[k] - (c == cls[k] ? 1.f : 0.f)) : 0.f;
                seg_st<VEC>(gout + (long)c * P, i0, P, g);
            }
    } else {
        seg_ohem_stream_stats<VEC>(xin, i0, P, C, cls, m, s, xy);
#pragma unroll
        for (int k = 0; k < SEG_PIX; ++k) s[k] = 1.f / s[k];
        for (int c0 = 0; c0 < C; c0 += SEG_STREAM_PLANES) {
            float x[SEG_STREAM_PLANES][SEG_PIX];
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) seg_ld<VEC>(xin + (long)(c0 + j) * P, i0, P, x[j]);
#pragma unroll
            for (int j = 0; j < SEG_STREAM_PLANES; ++j)
                if (c0 + j < C) {
                    float g[SEG_PIX];
#pragma unroll
                    for (int k = 0; k < SEG_PIX; ++k)
                        g[k] = w[k] != 0.f ? w[k] * (expf(x[j][k] - m[k]) * s[k] - (c0 + j == cls[k] ? 1.f : 0.f)) : 0.f;
                    seg_st<VEC>(gout + (long)(c0 + j) * P, i0, P, g);
                }
        }
    }
}

struct seg_ohem_ws {
    long hist, part_set, part_gt, part_sum, part_l, l, total;
};
static seg_ohem_ws seg_ohem_layout(int N, int P) {
    const long nwg = (long)N * sgx_cdiv(P, SEG_CHUNK);
    seg_ohem_ws w;
    w.hist = SEG_OHEM_OFF_HIST;
    w.part_l = SEG_OHEM_OFF_PART_L;
    w.part_set = SEG_OHEM_OFF_PART;
    w.part_gt = w.part_set + nwg * 4;
    w.part_sum = w.part_gt + nwg * 4;
    w.l = SEG_OHEM_OFF_L(nwg);
    w.total = w.l + (long)N * P * 4;
    return w;
}
extern "C" int64_t sgx_seg_ohem_ws_bytes(int32_t N, int32_t P) { return N > 0 && P > 0 ? seg_ohem_layout(N, P).total : 0; }

#define SEG_OHEM_LAUNCH4(kernel, vec, reg, grid, ...)                                                  \
    do {                                                                                               \
        if ((vec) && (reg)) SGX_LAUNCH((kernel<true, true>), grid, block, 0, stream, __VA_ARGS__);     \
        else if (vec) SGX_LAUNCH((kernel<true, false>), grid, block, 0, stream, __VA_ARGS__);          \
        else if (reg) SGX_LAUNCH((kernel<false, true>), grid, block, 0, stream, __VA_ARGS__);          \
        else SGX_LAUNCH((kernel<false, false>), grid, block, 0, stream, __VA_ARGS__);                  \
    } while (0)

// loss: one float; dlogits [N,C,P] = d loss / d logits (multiply by the upstream gradient); ws: sgx_seg_ohem_ws_bytes(N, P) bytes, 16-byte aligned
extern "C" int32_t sgx_seg_ohem_ce_fwd_bwd(int32_t N, int32_t C, int32_t P, const float* logits, const int64_t* labels, int32_t ignore_index, float thresh,
                                           double mining_percent, int32_t exclude_ignored, void* ws, int64_t ws_bytes, float* loss, float* dlogits, void* stream) {
    SGX_CHECK_ARG(logits && labels && ws && loss && dlogits && N > 0 && C > 0 && P > 0, "seg_ohem_ce: bad args");
    SGX_CHECK_ARG(N <= 65535 && P <= SEG_MAX_P, "seg_ohem_ce: at most 65535 images of 2^30 pixels (got %d x %d)", N, P);
    SGX_CHECK_ARG(mining_percent >= 0.0 && mining_percent <= 1.0, "seg_ohem_ce: mining_percent %g outside [0, 1]", mining_percent);
    const int chunks = sgx_cdiv(P, SEG_CHUNK);
    SGX_CHECK_ARG((long)N * chunks <= 0x7fffffffL / 2, "seg_ohem_ce: too many workgroups");
    const seg_ohem_ws o = seg_ohem_layout(N, P);
    SGX_CHECK_ARG(ws_bytes >= o.total && SEG_ALIGNED16(ws), "seg_ohem_ce: workspace of %ld bytes, 16-byte aligned, needed (got %ld)", o.total, (long)ws_bytes);
    char* base = (char*)ws;
    seg_ohem_rec* rec = (seg_ohem_rec*)base;
    unsigned long long* hist = (unsigned long long*)(base + o.hist);
    unsigned *pset = (unsigned*)(base + o.part_set), *pgt = (unsigned*)(base + o.part_gt);
    float *psum = (float*)(base + o.part_sum), *l = (float*)(base + o.l);
    double* pl = (double*)(base + o.part_l);
    const int nwg = N * chunks;
    const long total = (long)N * P;
    const bool vec = seg_vec_ok(P, logits, dlogits, labels), reg = C <= SEG_CE_REG_CAP;
    const dim3 grid((unsigned)chunks, (unsigned)N), block(SEG_THREADS), one(1);
    const int quads_wgs = sgx_cdiv(total / 4 > 0 ? total / 4 : 1, SEG_THREADS);
    const dim3 stream_grid((unsigned)SGX_STRIDE_GRID(quads_wgs < SEG_OHEM_WGS ? quads_wgs : SEG_OHEM_WGS));
    const int nzero = (int)(o.part_l / 8);  // the record and the histograms
    SGX_LAUNCH(seg_ohem_zero_kernel, dim3((unsigned)SGX_STRIDE_GRID(sgx_cdiv(nzero, SEG_THREADS))), block, 0, stream, (unsigned long long*)base, nzero);
    SEG_OHEM_LAUNCH4(seg_ohem_pixel_kernel, vec, reg, grid, C, P, logits, labels, ignore_index, exclude_ignored, thresh, base);
    SGX_CHECK_LAUNCH("seg_ohem_ce pixel pass");
    for (int level = 0; level < 3; ++level) {
        if (level > 0) SGX_LAUNCH(seg_ohem_refine_kernel, stream_grid, block, 0, stream, level, (const seg_ohem_rec*)rec, (const float*)l, total, hist);
        SGX_LAUNCH(seg_ohem_select_kernel, one, block, 0, stream, level, rec, (const unsigned long long*)hist, (const unsigned*)pset, (const unsigned*)pgt,
                   (const float*)psum, nwg, thresh, mining_percent);
    }
    SGX_CHECK_LAUNCH("seg_ohem_ce select");
    SGX_LAUNCH(seg_ohem_sum_kernel, stream_grid, block, 0, stream, (const seg_ohem_rec*)rec, (const float*)l, total, pl);
    SGX_LAUNCH(seg_ohem_final_kernel, one, block, 0, stream, rec, (const double*)pl, (int)stream_grid.x, thresh, loss);
    SGX_CHECK_LAUNCH("seg_ohem_ce sum");
    SEG_OHEM_LAUNCH4(seg_ohem_grad_kernel, vec, reg, grid, C, P, logits, labels, ignore_index, (const float*)l, (const seg_ohem_rec*)rec, dlogits);
    SGX_CHECK_LAUNCH("seg_ohem_ce gradient pass");
    return SGX_OK;
}
