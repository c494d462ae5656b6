// Detection post-processing on gfx950: score filter -> exact top-k -> greedy NMS.  No MFMA: candidate selection is an HBM stream over the
// B*L*C scores, suppression is latency-bound.
//
// Replaces PPYoloEPostPredictionCallback.forward (pp_yolo_e/post_prediction_callback.py:42-123) and the
// torchvision.ops.nms / batched_nms it calls (:85,87).  Ordering rule (matches a stable descending sort):
// candidates are ranked by (score desc, candidate index asc), candidate index = anchor*C + class
// (the row-major order of `(scores > thr).nonzero()`), or the anchor index in single-label mode; the composite key
// (score bits << 22 | ~index) is unique, so "the top k" is a set, whatever order candidates are visited in.
//
// Multi-label mode (the recipes' setting) runs in two stages:
//   stage 1, the WHOLE chip (grid = score slabs x images, 16-byte loads): two histogram passes narrow the k-th largest key down to its top 22
//            bits (11 bits per pass: LDS histogram per workgroup, merged with global atomics), a third pass appends every candidate at or
//            above that 22-bit prefix - the top k plus the few that share the boundary bin - to a per-image list;
//   stage 2, one workgroup per image on the list: exact radix select of the k-th key, bitonic sort in LDS, then suppression as a
//            triangular IoU bit matrix (all pairs in parallel) scanned by ONE wave without barriers - the torchvision-CUDA formulation,
//            kept on the device.
// (Round 1 ran everything in one 1024-thread workgroup per image: seven passes over the image's 672k scores with 32 of 256 CUs busy and
// two barriers per kept box - 2.17 ms per 32-image batch.)  Single-label mode and lists that overflow (more than NMS_LIST_CAP candidates
// sharing the boundary prefix: pathological ties) take stage 2's streaming path over the raw scores, which needs no list.
// Compile with -ffp-contract=off: the IoU test must round exactly like the CPU restatement.
#include "sgx_common.h"

#define NMS_THREADS 1024
#define NMS_MAXK_LIMIT 4096  // largest instantiated top-k capacity (LDS: 37 B per candidate + 8 KB histogram <= 160 KB)
#define NMS_IDXBITS 22
#define NMS_HBINS 2048
#define NMS_LIST_CAP 8192    // per-image candidate list of stage 1 (top k <= 4096 + boundary-bin slack)
#define NMS_S1_THREADS 256
// per-image counters of stage 1 (word 0: keys appended to the list, word 1: candidates above the score threshold), ONE 128-byte line per
// image: every workgroup of a selection pass ends with an atomic on them, and atomics on 32 counters packed into one line serialise
// through one L2 channel (r5k: 2 x 1344 of them cost the one-pass kernel 15 of its 30 us)
#define NMS_CTR_INTS 32

typedef unsigned long long u64;
#include <atomic>
static std::atomic<int> g_nms_split{1};
extern "C" int32_t sgx_debug_set_nms_split(int32_t on) {
    g_nms_split = on != 0;
    return SGX_OK;
}

// workspace layout (ints unless noted): hist1 [B][2048] | hist2 [B][2048] | list_count [B] | total [B] | list (u64) [B][NMS_LIST_CAP]
// ... | per image (split suppression, top-k <= 1024): sorted candidates (keys u64[1024], boxes f32[1024][4], boxes as the IoU test sees them
// f32[1024][4], areas f32[1024], classes int[1024], {n, class mode} int[16]) and the triangular suppression bit matrix u64[8704]
#define NMS_SPLIT_K 1024
#define NMS_CAND_BYTES (NMS_SPLIT_K * (8 + 16 + 16 + 4 + 4) + 64)
#define NMS_MASK_WORDS_1024 8704
#define NMS_SPLIT_BYTES (NMS_CAND_BYTES + NMS_MASK_WORDS_1024 * 8)
static int64_t nms_ws_head(const sgx_nms_desc* d) { return (((int64_t)d->B * (2 * NMS_HBINS + NMS_CTR_INTS) * 4 + 255) & ~255L) + (int64_t)d->B * NMS_LIST_CAP * 8; }
extern "C" int64_t sgx_nms_workspace(const sgx_nms_desc* d) {
    if (!d || !d->multi_label) return 256;
    return nms_ws_head(d) + 256 + (int64_t)d->B * NMS_SPLIT_BYTES;
}

__device__ __forceinline__ bool nms_candidate(const sgx_nms_desc& d, const float* sc, long e, float& score, int& cls) {
    if (d.multi_label) {
        score = sc[e];
        cls = (int)(e % d.C);
        return score > d.score_threshold;
    }
    const float* row = sc + e * d.C;
    float m = row[0];
    int mi = 0;
    for (int c = 1; c < d.C; ++c)
        if (row[c] > m) {
            m = row[c];
            mi = c;
        }
    score = m;
    cls = mi;
    return m >= d.score_threshold;
}
__device__ __forceinline__ u64 nms_key(float score, long e) {
    return ((u64)__float_as_uint(score) << NMS_IDXBITS) | (u64)(((1u << NMS_IDXBITS) - 1u) - (unsigned)e);
}

// ---- stage 1 (multi-label): candidate selection over the whole chip ---------------------------------------------------------------
// Bin of the k-th largest entry of a histogram counted from the top bin, how many entries lie strictly above that bin, and the total.
// Every thread of the NT-thread workgroup calls it (three barriers); thread t owns nbins / NT consecutive bins, a suffix sum over the threads
// (wave shuffles + one LDS hop across waves) finds the thread whose bins contain the k-th entry - no serial walk over the bins (round 1's
// thread-0 loop over 2048 bins per radix digit was most of the per-image time).  Fewer than k entries in total: bin = 0, above = 0
// ("everything at or above bin 0").  hist may be global memory written by an earlier kernel.  sh: NT / 64 + 3 ints of LDS.
template <int NT>
__device__ __forceinline__ void nms_kth_from_top(const int* hist, int nbins, int k, int* sh, int& bin, int& above, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = NT / 64;
    const int per = nbins / NT;
    int local = 0;
    for (int q = 0; q < per; ++q) local += hist[tid * per + q];
    int v = local;  // -> sum over the lanes >= lane of this wave
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(v, off);
        if (lane + off < 64) v += t;
    }
    if (tid == 0) {
        sh[NW] = 0;
        sh[NW + 1] = 0;
    }
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    int higher = 0, all = 0;
    for (int w = 0; w < NW; ++w) {
        const int t = sh[w];
        all += t;
        if (w > wave) higher += t;
    }
    const int incl = v + higher, excl = incl - local;
    if (excl < k && incl >= k) {
        int cum = excl, b = (tid + 1) * per - 1;
        for (; b > tid * per; --b) {
            if (cum + hist[b] >= k) break;
            cum += hist[b];
        }
        sh[NW] = b;
        sh[NW + 1] = cum;
    }
    __syncthreads();
    bin = sh[NW];
    above = sh[NW + 1];
    total = all;
    __syncthreads();  // sh may be reused by the next call
}
// PASS 0: hist1 over key bits 52..42 (score bits 30..20).  PASS 1: hist2 over key bits 41..31 among keys in hist1's boundary bin.
// PASS 2: append the keys at or above the 22-bit boundary prefix to the image's list; total[b] = number of candidates.
template <int PASS>
__global__ __launch_bounds__(NMS_S1_THREADS) void nms_select_kernel(sgx_nms_desc d, const float* scores, int* ws, int slab) {
    __shared__ int lh[NMS_HBINS];
    __shared__ int part[NMS_S1_THREADS / 64 + 3];
    __shared__ int lcount, lbase;
    u64* const lbuf = reinterpret_cast<u64*>(lh);  // PASS 2 reuses the histogram's LDS: up to NMS_HBINS / 2 selected keys per workgroup
    const int b = blockIdx.y, tid = threadIdx.x;
    const long E = (long)d.L * d.C;
    const float* sc = scores + (long)b * E;
    int* hist1 = ws + (long)b * NMS_HBINS;
    int* hist2 = ws + ((long)d.B + b) * NMS_HBINS;
    int* list_count = ws + 2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS;
    int* total = ws + 2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS + 1;
    u64* list = reinterpret_cast<u64*>(reinterpret_cast<char*>(ws) + (((long)d.B * (2 * NMS_HBINS + NMS_CTR_INTS) * 4 + 255) & ~255L)) + (long)b * NMS_LIST_CAP;
    const int K = d.nms_top_k;
    int b1 = 0, above1 = 0, b2 = 0, above2 = 0, tot1 = 0, tot2 = 0;
    if (PASS >= 1) nms_kth_from_top<NMS_S1_THREADS>(hist1, NMS_HBINS, K, part, b1, above1, tot1);
    if (PASS >= 2) {
        nms_kth_from_top<NMS_S1_THREADS>(hist2, NMS_HBINS, K - above1, part, b2, above2, tot2);
        if (blockIdx.x == 0 && tid == 0) total[0] = tot1;
    }
    if (PASS < 2) {
        for (int q = tid; q < NMS_HBINS; q += NMS_S1_THREADS) lh[q] = 0;
    } else if (tid == 0) lcount = 0;
    __syncthreads();
    const long e0 = (long)blockIdx.x * slab, e1 = e0 + slab < E ? e0 + slab : E;
    const bool vec = ((((uintptr_t)sc) & 15) == 0) && (e0 % 4 == 0);
    auto visit = [&](float s, long e) {
        if (!(s > d.score_threshold)) return;
        const u64 k = nms_key(s, e);
        const int h1 = (int)(k >> 42), h2 = (int)((k >> 31) & (NMS_HBINS - 1));
        if (PASS == 0) atomicAdd(&lh[h1], 1);
        else if (PASS == 1) {
            if (h1 == b1) atomicAdd(&lh[h2], 1);
        } else if (h1 > b1 || (h1 == b1 && h2 >= b2)) {
            // collected in LDS first: ONE global atomic per workgroup reserves its range of the image's list (one atomic per key, on 32
            // counters that share a cache line, cost 220 us per batch - r2n); a workgroup with more than NMS_HBINS / 2 selected keys
            // (pathological ties) appends the excess directly
            const int slot = atomicAdd(&lcount, 1);
            if (slot < NMS_HBINS / 2) lbuf[slot] = k;
            else {
                const int g = atomicAdd(list_count, 1);
                if (g < NMS_LIST_CAP) list[g] = k;
            }
        }
    };
    long e = e0 + (vec ? 4L * tid : tid);
    if (vec) {
        for (; e + 3 < e1; e += 4L * NMS_S1_THREADS) {
            const float4 v = sgx_ld4(sc + e);
            visit(v.x, e); visit(v.y, e + 1); visit(v.z, e + 2); visit(v.w, e + 3);
        }
        for (long r = e; r < e1 && r < e + 4; ++r) visit(sc[r], r);  // ragged tail of the slab (at most one lane has one)
    } else {
        for (; e < e1; e += NMS_S1_THREADS) visit(sc[e], e);
    }
    __syncthreads();
    if (PASS < 2) {
        int* gh = PASS == 0 ? hist1 : hist2;
        for (int q = tid; q < NMS_HBINS; q += NMS_S1_THREADS)
            if (lh[q]) atomicAdd(&gh[q], lh[q]);
    } else {
        const int cnt = lcount < NMS_HBINS / 2 ? lcount : NMS_HBINS / 2;
        if (tid == 0 && cnt) lbase = atomicAdd(list_count, cnt);
        __syncthreads();
        for (int q = tid; q < cnt; q += NMS_S1_THREADS)
            if (lbase + q < NMS_LIST_CAP) list[lbase + q] = lbuf[q];
    }
}

// ---- stage 1, round 5: ONE pass over the scores behind a sampled threshold --------------------------------------------------------------
// The three passes above read the 86 MB of scores three times to find the k-th largest key EXACTLY before a single key is selected.
// Stage 2 does not need that: any superset of the top k that fits its list is as good (it selects / sorts exactly).  So a threshold is
// first ESTIMATED from a sample: one 128-byte line out of every NMS_SAMPLE_STEP (1/32 of the scores, whole lines: 2.7 MB per batch), per
// image the r-th largest sampled key, r = k / 10 - the threshold's true rank is then about 32 r = 3.2 k with a spread of 32 sqrt(r)
// (k = 1000: 3200 +- 320), i.e. at least k and at most the list's 8192 entries by a wide margin; its two histogram levels resolve the top
// 22 bits of the key, like the exact selection's.  Then ONE pass appends every key at or above the threshold and counts the candidates.
// Exactness does not rest on the estimate: stage 2 takes the list only if it holds at least min(k, candidates) keys and did not
// overflow - otherwise (adversarial inputs: the sample missing the top of the distribution) it streams the image's raw scores itself,
// the path a caller without a workspace always gets.  Same rows bit for bit either way (tests: every test_nms* under both selections).
#define NMS_SAMPLE_STEP 32
static std::atomic<int> g_nms_sampled{1};
extern "C" int32_t sgx_debug_set_nms_selection(int32_t sampled) {  // measurement / tests: 0 = the exact three-pass selection
    g_nms_sampled = sampled ? 1 : 0;
    return SGX_OK;
}
// where sgx_nms leaves "image b's stage 2 streamed the raw scores instead of stage 1's list" (1 / 0): int index offset + b * stride of the
// workspace the call was given (multi-label calls with a workspace; read it after the call's stream work is done)
extern "C" int32_t sgx_debug_nms_fallback_slot(const sgx_nms_desc* d, int64_t* offset_ints, int32_t* stride_ints) {
    SGX_CHECK_ARG(d && offset_ints && stride_ints, "nms fallback slot: null pointer");
    *offset_ints = 2L * d->B * NMS_HBINS + 2;
    *stride_ints = NMS_CTR_INTS;
    return SGX_OK;
}
__global__ __launch_bounds__(NMS_THREADS) void nms_sample_kernel(sgx_nms_desc d, const float* scores, int* ws) {
    __shared__ int hist[NMS_HBINS];
    __shared__ int sh[NMS_THREADS / 64 + 3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long E = (long)d.L * d.C;
    const float* sc = scores + (long)b * E;
    int* const thr_words = ws + (long)b * NMS_HBINS;  // (the first histogram's slot of this image: two words hold the threshold key)
    int* list_count = ws + 2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS;
    int* total = ws + 2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS + 1;
    const long lines = E / 32, slines = (lines + NMS_SAMPLE_STEP - 1) / NMS_SAMPLE_STEP;  // sampled lines: 0, STEP, 2 STEP, ...
    const long ns4 = slines * 8;
    const int r = d.nms_top_k / 10 > 8 ? d.nms_top_k / 10 : 8;
    int b1 = 0, above1 = 0, tot1 = 0, b2 = 0, above2 = 0, tot2 = 0;
#pragma unroll 1
    for (int level = 0; level < 2; ++level) {
        for (int q = tid; q < NMS_HBINS; q += NMS_THREADS) hist[q] = 0;
        __syncthreads();
        // (four independent 16-byte loads per trip: one workgroup per image has nothing else to hide their latency behind)
        for (long s0 = tid; s0 < ns4; s0 += 4L * NMS_THREADS) {
            float4 v[4];
            long e4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long s4 = s0 + (long)u * NMS_THREADS;
                e4[u] = (s4 >> 3) * (32L * NMS_SAMPLE_STEP) + (s4 & 7) * 4;
                const bool ok = s4 < ns4 && e4[u] + 3 < E;
                v[u] = ok ? sgx_ld4(sc + e4[u]) : make_float4(0.f, 0.f, 0.f, 0.f);  // (0 is never above the non-negative score threshold)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float vv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (!(vv[i] > d.score_threshold)) continue;
                    const u64 k = nms_key(vv[i], e4[u] + i);
                    const int h1 = (int)(k >> 42), h2 = (int)((k >> 31) & (NMS_HBINS - 1));
                    if (level == 0) atomicAdd(&hist[h1], 1);
                    else if (h1 == b1) atomicAdd(&hist[h2], 1);
                }
            }
        }
        __syncthreads();
        if (level == 0) nms_kth_from_top<NMS_THREADS>(hist, NMS_HBINS, r, sh, b1, above1, tot1);
        else nms_kth_from_top<NMS_THREADS>(hist, NMS_HBINS, r - above1, sh, b2, above2, tot2);
    }
    if (tid == 0) {
        // fewer than r sampled candidates: everything above the score threshold is selected (key 0 sorts below every real key)
        const u64 thr = tot1 < r ? 0ull : (((u64)b1 << 42) | ((u64)b2 << 31));
        thr_words[0] = (int)(unsigned)(thr & 0xffffffffu);
        thr_words[1] = (int)(unsigned)(thr >> 32);
        list_count[0] = 0;
        total[0] = 0;
    }
}
// the one pass: keys >= the image's sampled threshold -> its list (LDS first, one global atomic per workgroup), candidates counted
__global__ __launch_bounds__(NMS_S1_THREADS) void nms_append_kernel(sgx_nms_desc d, const float* scores, int* ws, int slab) {
    __shared__ u64 lbuf[NMS_HBINS / 2];
    __shared__ int lcount, lbase, lcand;
    const int b = blockIdx.y, tid = threadIdx.x;
    const long E = (long)d.L * d.C;
    const float* sc = scores + (long)b * E;
    const int* thr_words = ws + (long)b * NMS_HBINS;
    int* list_count = ws + 2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS;
    int* total = ws + 2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS + 1;
    u64* list = reinterpret_cast<u64*>(reinterpret_cast<char*>(ws) + (((long)d.B * (2 * NMS_HBINS + NMS_CTR_INTS) * 4 + 255) & ~255L)) + (long)b * NMS_LIST_CAP;
    const u64 thr = ((u64)(unsigned)thr_words[1] << 32) | (u64)(unsigned)thr_words[0];
    if (tid == 0) lcount = 0, lcand = 0;
    __syncthreads();
    const long e0 = (long)blockIdx.x * slab, e1 = e0 + slab < E ? e0 + slab : E;
    const bool vec = ((((uintptr_t)sc) & 15) == 0) && (e0 % 4 == 0);
    // Selected keys wait in four registers per lane and reach LDS after the streaming loop with ONE counter update per lane: at the
    // ~0.5 % of the scores the sampled threshold lets through, 7 of 10 wave-trips of the loop hold a selected key, and a returning LDS
    // atomic inside the loop parked every one of them (r5i: this pass 30 us where the histogram pass of the same bytes takes 15).  A
    // lane with more than four (clustered scores) appends the excess at once, as before.
    int cand = 0, nm = 0;
    u64 m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    auto put = [&](u64 k) {
        const int slot = atomicAdd(&lcount, 1);
        if (slot < NMS_HBINS / 2) lbuf[slot] = k;
        else {
            const int g = atomicAdd(list_count, 1);
            if (g < NMS_LIST_CAP) list[g] = k;
        }
    };
    auto visit = [&](float s, long e) {
        if (!(s > d.score_threshold)) return;
        ++cand;
        const u64 k = nms_key(s, e);
        if (k >= thr) {
            if (nm < 4) {
                m3 = m2; m2 = m1; m1 = m0; m0 = k;
                ++nm;
            } else put(k);
        }
    };
    long e = e0 + (vec ? 4L * tid : tid);
    if (vec) {
        // eight independent 16-byte loads per trip, THEN the visits: the visits' stores and atomics (which may alias the scores as far as
        // the compiler knows) otherwise pin every load behind the previous trip - sixteen memory latencies in a row per lane (r5j: this
        // pass 30 us against 15 for the histogram pass over the same bytes)
        constexpr int U = 8;
        for (; e + 3 + 4L * NMS_S1_THREADS * (U - 1) < e1; e += 4L * NMS_S1_THREADS * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = sgx_ld4(sc + e + 4L * NMS_S1_THREADS * u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long eu = e + 4L * NMS_S1_THREADS * u;
                visit(v[u].x, eu); visit(v[u].y, eu + 1); visit(v[u].z, eu + 2); visit(v[u].w, eu + 3);
            }
        }
        for (; e + 3 < e1; e += 4L * NMS_S1_THREADS) {
            const float4 v = sgx_ld4(sc + e);
            visit(v.x, e); visit(v.y, e + 1); visit(v.z, e + 2); visit(v.w, e + 3);
        }
        for (long q = e; q < e1 && q < e + 4; ++q) visit(sc[q], q);
    } else {
        for (; e < e1; e += NMS_S1_THREADS) visit(sc[e], e);
    }
    if (nm > 0) put(m0);
    if (nm > 1) put(m1);
    if (nm > 2) put(m2);
    if (nm > 3) put(m3);
    for (int off = 32; off > 0; off >>= 1) cand += __shfl_down(cand, off);
    if ((tid & 63) == 0 && cand) atomicAdd(&lcand, cand);
    __syncthreads();
    const int cnt = lcount < NMS_HBINS / 2 ? lcount : NMS_HBINS / 2;
    if (tid == 0 && (cnt || lcand)) {  // both counters in one 64-bit atomic (low word: list count - its old value is this workgroup's base)
        const u64 old = atomicAdd(reinterpret_cast<unsigned long long*>(list_count), ((u64)(unsigned)lcand << 32) | (u64)(unsigned)cnt);
        lbase = (int)(unsigned)(old & 0xffffffffu);
    }
    __syncthreads();
    for (int q = tid; q < cnt; q += NMS_S1_THREADS)
        if (lbase + q < NMS_LIST_CAP) list[lbase + q] = lbuf[q];
}

// ---- stage 2: one workgroup per image --------------------------------------------------------------------------------------------
// Triangular suppression bit matrix for NMS_MAXK = 1024: row i keeps the 64-bit words w >= i / 64 (bit j of word w: "i suppresses 64*w + j").
// Rows are grouped in blocks of 64 (g = i / 64, 16 - g words per row): 8 704 words = 68 KB of LDS.
#define NMS_MW 16
__device__ __forceinline__ int nms_mask_row(int i) {
    const int g = i >> 6;
    return 64 * (NMS_MW * g - g * (g - 1) / 2) + (i & 63) * (NMS_MW - g);
}
template <int NMS_MAXK>
__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(sgx_nms_desc d, const float* boxes, const float* scores, float* out, int* out_count,
                                                          int* out_index, int* num_candidates, const int* ws, char* split) {
    constexpr bool MASK = NMS_MAXK == 1024;
    __shared__ int hist[NMS_HBINS];
    __shared__ u64 keys[NMS_MAXK];
    __shared__ float bx[NMS_MAXK][4];
    __shared__ float area[NMS_MAXK];
    __shared__ int cls_s[NMS_MAXK];
    __shared__ unsigned char sup[NMS_MAXK];
    __shared__ int s_count, s_n, s_kept, s_remaining;
    __shared__ u64 s_prefix;
    __shared__ float s_maxc;
    __shared__ int keep_list[NMS_MAXK];
    __shared__ float wmax[NMS_THREADS / 64];
    __shared__ float cur[5];
    __shared__ int kth_sh[NMS_THREADS / 64 + 3];
    __shared__ u64 rem[NMS_MW];
    __shared__ u64 mask[MASK ? 64 * (NMS_MW * (NMS_MW + 1) / 2) : 1];

    const int b = blockIdx.x, tid = threadIdx.x;
    const float* sc = scores + (long)b * d.L * d.C;
    const float* bxs = boxes + (long)b * d.L * 4;
    const long E = d.multi_label ? (long)d.L * d.C : (long)d.L;
    const int K = d.nms_top_k < NMS_MAXK ? d.nms_top_k : NMS_MAXK;
    // stage 1's list (multi-label with a workspace): every candidate at or above the 22-bit boundary prefix - a superset of the top K
    const int m_list = ws ? ws[2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS] : 0;
    // (sampled selection: the list must also hold at least min(K, candidates) keys - a threshold estimated too high is the one way it
    // could miss part of the top K; the exact selection's list always does)
    const int m_cand = ws ? ws[2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS + 1] : 0;
    const bool use_list = ws != nullptr && m_list <= NMS_LIST_CAP && m_list >= (m_cand < K ? m_cand : K);
    //  the streaming fallback is exact but many times slower than the list: every call leaves, per image, whether stage 2 took it
    // (int 2 of the image's counter line; sgx_debug_nms_fallback_slot) so that benches and tests can assert the sampled selection held
    if (ws != nullptr && d.multi_label && tid == 0) const_cast<int*>(ws)[2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS + 2] = use_list ? 0 : 1;
    const u64* list = ws ? reinterpret_cast<const u64*>(reinterpret_cast<const char*>(ws) + (((long)d.B * (2 * NMS_HBINS + NMS_CTR_INTS) * 4 + 255) & ~255L)) + (long)b * NMS_LIST_CAP
                         : nullptr;
    // visits every candidate's composite key: the list, or (single-label / overflowing list) the raw scores of the image
    auto for_each_key = [&](auto fn) {
        if (use_list) {
            for (int i = tid; i < m_list; i += NMS_THREADS) fn(list[i]);
        } else {
            for (long e = tid; e < E; e += NMS_THREADS) {
                float s;
                int c;
                if (nms_candidate(d, sc, e, s, c)) fn(nms_key(s, e));
            }
        }
    };

    // ---- pass 0: count candidates ----
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (use_list) {
        if (tid == 0) s_count = ws[2L * d.B * NMS_HBINS + (long)b * NMS_CTR_INTS + 1];
    } else {
        int local = 0;
        for_each_key([&](u64) { ++local; });
        if (local) atomicAdd(&s_count, local);
    }
    __syncthreads();
    const int count = s_count;
    const int n = count < K ? count : K;
    // ---- radix select of the n-th largest composite key (only when count > K) ----
    u64 thr_key = 0;  // select keys >= thr_key
    // (a list that fits the sort buffer needs no selection: it is a superset of the top K, sorting it whole puts the top n first - the
    // usual case, the list being the top K plus the few ties of the boundary bin; five histogram passes and ~25 barriers saved)
    if (count > K && !(use_list && m_list <= NMS_MAXK)) {
        const int total_bits = 31 + NMS_IDXBITS;  // 53
        const int widths[5] = {11, 11, 11, 11, total_bits - 44};
        if (tid == 0) {
            s_prefix = 0;
            s_remaining = K;
        }
        int shift = total_bits;
        for (int pass = 0; pass < 5; ++pass) {
            const int wbits = widths[pass];
            shift -= wbits;
            for (int i = tid; i < NMS_HBINS; i += NMS_THREADS) hist[i] = 0;
            __syncthreads();
            const u64 prefix = s_prefix;
            for_each_key([&](u64 k) {
                if ((k >> (shift + wbits)) == prefix) atomicAdd(&hist[(int)((k >> shift) & ((1u << wbits) - 1u))], 1);
            });
            __syncthreads();
            int dsel, cum, tot;
            nms_kth_from_top<NMS_THREADS>(hist, NMS_HBINS, s_remaining, kth_sh, dsel, cum, tot);  // (a 9-bit last digit leaves the upper bins at zero)
            if (tid == 0) {
                s_remaining = s_remaining - cum;
                s_prefix = (prefix << wbits) | (u64)dsel;
            }
            __syncthreads();
        }
        thr_key = s_prefix;
    }
    // ---- gather survivors (unordered), then bitonic sort descending ----
    if (tid == 0) s_n = 0;
    for (int i = tid; i < NMS_MAXK; i += NMS_THREADS) keys[i] = 0;  // 0 sorts last (real keys have score bits > 0)
    __syncthreads();
    for_each_key([&](u64 k) {
        if (k >= thr_key) {
            int slot = atomicAdd(&s_n, 1);
            if (slot < NMS_MAXK) keys[slot] = k;
        }
    });
    __syncthreads();
    if constexpr (NMS_MAXK == NMS_THREADS) {
        // one key per thread: the compare-exchange steps with a partner inside the wave (stride < 64: 45 of the 55 steps of a 1024-key
        // bitonic network) run on wave shuffles in registers - only the ten wide steps go through LDS and barriers
        u64 k = keys[tid];
        for (int size = 2; size <= NMS_MAXK; size <<= 1) {
            const bool desc = (tid & size) == 0;
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                u64 other;
                if (stride >= 64) {
                    keys[tid] = k;
                    __syncthreads();
                    other = keys[tid ^ stride];
                    __syncthreads();
                } else {
                    other = __shfl_xor(k, stride);
                }
                const bool lower = (tid & stride) == 0;
                const u64 hi = k > other ? k : other, lo = k > other ? other : k;
                k = (lower == desc) ? hi : lo;
            }
        }
        keys[tid] = k;
        __syncthreads();
    }
    for (int size = 2; size <= (NMS_MAXK == NMS_THREADS ? 0 : NMS_MAXK); size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < NMS_MAXK; i += NMS_THREADS) {
                int j = i ^ stride;
                if (j > i) {
                    u64 a = keys[i], c = keys[j];
                    bool desc = (i & size) == 0;
                    if (desc ? (a < c) : (a > c)) {
                        keys[i] = c;
                        keys[j] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // ---- load boxes / classes of the n survivors (candidate t is owned by thread t % NMS_THREADS) ----
    if (tid == 0) s_maxc = -INFINITY;
    __syncthreads();
    float mymax = -INFINITY;
    for (int t = tid; t < NMS_MAXK; t += NMS_THREADS) {
        if (t < n) {
            u64 k = keys[t];
            long e = (long)(((1u << NMS_IDXBITS) - 1u) - (unsigned)(k & ((1u << NMS_IDXBITS) - 1u)));
            long anchor = d.multi_label ? e / d.C : e;
            int c;
            if (d.multi_label) c = (int)(e % d.C);
            else {
                float s;
                nms_candidate(d, sc, e, s, c);
            }
            cls_s[t] = c;
            for (int q = 0; q < 4; ++q) {
                float v = bxs[anchor * 4 + q];
                bx[t][q] = v;
                mymax = fmaxf(mymax, v);
            }
        }
        sup[t] = 0;
    }
    // class_mode 3 = torchvision's own CPU dispatch (ops/boxes.py batched_nms): coordinate trick while boxes.numel() <= 4000
    const int class_mode = d.class_mode == 3 ? (4 * n > 4000 ? 2 : 1) : d.class_mode;
    if (class_mode == 1) {
        // torchvision batched_nms coordinate trick: boxes + cls * (max_coordinate + 1)
        for (int off = 32; off > 0; off >>= 1) mymax = fmaxf(mymax, __shfl_xor(mymax, off));
        if ((tid & 63) == 0) wmax[tid >> 6] = mymax;
        __syncthreads();
        if (tid == 0) {
            float m = wmax[0];
            for (int w = 1; w < NMS_THREADS / 64; ++w) m = fmaxf(m, wmax[w]);
            s_maxc = m;
        }
        __syncthreads();
    }
    __syncthreads();
    // boxes as the suppression test sees them: original coordinates (+ the class offset in mode 1), recomputed from LDS where needed
    const float offscale = class_mode == 1 ? s_maxc + 1.f : 0.f;
    auto nbox = [&](int t, float* o) {
        const float offv = class_mode == 1 ? (float)cls_s[t] * offscale : 0.f;
        for (int q = 0; q < 4; ++q) o[q] = bx[t][q] + offv;
    };
    for (int t = tid; t < n; t += NMS_THREADS) {
        float nb[4];
        nbox(t, nb);
        area[t] = (nb[2] - nb[0]) * (nb[3] - nb[1]);
    }
    if (tid == 0) s_kept = 0;
    __syncthreads();
    if (MASK && split && d.iou_threshold < 2.0f) {
        // Split suppression: this workgroup hands the sorted candidates over; the bit matrix is then built by the WHOLE chip (grid = 64-row
        // strips x images, nms_mask_kernel) and walked by one wave per image (nms_walk_kernel).  Inside this kernel the matrix build ran on
        // 32 of 256 CUs and was the larger half of the 170-190 us the call took (r2z profile).
        char* const o = split + (long)b * NMS_SPLIT_BYTES;
        u64* okeys = reinterpret_cast<u64*>(o);
        float* obx = reinterpret_cast<float*>(o + NMS_SPLIT_K * 8);
        float* onb = obx + NMS_SPLIT_K * 4;
        float* oarea = onb + NMS_SPLIT_K * 4;
        int* ocls = reinterpret_cast<int*>(oarea + NMS_SPLIT_K);
        int* ometa = ocls + NMS_SPLIT_K;
        for (int t = tid; t < NMS_SPLIT_K; t += NMS_THREADS) {
            okeys[t] = keys[t];
            if (t < n) {
                float nb[4];
                nbox(t, nb);
                for (int q = 0; q < 4; ++q) {
                    obx[t * 4 + q] = bx[t][q];
                    onb[t * 4 + q] = nb[q];
                }
                oarea[t] = area[t];
                ocls[t] = cls_s[t];
            }
        }
        if (tid == 0) {
            ometa[0] = n;
            ometa[1] = class_mode;
        }
        return;
    }
    // does box i (kept) suppress box t?  (the arithmetic order of torchvision's nms kernel)
    auto suppresses = [&](const float* ci, float ai, int t) {
        float nb[4];
        nbox(t, nb);
        float xx1 = fmaxf(ci[0], nb[0]), yy1 = fmaxf(ci[1], nb[1]);
        float xx2 = fminf(ci[2], nb[2]), yy2 = fminf(ci[3], nb[3]);
        float w = xx2 - xx1; w = w < 0.f ? 0.f : w;
        float h = yy2 - yy1; h = h < 0.f ? 0.f : h;
        float inter = w * h;
        float ovr = inter / (ai + area[t] - inter);
        return ovr > d.iou_threshold;
    };
    // An IoU never exceeds 1, so with a threshold >= 2 nothing can be suppressed and the scan degenerates to "the first max_predictions
    // of the sorted candidates": the pre-NMS top-k of the decoding modules (kernels.decode_topk) takes this exit instead of a scan.
    const bool no_suppression = d.iou_threshold >= 2.0f;
    if (no_suppression) {
        const int kn = n < d.max_predictions ? n : d.max_predictions;
        for (int t = tid; t < kn; t += NMS_THREADS) keep_list[t] = t;
        if (tid == 0) s_kept = kn;
        __syncthreads();
    } else if (MASK) {
        // ---- suppression as a triangular bit matrix, 64 candidates (one flag word) at a time: the 16 waves build the matrix rows of the
        // chunk's candidates that are still alive (a wave owns a row, a lane one column: 64 IoU tests per step, the word is their ballot),
        // then wave 0 walks the chunk without barriers.  Rows of candidates suppressed by earlier chunks are never built (about two thirds
        // of them at the recipe thresholds), and nothing past the max_predictions-th kept box is.
        const int nw = (n + 63) >> 6;  // flag words in use
        const int lane = tid & 63, wave = tid >> 6;
        for (int w = tid; w < NMS_MW; w += NMS_THREADS) rem[w] = 0;
        __syncthreads();
        u64 later = 0;  // wave 0, lane w: flags this chunk's kept boxes set in word w > chunk
        for (int c = 0; c < nw; ++c) {
            const u64 remc = rem[c];
            const int kept_in = s_kept;  // read on this side of the barriers: wave 0's lane 0 rewrites it at the end of its walk
            for (int r = wave; r < 64; r += NMS_THREADS / 64) {
                const int i = 64 * c + r;
                if (i >= n || ((remc >> r) & 1ull)) continue;  // wave-uniform
                float ci[4];
                nbox(i, ci);
                const float ai = area[i];
                const int ic = cls_s[i], base = nms_mask_row(i);
                for (int w = c; w < nw; ++w) {
                    const int t = 64 * w + lane;
                    const bool hit = t > i && t < n && (class_mode != 2 || cls_s[t] == ic) && suppresses(ci, ai, t);
                    const u64 bits = __ballot(hit);
                    if (lane == 0) mask[base + (w - c)] = bits;
                }
            }
            __syncthreads();
            if (wave == 0) {
                // the kept candidates of this word are the flags that are still clear - found with ffs, so suppressed ones cost nothing; every
                // kept candidate ORs its row into the flags (its own word through a same-address LDS read, the later words lane by lane)
                int kept = kept_in;
                u64 cur = remc;
                if (c == nw - 1 && (n & 63)) cur |= ~0ull << (n & 63);  // slots past the last candidate
                u64 avail = ~cur;
                while (avail && kept < d.max_predictions) {  // wave-uniform
                    const int bit = __ffsll(avail) - 1;
                    const int i = 64 * c + bit;
                    if (lane == 0) keep_list[kept] = i;
                    ++kept;
                    const int base = nms_mask_row(i);
                    cur |= mask[base];
                    if (lane > c && lane < nw) later |= mask[base + (lane - c)];
                    avail = ~cur & ~((2ull << bit) - 1ull);
                }
                if (lane > c && lane < nw) rem[lane] |= later;
                if (lane == 0) s_kept = kept;
            }
            __syncthreads();
            if (s_kept >= d.max_predictions) break;  // uniform
        }
    }
    // ---- greedy scan (top-k capacities above 1024: the bit matrix would not fit in LDS): one barrier pair per kept box ----
    for (int i = 0; i < ((no_suppression || MASK) ? 0 : n); ++i) {
        if (sup[i]) continue;  // uniform: flags only change before a barrier
        if (tid == 0) {
            float nb[4];
            nbox(i, nb);
            cur[0] = nb[0]; cur[1] = nb[1]; cur[2] = nb[2]; cur[3] = nb[3]; cur[4] = area[i];
            keep_list[s_kept] = i;
            s_kept = s_kept + 1;
        }
        __syncthreads();
        for (int t = tid; t < n; t += NMS_THREADS) {
            if (t > i && !sup[t] && (class_mode != 2 || cls_s[t] == cls_s[i]) && suppresses(cur, cur[4], t)) sup[t] = 1;
        }
        __syncthreads();
        if (s_kept >= d.max_predictions) break;  // uniform
    }
    __syncthreads();
    const int kept = s_kept < d.max_predictions ? s_kept : d.max_predictions;
    if (tid == 0) {
        out_count[b] = kept;
        if (num_candidates) num_candidates[b] = n;
    }
    for (int r = tid; r < d.max_predictions; r += NMS_THREADS) {
        float* o = out + ((long)b * d.max_predictions + r) * 6;
        if (r < kept) {
            int i = keep_list[r];
            u64 k = keys[i];
            unsigned e = ((1u << NMS_IDXBITS) - 1u) - (unsigned)(k & ((1u << NMS_IDXBITS) - 1u));
            o[0] = bx[i][0]; o[1] = bx[i][1]; o[2] = bx[i][2]; o[3] = bx[i][3];
            o[4] = __uint_as_float((unsigned)(k >> NMS_IDXBITS));
            o[5] = (float)cls_s[i];
            if (out_index) out_index[(long)b * d.max_predictions + r] = (int)e;
        } else {
            for (int q = 0; q < 6; ++q) o[q] = 0.f;
            if (out_index) out_index[(long)b * d.max_predictions + r] = -1;
        }
    }
}

// ---- split suppression (top-k <= 1024) ---------------------------------------------------------------------------------------------------
// nms_mask_kernel: Row i of the triangular matrix: bit j of word w - c = "i suppresses 64 w + j" for the words w >= c = i / 64; a wave owns
// a row, a lane one column, the word is the ballot of 64 IoU tests (the arithmetic order of torchvision's kernel, as above).  Every row is
// built (the in-kernel form skipped rows already suppressed: about three times the tests, on a chip that was 7/8 idle).
// Work items = (strip c of 64 rows, group g of NMS_MASK_WG words): 40 per image instead of one workgroup per strip - strip 0 alone was 16
// words x 64 rows on four waves (the r3z trace: 68 us per call, the longest kernel of the post-prediction call, bound by its longest
// workgroup); an item is at most 4 words x 64 rows = 64 ballots per wave, and stages only its own 64 rows and 256 columns.
#define NMS_MASK_THREADS 256
#define NMS_MASK_WG 4                                        // words per work item
#define NMS_MASK_ITEMS 40                                    // sum over strips c of ceil((NMS_MW - c) / NMS_MASK_WG) for NMS_MW = 16
__global__ __launch_bounds__(NMS_MASK_THREADS) void nms_mask_kernel(sgx_nms_desc d, char* split) {
    static_assert(NMS_MW == 16 && NMS_MASK_WG == 4, "NMS_MASK_ITEMS and the item table are written for 16 words in groups of 4");
    __shared__ float rnb[64][4], cnb[64 * NMS_MASK_WG][4];
    __shared__ float rarea[64], carea[64 * NMS_MASK_WG];
    __shared__ int rcls[64], ccls[64 * NMS_MASK_WG];
    // item -> (strip, group): strips 0-3 have 4 groups, 4-7 three, 8-11 two, 12-15 one
    int item = blockIdx.x, c, g;
    if (item < 16) { c = item >> 2; g = item & 3; }
    else if (item < 28) { c = 4 + (item - 16) / 3; g = (item - 16) % 3; }
    else if (item < 36) { c = 8 + ((item - 28) >> 1); g = (item - 28) & 1; }
    else { c = 12 + (item - 36); g = 0; }
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char* const o = split + (long)b * NMS_SPLIT_BYTES;
    const float* gnb = reinterpret_cast<const float*>(o + NMS_SPLIT_K * 8) + NMS_SPLIT_K * 4;
    const float* garea = gnb + NMS_SPLIT_K * 4;
    const int* gcls = reinterpret_cast<const int*>(garea + NMS_SPLIT_K);
    const int* meta = gcls + NMS_SPLIT_K;
    u64* const mask = reinterpret_cast<u64*>(o + NMS_CAND_BYTES);
    const int n = meta[0], class_mode = meta[1];
    const int nw = (n + 63) >> 6;
    const int w0 = c + NMS_MASK_WG * g;                                   // first word of the item
    if (64 * c >= n || w0 >= nw) return;                                 // whole workgroup
    const int w1 = w0 + NMS_MASK_WG < nw ? w0 + NMS_MASK_WG : nw;        // one past its last word
    if (tid < 64) {
        const int t = 64 * c + tid;
        if (t < n) {
            for (int q = 0; q < 4; ++q) rnb[tid][q] = gnb[t * 4 + q];
            rarea[tid] = garea[t];
            rcls[tid] = gcls[t];
        }
    }
    for (int j = tid; j < 64 * (w1 - w0); j += NMS_MASK_THREADS) {
        const int t = 64 * w0 + j;
        if (t < n) {
            for (int q = 0; q < 4; ++q) cnb[j][q] = gnb[t * 4 + q];
            carea[j] = garea[t];
            ccls[j] = gcls[t];
        }
    }
    __syncthreads();
    for (int r = wave; r < 64; r += NMS_MASK_THREADS / 64) {
        const int i = 64 * c + r;
        if (i >= n) break;  // wave-uniform
        const float ci0 = rnb[r][0], ci1 = rnb[r][1], ci2 = rnb[r][2], ci3 = rnb[r][3], ai = rarea[r];
        const int ic = rcls[r], base = nms_mask_row(i);
        for (int w = w0; w < w1; ++w) {
            const int j = 64 * (w - w0) + lane, t = 64 * w + lane;
            bool hit = false;
            if (t > i && t < n && (class_mode != 2 || ccls[j] == ic)) {
                const float xx1 = fmaxf(ci0, cnb[j][0]), yy1 = fmaxf(ci1, cnb[j][1]);
                const float xx2 = fminf(ci2, cnb[j][2]), yy2 = fminf(ci3, cnb[j][3]);
                float ww = xx2 - xx1; ww = ww < 0.f ? 0.f : ww;
                float hh = yy2 - yy1; hh = hh < 0.f ? 0.f : hh;
                const float inter = ww * hh;
                const float ovr = inter / (ai + carea[j] - inter);
                hit = ovr > d.iou_threshold;
            }
            const u64 bits = __ballot(hit);
            if (lane == 0) mask[base + (w - c)] = bits;
        }
    }
}
// nms_walk_kernel: one workgroup per image loads the matrix into LDS (68 KB, coalesced), ONE wave walks it - the kept candidates of a word
// are the flags that are still clear, found with ffs; every kept candidate ORs its row into the flags (its own word through a same-address
// LDS read, the later words lane by lane) - then the rows are written.
#define NMS_WALK_THREADS 256
__global__ __launch_bounds__(NMS_WALK_THREADS) void nms_walk_kernel(sgx_nms_desc d, const char* split, float* out, int* out_count, int* out_index,
                                                                    int* num_candidates) {
    __shared__ u64 mask[NMS_MASK_WORDS_1024];
    __shared__ int keep_list[NMS_SPLIT_K];
    __shared__ int s_kept;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const char* const o = split + (long)b * NMS_SPLIT_BYTES;
    const u64* keys = reinterpret_cast<const u64*>(o);
    const float* bx = reinterpret_cast<const float*>(o + NMS_SPLIT_K * 8);
    const int* cls = reinterpret_cast<const int*>(bx + 2 * NMS_SPLIT_K * 4 + NMS_SPLIT_K);
    const int* meta = cls + NMS_SPLIT_K;
    const u64* gmask = reinterpret_cast<const u64*>(o + NMS_CAND_BYTES);
    const int n = meta[0];
    const int nw = (n + 63) >> 6;
    // only the rows of existing candidates were written: strip g holds 64 rows of (16 - g) words
    const int used = n > 0 ? nms_mask_row(n - 1) + (NMS_MW - ((n - 1) >> 6)) : 0;
    // (eight 8-byte loads in flight per lane: written as `mask[q] = gmask[q]` the copy of the 68 KB was ~34 dependent round trips per lane)
    for (int q0 = 0; q0 < used; q0 += 8 * NMS_WALK_THREADS) {
        u64 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u * NMS_WALK_THREADS + tid;
            v[u] = q < used ? gmask[q] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u * NMS_WALK_THREADS + tid;
            if (q < used) mask[q] = v[u];
        }
    }
    __syncthreads();
    if (wave == 0) {
        int kept = 0;
        u64 rem = 0;  // lane w: suppression flags of word w
        for (int c = 0; c < nw && kept < d.max_predictions; ++c) {
            u64 cur = __shfl(rem, c);
            if (c == nw - 1 && (n & 63)) cur |= ~0ull << (n & 63);  // slots past the last candidate
            // the chunk's own words (row r of the chunk, word c) one per lane: the serial chain kept -> flags -> next kept then runs on
            // scalar reads of a register (two v_readlane), not on one LDS round trip per kept candidate
            const u64 diag = 64 * c + lane < n ? mask[nms_mask_row(64 * c + lane)] : 0ull;
            // The chain kept -> flags -> next kept on the SCALAR unit: the flags are wave-uniform, so they move to scalar registers once per
            // chunk and every step is s_ff1 / two v_readlane / a few 64-bit scalar ops (as vector code a step was ~25 dependent VALU
            // instructions: 300 kept candidates x ~320 cycles = the 45-50 us the kernel took whatever its memory side did, r3zf)
            u64 cur_s = sgx_uniform_u64(cur);
            u64 avail = ~cur_s;
            u64 kept_bits = 0;  // the chunk's kept candidates
            while (avail && kept < d.max_predictions) {  // wave-uniform
                const int bit = __ffsll(avail) - 1;
                if (lane == 0) keep_list[kept] = 64 * c + bit;
                ++kept;
                kept_bits |= 1ull << bit;
                cur_s |= sgx_readlane_u64(diag, bit);
                avail = ~cur_s & ~((2ull << bit) - 1ull);
            }
            // what the chunk's kept candidates suppress in the LATER words: lane w ORs word w of their rows - independent LDS reads after
            // the chain, not one read (and its wait) inside every step of it
            if (lane > c && lane < nw) {
                u64 later = 0;
                const int stride_w = NMS_MW - c, off = nms_mask_row(64 * c) + (lane - c);  // rows of a strip are (NMS_MW - c) words apart
                for (u64 kb = kept_bits; kb; kb &= kb - 1ull) later |= mask[off + (__ffsll(kb) - 1) * stride_w];
                rem |= later;
            }
        }
        if (lane == 0) s_kept = kept;
    }
    __syncthreads();
    const int kept = s_kept < d.max_predictions ? s_kept : d.max_predictions;
    if (tid == 0) {
        out_count[b] = kept;
        if (num_candidates) num_candidates[b] = n;
    }
    for (int r = tid; r < d.max_predictions; r += NMS_WALK_THREADS) {
        float* q = out + ((long)b * d.max_predictions + r) * 6;
        if (r < kept) {
            const int i = keep_list[r];
            const u64 k = keys[i];
            const unsigned e = ((1u << NMS_IDXBITS) - 1u) - (unsigned)(k & ((1u << NMS_IDXBITS) - 1u));
            q[0] = bx[i * 4 + 0]; q[1] = bx[i * 4 + 1]; q[2] = bx[i * 4 + 2]; q[3] = bx[i * 4 + 3];
            q[4] = __uint_as_float((unsigned)(k >> NMS_IDXBITS));
            q[5] = (float)cls[i];
            if (out_index) out_index[(long)b * d.max_predictions + r] = (int)e;
        } else {
            for (int z = 0; z < 6; ++z) q[z] = 0.f;
            if (out_index) out_index[(long)b * d.max_predictions + r] = -1;
        }
    }
}

extern "C" int32_t sgx_nms(const sgx_nms_desc* d, const float* boxes, const float* scores, float* out, int32_t* out_count, int32_t* out_index,
                           int32_t* num_candidates, void* ws, int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(d && boxes && scores && out && out_count, "nms: null pointer");
    SGX_CHECK_ARG(d->B > 0 && d->L > 0 && d->C > 0, "nms: bad dims");
    SGX_CHECK_ARG(d->nms_top_k > 0 && d->nms_top_k <= NMS_MAXK_LIMIT, "nms: nms_top_k=%d unsupported (max %d)", d->nms_top_k, NMS_MAXK_LIMIT);
    SGX_CHECK_ARG(d->max_predictions > 0 && d->max_predictions <= NMS_MAXK_LIMIT, "nms: bad max_predictions");
    SGX_CHECK_ARG((long)d->L * (d->multi_label ? d->C : 1) <= (1L << NMS_IDXBITS), "nms: too many candidates for the %d-bit index field", NMS_IDXBITS);
    SGX_CHECK_ARG(d->class_mode >= 0 && d->class_mode <= 3, "nms: bad class_mode");
    SGX_CHECK_ARG(d->score_threshold >= 0.f, "nms: negative score threshold unsupported (keys assume non-negative scores)");
    const int* wsi = nullptr;
    if (d->multi_label) {
        // stage 1 on the whole chip (a caller without a workspace gets the streaming stage 2: same rows, one workgroup per image)
        if (ws && ws_bytes >= sgx_nms_workspace(d)) {
            wsi = (const int*)ws;
            const long E = (long)d->L * d->C;
            const bool sampled = g_nms_sampled.load(std::memory_order_relaxed) && d->nms_top_k <= 2048 && E % 4 == 0 && ((uintptr_t)scores % 16) == 0 &&
                                 E >= 32L * NMS_SAMPLE_STEP * 8;  // (a sample of at least 8 lines; 3.2 k expected keys must fit the list)
            if (!sampled) SGX_MEMSET_ASYNC(ws, 0, (size_t)d->B * (2 * NMS_HBINS + NMS_CTR_INTS) * 4, stream);
            int S = (int)((E + 16383) / 16384);  // >= 16 k scores per workgroup, at most ~2048 workgroups in flight
            if (S * d->B > 2048) S = (2048 + d->B - 1) / d->B;
            if (S < 1) S = 1;
            const int slab = (int)((((E + S - 1) / S) + 3) / 4 * 4);
            const dim3 grid((unsigned)((E + slab - 1) / slab), (unsigned)d->B);
            if (sampled) {
                SGX_LAUNCH(nms_sample_kernel, dim3((unsigned)d->B), dim3(NMS_THREADS), 0, stream, *d, scores, (int*)ws);
                SGX_LAUNCH(nms_append_kernel, grid, dim3(NMS_S1_THREADS), 0, stream, *d, scores, (int*)ws, slab);
            } else {
                SGX_LAUNCH(nms_select_kernel<0>, grid, dim3(NMS_S1_THREADS), 0, stream, *d, scores, (int*)ws, slab);
                SGX_LAUNCH(nms_select_kernel<1>, grid, dim3(NMS_S1_THREADS), 0, stream, *d, scores, (int*)ws, slab);
                SGX_LAUNCH(nms_select_kernel<2>, grid, dim3(NMS_S1_THREADS), 0, stream, *d, scores, (int*)ws, slab);
            }
            SGX_CHECK_LAUNCH("nms_select");
        }
    }
    const int need = d->nms_top_k > d->max_predictions ? d->nms_top_k : d->max_predictions;
    // split suppression (matrix build on the whole chip): needs the workspace; sgx_debug_set_nms_split(0) keeps everything in nms_kernel
    char* split = (wsi && need <= 1024 && d->iou_threshold < 2.0f && g_nms_split.load(std::memory_order_relaxed)) ? (char*)ws + nms_ws_head(d) + 256 - ((nms_ws_head(d) + 256) & 255) : nullptr;
    if (need <= 1024) SGX_LAUNCH(nms_kernel<1024>, dim3(d->B), dim3(NMS_THREADS), 0, stream, *d, boxes, scores, out, out_count, out_index, num_candidates, wsi, split);
    else if (need <= 2048) SGX_LAUNCH(nms_kernel<2048>, dim3(d->B), dim3(NMS_THREADS), 0, stream, *d, boxes, scores, out, out_count, out_index, num_candidates, wsi, (char*)nullptr);
    else SGX_LAUNCH(nms_kernel<4096>, dim3(d->B), dim3(NMS_THREADS), 0, stream, *d, boxes, scores, out, out_count, out_index, num_candidates, wsi, (char*)nullptr);
    if (split) {
        SGX_LAUNCH(nms_mask_kernel, dim3(NMS_MASK_ITEMS, (unsigned)d->B), dim3(NMS_MASK_THREADS), 0, stream, *d, split);
        SGX_LAUNCH(nms_walk_kernel, dim3(d->B), dim3(NMS_WALK_THREADS), 0, stream, *d, (const char*)split, out, out_count, out_index, num_candidates);
    }
    SGX_CHECK_LAUNCH("nms");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Detection matching for the validation metrics (mAP): predictions (NMS rows) vs ground truth, per image and IoU threshold.
// Replaces compute_detection_matching / compute_img_detection_matching / IoUMatching.compute_targets / compute_crowd_targets /
// get_top_k_idx_per_cls (training/utils/detection_utils.py:1120-1290, 880-1005, 1342-1358), which the reference runs as a Python
// loop over images with a Python loop over candidate (prediction, target) pairs inside.
// One workgroup per image.  Per IoU threshold j the reference's rule reduces to an independent greedy pass: predictions in
// (score desc, index asc) order, restricted to the top_k of their class; each takes the free same-class target of highest IoU
// (first index among equals: stable descending sort) and is a true positive iff that IoU > thr[j] (and > thr[0], the reference's
// candidate filter).  Crowd targets: a used prediction is ignored at threshold j iff its best same-class IoA (intersection over
// detection area) > thr[j]; predictions outside the per-class top_k are ignored at every threshold.
// Arithmetic order follows box_iou / crowd_ioa (:257-276, :797-810) and cxcywh2xyxy (:725-736); compiled with -ffp-contract=off.
// ---------------------------------------------------------------------------------------------------------------------
#define MATCH_THREADS 256
__device__ __forceinline__ float match_iou(const float* p, const float* t) {
    const float area1 = (p[2] - p[0]) * (p[3] - p[1]);
    const float area2 = (t[2] - t[0]) * (t[3] - t[1]);
    float w = fminf(p[2], t[2]) - fmaxf(p[0], t[0]);
    float h = fminf(p[3], t[3]) - fmaxf(p[1], t[1]);
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    return inter / (area1 + area2 - inter);
}
__device__ __forceinline__ void match_load_target(const float* t, int denorm, float W, float H, float* box, float* cls) {
    // row = (img, cls, cx, cy, w, h);  y1 = cy - h*0.5; x1 = cx - w*0.5; y2 = h + y1; x2 = w + x1  (then optional de-normalisation)
    *cls = t[1];
    const float y1 = t[3] - t[5] * 0.5f, x1 = t[2] - t[4] * 0.5f;
    float b[4] = {x1, y1, t[4] + x1, t[5] + y1};
    if (denorm) {
        b[0] *= W; b[2] *= W; b[1] *= H; b[3] *= H;
    }
    box[0] = b[0]; box[1] = b[1]; box[2] = b[2]; box[3] = b[3];
}
__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(sgx_match_desc d, const float* preds, const int* pred_count, const float* targets,
                                                              const int* gt_count, const int* gt_index, const float* crowd, const int* crowd_count,
                                                              const int* crowd_index, const float* thr, unsigned char* matched,
                                                              unsigned char* ignore) {
    SGX_DYN_SMEM(float, sm);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int P = d.P, nthr = d.nthr;
    int n = pred_count[b];
    n = n < P ? n : P;
    const int nt = d.nmax > 0 ? min(gt_count[b], d.nmax) : 0;
    const int nc = d.cmax > 0 ? min(crowd_count[b], d.cmax) : 0;
    float* pbox = sm;                        // [P][4]
    float* pscore = pbox + (size_t)P * 4;    // [P]
    float* pcls = pscore + P;                // [P]
    float* tbox = pcls + P;                  // [nmax][4]
    float* tcls = tbox + (size_t)d.nmax * 4; // [nmax]
    float* cbox = tcls + d.nmax;             // [cmax][4]
    float* ccls = cbox + (size_t)d.cmax * 4; // [cmax]
    int* order = (int*)(ccls + d.cmax);      // [P]
    unsigned char* used = (unsigned char*)(order + P);      // [P]
    unsigned char* tmat = used + P;                          // [nthr][nmax]
    const float Wf = (float)d.W, Hf = (float)d.H;
    const bool clip = nt > 0 || nc > 0;  // the reference clips the predictions only when there is something to match (:1262-1264)
    for (int i = tid; i < n; i += MATCH_THREADS) {
        const float* r = preds + ((size_t)b * P + i) * 6;
        float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        if (clip) {
            x1 = fminf(fmaxf(x1, 0.f), Wf); x2 = fminf(fmaxf(x2, 0.f), Wf);
            y1 = fminf(fmaxf(y1, 0.f), Hf); y2 = fminf(fmaxf(y2, 0.f), Hf);
        }
        pbox[i * 4 + 0] = x1; pbox[i * 4 + 1] = y1; pbox[i * 4 + 2] = x2; pbox[i * 4 + 3] = y2;
        pscore[i] = r[4];
        pcls[i] = r[5];
    }
    for (int t = tid; t < nt; t += MATCH_THREADS) match_load_target(targets + (size_t)gt_index[(size_t)b * d.nmax + t] * 6, d.denormalize, Wf, Hf, tbox + t * 4, tcls + t);
    for (int t = tid; t < nc; t += MATCH_THREADS) match_load_target(crowd + (size_t)crowd_index[(size_t)b * d.cmax + t] * 6, d.denormalize, Wf, Hf, cbox + t * 4, ccls + t);
    for (int i = tid; i < nthr * d.nmax; i += MATCH_THREADS) tmat[i] = 0;
    __syncthreads();
    // global order (score desc, index asc) and membership in the per-class top_k
    for (int i = tid; i < n; i += MATCH_THREADS) {
        const float s = pscore[i], c = pcls[i];
        int grank = 0, crank = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = pscore[j];
            const bool before = sj > s || (sj == s && j < i);
            grank += before ? 1 : 0;
            crank += (before && pcls[j] == c) ? 1 : 0;
        }
        order[grank] = i;
        used[i] = (crank < d.top_k && s != 0.f) ? 1 : 0;  // zero scores drop out of the reference's nonzero() selection
    }
    __syncthreads();
    // one greedy pass per threshold
    if (tid < nthr) {
        const int j = tid;
        const float tj = thr[j], t0 = thr[0];
        unsigned char* free_t = tmat + (size_t)j * d.nmax;
        for (int r = 0; r < n; ++r) {
            const int i = order[r];
            unsigned char m = 0;
            if (used[i] && nt > 0) {
                float best = -1.f;
                int bi = -1;
                const float c = pcls[i];
                for (int t = 0; t < nt; ++t) {
                    if (tcls[t] != c || free_t[t]) continue;
                    const float v = match_iou(pbox + i * 4, tbox + t * 4);
                    if (v > best) {
                        best = v;
                        bi = t;
                    }
                }
                if (bi >= 0 && best > t0 && best > tj) {
                    free_t[bi] = 1;
                    m = 1;
                }
            }
            matched[((size_t)b * P + i) * nthr + j] = m;
        }
    }
    // crowd targets and the top_k rule -> ignore flags
    for (int i = tid; i < n; i += MATCH_THREADS) {
        float best = 0.f;
        bool any = false;
        if (used[i] && nc > 0) {
            const float* pb = pbox + i * 4;
            const float det_area = (pb[2] - pb[0]) * (pb[3] - pb[1]);
            for (int t = 0; t < nc; ++t) {
                float v = 0.f;
                if (ccls[t] == pcls[i]) {
                    float w = fminf(pb[2], cbox[t * 4 + 2]) - fmaxf(pb[0], cbox[t * 4 + 0]);
                    float h = fminf(pb[3], cbox[t * 4 + 3]) - fmaxf(pb[1], cbox[t * 4 + 1]);
                    w = w < 0.f ? 0.f : w;
                    h = h < 0.f ? 0.f : h;
                    v = (w * h) / det_area;
                }
                if (!any || v > best) best = v;
                any = true;
            }
        }
        for (int j = 0; j < nthr; ++j) ignore[((size_t)b * P + i) * nthr + j] = (!used[i] || (any && best > thr[j])) ? 1 : 0;
    }
    for (int i = n + tid; i < P; i += MATCH_THREADS)
        for (int j = 0; j < nthr; ++j) {
            matched[((size_t)b * P + i) * nthr + j] = 0;
            ignore[((size_t)b * P + i) * nthr + j] = 1;
        }
}
static size_t match_smem(const sgx_match_desc* d) {
    return ((size_t)d->P * 6 + (size_t)d->nmax * 5 + (size_t)d->cmax * 5) * 4 + (size_t)d->P * 4 + (size_t)d->P + (size_t)d->nthr * d->nmax + 64;
}
extern "C" int32_t sgx_detection_match(const sgx_match_desc* d, const float* preds, const int32_t* pred_count, const float* targets,
                                       const int32_t* gt_count, const int32_t* gt_index, const float* crowd, const int32_t* crowd_count,
                                       const int32_t* crowd_index, const float* thresholds, uint8_t* matched, uint8_t* ignore, void* stream) {
    SGX_CHECK_ARG(d && preds && pred_count && thresholds && matched && ignore, "detection_match: null pointer");
    SGX_CHECK_ARG(d->B > 0 && d->P > 0 && d->nthr > 0 && d->nthr <= MATCH_THREADS && d->top_k > 0, "detection_match: bad dims");
    SGX_CHECK_ARG(d->nmax == 0 || (targets && gt_count && gt_index), "detection_match: null targets");
    SGX_CHECK_ARG(d->cmax == 0 || (crowd && crowd_count && crowd_index), "detection_match: null crowd targets");
    const size_t smem = match_smem(d);
    if (smem > 160 * 1024) SGX_FAIL(SGX_ERR_UNSUPPORTED, "detection_match: %zu bytes of LDS needed (P=%d, targets %d, crowd %d)", smem, d->P, d->nmax, d->cmax);
#ifndef SGX_EMU
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) SGX_FAIL(SGX_ERR_HIP, "detection_match: cannot reserve %zu bytes of LDS: %s", smem, hipGetErrorString(e));
    }
#endif
    SGX_LAUNCH(match_kernel, dim3(d->B), dim3(MATCH_THREADS), smem, stream, *d, preds, pred_count, targets, gt_count, gt_index, crowd, crowd_count,
               crowd_index, thresholds, matched, ignore);
    SGX_CHECK_LAUNCH("detection_match");
    return SGX_OK;
}

// ------------------------------------------------------------------------------------------------
// predict(): the inverse box maps of the image processing and the packing of a batch's detections into ONE host-bound buffer (round 6).
// The reference maps every image's boxes back through its processing stages on the host, one numpy pass per stage per image
// (training/processing/processing.py:361-364 shift by the padding, :401-403 multiply by 1 / scale factor; pipelines.py:222-247 loops over the
// images).  Here: one launch for the batch - per image a short list of (kind, a_x, a_y) steps applied IN ORDER to x1, y1, x2, y2 in fp32
// (kind 0: += a, kind 1: *= a - one rounding each, as numpy's float32 arithmetic rounds them; this file is compiled without fma
// contraction) - and the rows of every image, followed by the B counts (int32 bit patterns), land in one contiguous fp32 buffer: one
// device-to-host copy per batch instead of a count copy + a concatenation + a row copy.
// ------------------------------------------------------------------------------------------------
__global__ void boxes_unmap_kernel(const float* rows, const int* counts, int B, int P, const float* steps, int nsteps, float* out) {
    const int b = blockIdx.y;
    const int n = counts[b] < P ? counts[b] : P;
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int*>(out + (size_t)B * P * 6)[b] = n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float* o = out + ((size_t)b * P + i) * 6;
    if (i >= n) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = 0.f;
        return;
    }
    const float* r = rows + ((size_t)b * P + i) * 6;
    float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
    const float* st = steps + (size_t)b * nsteps * 3;
    for (int s = 0; s < nsteps; ++s) {
        const float kind = st[3 * s], ax = st[3 * s + 1], ay = st[3 * s + 2];
        if (kind == 0.f) {
            x1 += ax; x2 += ax; y1 += ay; y2 += ay;
        } else if (kind == 1.f) {
            x1 *= ax; x2 *= ax; y1 *= ay; y2 *= ay;
        }  // (kind 2: no step - padding of a shorter list)
    }
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = r[4]; o[5] = r[5];
}
extern "C" int32_t sgx_detection_unmap(const float* rows, const int32_t* counts, int32_t B, int32_t P, const float* steps, int32_t nsteps, float* out,
                                       void* stream) {
    SGX_CHECK_ARG(rows && counts && out && (steps || nsteps == 0), "detection_unmap: null pointer");
    SGX_CHECK_ARG(B > 0 && P > 0 && nsteps >= 0 && nsteps <= 64, "detection_unmap: bad dims (B=%d P=%d nsteps=%d)", B, P, nsteps);
    SGX_LAUNCH(boxes_unmap_kernel, dim3((unsigned)((P + 127) / 128), (unsigned)B), dim3(128), 0, stream, rows, counts, B, P, steps, nsteps, out);
    SGX_CHECK_LAUNCH("detection_unmap");
    return SGX_OK;
}

// ------------------------------------------------------------------------------------------------
// Sliding-window inference: the cross-tile merge (sliding_window_detection_forward_wrapper.py:113-133).
// The reference shifts every tile's post-NMS rows by the tile's origin (:116, one fp32 add per coordinate), concatenates them per image on
// the host (:122) and calls torchvision.ops.batched_nms once per image (:127) - always per class, whatever the tile stage did, and without a
// max_predictions cut (:131).  Here the whole batch stays on the device:
//   merge_collect_kernel  one workgroup per image: prefix sum of the tile counts, the valid rows in the order tile 0 .. T-1 / row 0 .. count-1
//                         (the "merged index"), boxes shifted, composite keys (score, merged index), the image's max coordinate
//   merge_rank_kernel     whole chip: a candidate's place in the (score desc, merged index asc) order is the number of larger keys - keys are
//                         unique, so the ranks are a permutation; no LDS capacity bounds the count (the per-image kernel above sorts <= 4096
//                         keys in LDS).  Writes the sorted candidates as the IoU test sees them: torchvision's CPU dispatch, the coordinate-
//                         offset form while 4 n <= 4000 (max_coordinate over THIS image's merged, shifted boxes), the per-class form above.
//   merge_mask_kernel     whole chip: the suppression bit matrix (row i, word w: "i suppresses 64 w + j"), the wave-ballot form of
//                         nms_mask_kernel, in HBM - n^2 / 8 bytes per image
//   merge_walk_kernel     one workgroup per image, thread w owns flag word w: 64 candidates at a time, the kept -> flags -> next kept chain
//                         of a word on the scalar unit (as nms_walk_kernel), then every thread ORs the rows of the word's kept candidates
//                         into its own flag word (loads of one round in flight together); rows written in kept order, no cut.
// Exact for any merged count up to SGX_TILE_MERGE_MAX_ROWS (a bound on T * P: the counts are device data); no host fallback.
// ------------------------------------------------------------------------------------------------
#define MERGE_THREADS 1024
#define MERGE_RANK_THREADS 256
#define MERGE_MASK_THREADS 256
#define MERGE_MASK_WG 4
#define MERGE_WALK_THREADS (SGX_TILE_MERGE_MAX_ROWS / 64)
static_assert(MERGE_WALK_THREADS == 256, "merge_walk_kernel: one flag word per thread of a 256-thread workgroup");
// an image's block of the workspace (byte offsets; rows = T * P rounded up to 64, so every array starts on a 256-byte line):
// meta int[64] {n, class mode, max coordinate bits} | key u64[rows] | box f32[rows][4] | cls f32[rows] | src int[rows] (unsorted, merged
// order) | sbox f32[rows][4] | snb f32[rows][4] (as the IoU test sees it) | sarea f32[rows] | scls f32[rows] | ssrc int[rows] (sorted) |
// mask u64[rows][rows / 64]
struct merge_layout {
    long per_image, key, box, cls, src, sbox, snb, sarea, scls, ssrc, mask;
    int rows, nws;
};
static merge_layout merge_make_layout(long TP) {
    merge_layout L;
    const long R = (TP + 63) / 64 * 64;
    L.rows = (int)R;
    L.nws = (int)(R / 64);
    long o = 256;
    L.key = o; o += R * 8;
    L.box = o; o += R * 16;
    L.cls = o; o += R * 4;
    L.src = o; o += R * 4;
    L.sbox = o; o += R * 16;
    L.snb = o; o += R * 16;
    L.sarea = o; o += R * 4;
    L.scls = o; o += R * 4;
    L.ssrc = o; o += R * 4;
    L.mask = o; o += R * L.nws * 8;
    L.per_image = o;
    return L;
}
// float bits whose unsigned order is the floats' order (-0 counts as +0: equal scores tie on the index)
__device__ __forceinline__ unsigned merge_score_bits(float s) {
    if (s == 0.f) s = 0.f;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int merge_tile_count(const int* cnt, int t, int P) {
    const int c = cnt[t];
    return c < 0 ? 0 : (c > P ? P : c);
}
__global__ __launch_bounds__(MERGE_THREADS) void merge_collect_kernel(const float* rows, const int* counts, const int* origins, int T, int P, merge_layout L,
                                                                      char* ws) {
    __shared__ int tbase[SGX_TILE_MERGE_MAX_ROWS];  // (T <= T * P <= SGX_TILE_MERGE_MAX_ROWS)
    __shared__ float wmax[MERGE_THREADS / 64];
    __shared__ int s_n;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    char* const o = ws + (long)b * L.per_image;
    int* meta = reinterpret_cast<int*>(o);
    u64* key = reinterpret_cast<u64*>(o + L.key);
    float* box = reinterpret_cast<float*>(o + L.box);
    float* cls = reinterpret_cast<float*>(o + L.cls);
    int* src = reinterpret_cast<int*>(o + L.src);
    const int* cnt = counts + (long)b * T;
    if (tid < 64) {  // wave 0: exclusive prefix sum of the tile counts, 64 tiles per trip
        int carry = 0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            const int c = t < T ? merge_tile_count(cnt, t, P) : 0;
            int v = c;
            for (int off = 1; off < 64; off <<= 1) {
                const int u = __shfl_up(v, off);
                if (lane >= off) v += u;
            }
            if (t < T) tbase[t] = carry + v - c;
            carry += __shfl(v, 63);
        }
        if (lane == 0) s_n = carry;
    }
    __syncthreads();
    const int n = s_n;
    const long TP = (long)T * P;
    float mymax = -INFINITY;
    for (long s = tid; s < TP; s += MERGE_THREADS) {
        const int t = (int)(s / P), r = (int)(s - (long)t * P);
        if (r >= merge_tile_count(cnt, t, P)) continue;
        const int m = tbase[t] + r;
        const float* row = rows + ((long)b * TP + s) * 6;
        const float fx = (float)origins[2 * t], fy = (float)origins[2 * t + 1];
        const float x1 = row[0] + fx, y1 = row[1] + fy, x2 = row[2] + fx, y2 = row[3] + fy;
        box[m * 4 + 0] = x1; box[m * 4 + 1] = y1; box[m * 4 + 2] = x2; box[m * 4 + 3] = y2;
        cls[m] = row[5];
        src[m] = (int)s;
        key[m] = ((u64)merge_score_bits(row[4]) << 32) | (u64)(0xffffffffu - (unsigned)m);
        mymax = fmaxf(fmaxf(fmaxf(mymax, x1), fmaxf(y1, x2)), y2);
    }
    for (int off = 32; off > 0; off >>= 1) mymax = fmaxf(mymax, __shfl_xor(mymax, off));
    if (lane == 0) wmax[tid >> 6] = mymax;
    __syncthreads();
    if (tid == 0) {
        float m = wmax[0];
        for (int w = 1; w < MERGE_THREADS / 64; ++w) m = fmaxf(m, wmax[w]);
        meta[0] = n;
        meta[1] = 4L * n > 4000 ? 2 : 1;  // torchvision/ops/boxes.py batched_nms on CPU: the coordinate trick while boxes.numel() <= 4000
        meta[2] = (int)__float_as_uint(m);
    }
}
__global__ __launch_bounds__(MERGE_RANK_THREADS) void merge_rank_kernel(merge_layout L, char* ws) {
    __shared__ u64 tk[MERGE_RANK_THREADS];
    const int b = blockIdx.y, tid = threadIdx.x;
    char* const o = ws + (long)b * L.per_image;
    const int* meta = reinterpret_cast<const int*>(o);
    const int n = meta[0], class_mode = meta[1];
    if ((int)blockIdx.x * MERGE_RANK_THREADS >= n) return;  // whole workgroup
    const u64* key = reinterpret_cast<const u64*>(o + L.key);
    const int i = blockIdx.x * MERGE_RANK_THREADS + tid;
    const u64 my = i < n ? key[i] : ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += MERGE_RANK_THREADS) {
        tk[tid] = j0 + tid < n ? key[j0 + tid] : 0ull;  // (0 is below every real key: their index field is never 0)
        __syncthreads();
        const int lim = n - j0 < MERGE_RANK_THREADS ? n - j0 : MERGE_RANK_THREADS;
        for (int j = 0; j < lim; ++j) rank += tk[j] > my ? 1 : 0;
        __syncthreads();
    }
    if (i >= n) return;
    const float* box = reinterpret_cast<const float*>(o + L.box);
    const float c = reinterpret_cast<const float*>(o + L.cls)[i];
    float* sbox = reinterpret_cast<float*>(o + L.sbox);
    float* snb = reinterpret_cast<float*>(o + L.snb);
    // boxes + idxs.to(boxes) * (max_coordinate + 1) (boxes.py), or the boxes themselves in the per-class form
    const float offv = class_mode == 1 ? c * (__uint_as_float((unsigned)meta[2]) + 1.f) : 0.f;
    float nb[4];
    for (int q = 0; q < 4; ++q) {
        const float v = box[i * 4 + q];
        sbox[rank * 4 + q] = v;
        nb[q] = v + offv;
        snb[rank * 4 + q] = nb[q];
    }
    reinterpret_cast<float*>(o + L.sarea)[rank] = (nb[2] - nb[0]) * (nb[3] - nb[1]);
    reinterpret_cast<float*>(o + L.scls)[rank] = c;
    reinterpret_cast<int*>(o + L.ssrc)[rank] = reinterpret_cast<const int*>(o + L.src)[i];
}
// work item = (strip c of 64 rows, group g of MERGE_MASK_WG words); words left of the strip's diagonal are never read and not built
__global__ __launch_bounds__(MERGE_MASK_THREADS) void merge_mask_kernel(merge_layout L, char* ws, float iou_threshold, int ngroups) {
    __shared__ float rnb[64][4], cnb[64 * MERGE_MASK_WG][4];
    __shared__ float rarea[64], carea[64 * MERGE_MASK_WG], rcls[64], ccls[64 * MERGE_MASK_WG];
    const int c = blockIdx.x / ngroups, g = blockIdx.x - c * ngroups;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char* const o = ws + (long)b * L.per_image;
    const int* meta = reinterpret_cast<const int*>(o);
    const int n = meta[0], class_mode = meta[1];
    const int nw = (n + 63) >> 6;
    const int w0 = MERGE_MASK_WG * g;
    const int w1 = w0 + MERGE_MASK_WG < nw ? w0 + MERGE_MASK_WG : nw;
    if (64 * c >= n || w0 >= nw || w1 <= c) return;  // whole workgroup
    const float* gnb = reinterpret_cast<const float*>(o + L.snb);
    const float* garea = reinterpret_cast<const float*>(o + L.sarea);
    const float* gcls = reinterpret_cast<const float*>(o + L.scls);
    u64* const mask = reinterpret_cast<u64*>(o + L.mask);
    if (tid < 64) {
        const int t = 64 * c + tid;
        if (t < n) {
            for (int q = 0; q < 4; ++q) rnb[tid][q] = gnb[t * 4 + q];
            rarea[tid] = garea[t];
            rcls[tid] = gcls[t];
        }
    }
    for (int j = tid; j < 64 * (w1 - w0); j += MERGE_MASK_THREADS) {
        const int t = 64 * w0 + j;
        if (t < n) {
            for (int q = 0; q < 4; ++q) cnb[j][q] = gnb[t * 4 + q];
            carea[j] = garea[t];
            ccls[j] = gcls[t];
        }
    }
    __syncthreads();
    for (int r = wave; r < 64; r += MERGE_MASK_THREADS / 64) {
        const int i = 64 * c + r;
        if (i >= n) break;  // wave-uniform
        const float ci0 = rnb[r][0], ci1 = rnb[r][1], ci2 = rnb[r][2], ci3 = rnb[r][3], ai = rarea[r], ic = rcls[r];
        for (int w = w0 > c ? w0 : c; w < w1; ++w) {
            const int j = 64 * (w - w0) + lane, t = 64 * w + lane;
            bool hit = false;
            if (t > i && t < n && (class_mode != 2 || ccls[j] == ic)) {
                const float xx1 = fmaxf(ci0, cnb[j][0]), yy1 = fmaxf(ci1, cnb[j][1]);
                const float xx2 = fminf(ci2, cnb[j][2]), yy2 = fminf(ci3, cnb[j][3]);
                float ww = xx2 - xx1; ww = ww < 0.f ? 0.f : ww;
                float hh = yy2 - yy1; hh = hh < 0.f ? 0.f : hh;
                const float inter = ww * hh;
                const float ovr = inter / (ai + carea[j] - inter);
                hit = ovr > iou_threshold;
            }
            const u64 bits = __ballot(hit);
            if (lane == 0) mask[(long)i * L.nws + w] = bits;
        }
    }
}
__global__ __launch_bounds__(MERGE_WALK_THREADS) void merge_walk_kernel(const float* rows, int T, int P, merge_layout L, const char* ws, float* out,
                                                                        int* out_count) {
    __shared__ int keep_list[SGX_TILE_MERGE_MAX_ROWS];
    __shared__ u64 s_cur, s_kept_bits;
    __shared__ int s_kept;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const char* const o = ws + (long)b * L.per_image;
    const int n = reinterpret_cast<const int*>(o)[0];
    const int nw = (n + 63) >> 6;
    const long nws = L.nws;
    const u64* mask = reinterpret_cast<const u64*>(o + L.mask);
    u64 rem = 0;   // thread w: the suppression flags of word w
    int kept = 0;  // (wave 0)
    for (int c = 0; c < nw; ++c) {
        if (tid == c) s_cur = rem;
        __syncthreads();
        if (wave == 0) {
            u64 cur = s_cur;
            if (c == nw - 1 && (n & 63)) cur |= ~0ull << (n & 63);  // slots past the last candidate
            const u64 diag = 64 * c + lane < n ? mask[(long)(64 * c + lane) * nws + c] : 0ull;
            u64 cur_s = sgx_uniform_u64(cur);
            u64 avail = ~cur_s, kept_bits = 0;
            while (avail) {  // wave-uniform
                const int bit = __ffsll(avail) - 1;
                if (lane == 0) keep_list[kept] = 64 * c + bit;
                ++kept;
                kept_bits |= 1ull << bit;
                cur_s |= sgx_readlane_u64(diag, bit);
                avail = ~cur_s & ~((2ull << bit) - 1ull);
            }
            if (lane == 0) s_kept_bits = kept_bits;
        }
        __syncthreads();
        if (tid > c && tid < nw) {
            // what the word's kept candidates suppress in this thread's word: eight independent loads per trip
            const u64* col = mask + (long)64 * c * nws + tid;
            u64 kb = s_kept_bits;
            while (kb) {
                int bit[8];
                u64 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    bit[u] = kb ? __ffsll(kb) - 1 : -1;
                    kb &= kb - 1ull;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = bit[u] >= 0 ? col[bit[u] * nws] : 0ull;
#pragma unroll
                for (int u = 0; u < 8; ++u) rem |= v[u];
            }
        }
    }
    if (tid == 0) s_kept = kept;
    __syncthreads();
    kept = s_kept;
    if (tid == 0) out_count[b] = kept;
    const float* sbox = reinterpret_cast<const float*>(o + L.sbox);
    const int* ssrc = reinterpret_cast<const int*>(o + L.ssrc);
    const long TP = (long)T * P;
    for (long r = tid; r < TP; r += MERGE_WALK_THREADS) {
        float* q = out + ((long)b * TP + r) * 6;
        if (r < kept) {
            const int i = keep_list[r];
            const float* row = rows + ((long)b * TP + ssrc[i]) * 6;
            q[0] = sbox[i * 4 + 0]; q[1] = sbox[i * 4 + 1]; q[2] = sbox[i * 4 + 2]; q[3] = sbox[i * 4 + 3];
            q[4] = row[4];
            q[5] = row[5];
        } else {
            for (int z = 0; z < 6; ++z) q[z] = 0.f;
        }
    }
}
static bool merge_dims_ok(int B, int T, int P) { return B > 0 && B <= 65535 && T > 0 && P > 0 && (long)T * P <= SGX_TILE_MERGE_MAX_ROWS; }
extern "C" int64_t sgx_tile_merge_workspace(int32_t B, int32_t T, int32_t P) {
    if (!merge_dims_ok(B, T, P)) return 256;
    return (int64_t)B * merge_make_layout((long)T * P).per_image;
}
extern "C" int32_t sgx_tile_merge(const float* rows, const int32_t* counts, const int32_t* origins, int32_t B, int32_t T, int32_t P, float iou_threshold,
                                  float* out, int32_t* out_count, void* ws, int64_t ws_bytes, void* stream) {
    SGX_CHECK_ARG(rows && counts && origins && out && out_count, "tile_merge: null pointer");
    SGX_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && P > 0, "tile_merge: bad dims (B=%d T=%d P=%d)", B, T, P);
    SGX_CHECK_ARG((long)T * P <= SGX_TILE_MERGE_MAX_ROWS, "tile_merge: %d tiles x %d rows = %ld merged rows per image, the limit is %d", T, P, (long)T * P,
                  SGX_TILE_MERGE_MAX_ROWS);
    if (!ws || ws_bytes < sgx_tile_merge_workspace(B, T, P) || ((uintptr_t)ws % 16) != 0)
        SGX_FAIL(SGX_ERR_WORKSPACE, "tile_merge: a 16-byte aligned workspace of %ld bytes is needed (got %ld)", (long)sgx_tile_merge_workspace(B, T, P), (long)ws_bytes);
    const merge_layout L = merge_make_layout((long)T * P);
    const int ngroups = (L.nws + MERGE_MASK_WG - 1) / MERGE_MASK_WG;
    SGX_LAUNCH(merge_collect_kernel, dim3((unsigned)B), dim3(MERGE_THREADS), 0, stream, rows, counts, origins, T, P, L, (char*)ws);
    SGX_LAUNCH(merge_rank_kernel, dim3((unsigned)(L.rows / MERGE_RANK_THREADS + (L.rows % MERGE_RANK_THREADS ? 1 : 0)), (unsigned)B), dim3(MERGE_RANK_THREADS), 0,
               stream, L, (char*)ws);
    SGX_LAUNCH(merge_mask_kernel, dim3((unsigned)(L.nws * ngroups), (unsigned)B), dim3(MERGE_MASK_THREADS), 0, stream, L, (char*)ws, iou_threshold, ngroups);
    SGX_LAUNCH(merge_walk_kernel, dim3((unsigned)B), dim3(MERGE_WALK_THREADS), 0, stream, rows, T, P, L, (const char*)ws, out, out_count);
    SGX_CHECK_LAUNCH("tile_merge");
    return SGX_OK;
}
