// Optimizer and EMA steps over flat fp32 arenas: one HBM-bound launch per arena instead of the reference's
// ~500 (AdamW foreach) / 921x3 (ModelEMA.update, training/utils/ema.py:139-141) tiny ATen kernels.
// AdamW follows torch.optim.AdamW (decoupled weight decay, bias correction, eps added after sqrt):
//   p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;
//   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// SGD follows torch.optim.SGD (coupled weight decay, momentum buffer initialised with the first gradient).
// Per-segment weight decay reproduces the zero-WD groups of optimizer_utils.py:32-59.
#include "sgx_common.h"

// first segment whose end is beyond i (segments ascend): binary search, ~9 L1-resident probes for a 500-tensor model
__device__ __forceinline__ float seg_wd_of(long i, const long long* seg_end, const float* seg_wd, int nseg) {
    int lo = 0, hi = nseg;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (i < (long)seg_end[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo < nseg ? seg_wd[lo] : 0.f;
}

__device__ __forceinline__ void adamw_one(float& pi, float gi, float& mi, float& vi, float wd, float lr, float b1, float b2, float eps, float bc1, float bc2s) {
    pi = pi * (1.f - lr * wd);
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    pi -= (lr / bc1) * (mi / denom);
}
// Four elements per lane (16-byte accesses) and ONE segment search per four: the per-element form spent nine dependent L1 probes per
// element on the weight-decay lookup and moved 4 bytes per memory instruction - 133 us for the 12.9 M parameters of YOLO-NAS-S (r5m),
// 2.7 TB/s.  A group of four that straddles a segment end looks every element up by itself.  Same arithmetic per element.
__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float bc1, float bc2s,
                             const long long* seg_end, const float* seg_wd, int nseg, const float* grad_scale) {
    const float gs = grad_scale ? grad_scale[0] : 1.f;
    const long n4 = n / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        float4 P = sgx_ld4(p + i), G = sgx_ld4(g + i), M = sgx_ld4(m + i), V = sgx_ld4(v + i);
        int lo = 0, hi = nseg;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (i < (long)seg_end[mid]) hi = mid;
            else lo = mid + 1;
        }
        float w0, w1, w2, w3;
        w0 = lo < nseg ? seg_wd[lo] : 0.f;
        if (lo >= nseg || i + 3 < (long)seg_end[lo]) w1 = w2 = w3 = w0;
        else {
            w1 = seg_wd_of(i + 1, seg_end, seg_wd, nseg);
            w2 = seg_wd_of(i + 2, seg_end, seg_wd, nseg);
            w3 = seg_wd_of(i + 3, seg_end, seg_wd, nseg);
        }
        adamw_one(P.x, G.x * gs, M.x, V.x, w0, lr, b1, b2, eps, bc1, bc2s);
        adamw_one(P.y, G.y * gs, M.y, V.y, w1, lr, b1, b2, eps, bc1, bc2s);
        adamw_one(P.z, G.z * gs, M.z, V.z, w2, lr, b1, b2, eps, bc1, bc2s);
        adamw_one(P.w, G.w * gs, M.w, V.w, w3, lr, b1, b2, eps, bc1, bc2s);
        sgx_st4(p + i, P); sgx_st4(m + i, M); sgx_st4(v + i, V);
    }
    for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {  // (n % 4 trailing elements)
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_one(pi, g[i] * gs, mi, vi, seg_wd_of(i, seg_end, seg_wd, nseg), lr, b1, b2, eps, bc1, bc2s);
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}
extern "C" int32_t sgx_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                  int32_t step, const int64_t* seg_end, const float* seg_wd, int32_t nseg, const float* grad_scale, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(p && g && m && v && step >= 1 && (nseg == 0 || (seg_end && seg_wd)), "adamw: bad args");
    float bc1 = 1.f - powf(beta1, (float)step);
    float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    SGX_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0, "adamw: arenas must be 16-byte aligned");
    long blocks = (n / 4 + 255) / 256 + 1;
    SGX_LAUNCH(adamw_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, stream, p, g, m, v, (long)n, lr, beta1, beta2, eps, bc1, bc2s,
               (const long long*)seg_end, seg_wd, nseg, grad_scale);
    SGX_CHECK_LAUNCH("adamw");
    return SGX_OK;
}

__global__ void sgd_kernel(float* p, const float* g, float* mom, long n, float lr, float momentum, float dampening, int nesterov, int first,
                           const long long* seg_end, const float* seg_wd, int nseg) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float wd = seg_wd_of(i, seg_end, seg_wd, nseg);
        float gi = g[i] + wd * p[i];
        if (momentum != 0.f) {
            float b = first ? gi : momentum * mom[i] + (1.f - dampening) * gi;
            mom[i] = b;
            gi = nesterov ? gi + momentum * b : b;
        }
        p[i] -= lr * gi;
    }
}
extern "C" int32_t sgx_sgd_step(float* p, const float* g, float* mom, int64_t n, float lr, float momentum, float dampening, int32_t nesterov,
                                int32_t first_step, const int64_t* seg_end, const float* seg_wd, int32_t nseg, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(p && g && (momentum == 0.f || mom) && (nseg == 0 || (seg_end && seg_wd)), "sgd: bad args");
    long blocks = (n + 255) / 256;
    SGX_LAUNCH(sgd_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, stream, p, g, mom, (long)n, lr, momentum, dampening, nesterov,
               first_step, (const long long*)seg_end, seg_wd, nseg);
    SGX_CHECK_LAUNCH("sgd");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Adam, RMSprop / RMSpropTF, Lion: the same sweep as adamw_kernel (four elements per lane, 16-byte accesses, one weight-decay segment
// search per four) around a per-element update `Op`.  Op::NS state arenas are loaded and stored; a disabled state buffer (RMSprop's
// grad_avg / momentum_buffer) is not an argument of its instantiation, so it is neither allocated nor moved.  Hyper-parameters reach the
// C entry points as doubles (Python's floats) and derived constants (1 - beta, lr / bias correction) are formed in double and rounded
// ONCE, the way ATen rounds the scalar arguments of mul_ / add_(alpha=) / addcmul_(value=); each `one()` keeps ATen's operation order.
__device__ __forceinline__ float4 seg_wd4(long i, const long long* seg_end, const float* seg_wd, int nseg) {
    int lo = 0, hi = nseg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i < (long)seg_end[mid]) hi = mid;
        else lo = mid + 1;
    }
    const float w0 = lo < nseg ? seg_wd[lo] : 0.f;
    if (lo >= nseg || i + 3 < (long)seg_end[lo]) return make_float4(w0, w0, w0, w0);
    return make_float4(w0, seg_wd_of(i + 1, seg_end, seg_wd, nseg), seg_wd_of(i + 2, seg_end, seg_wd, nseg), seg_wd_of(i + 3, seg_end, seg_wd, nseg));
}
struct sweep_state {
    float* s[3];
};
template <class Op>
__global__ void sweep_kernel(Op op, float* p, const float* g, sweep_state st, long n, const long long* seg_end, const float* seg_wd, int nseg,
                             const float* grad_scale) {
    const float gs = grad_scale ? grad_scale[0] : 1.f;
    const long n4 = n / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        alignas(16) float P[4], G[4], S[Op::NS][4];
        *reinterpret_cast<float4*>(P) = sgx_ld4(p + i);
        *reinterpret_cast<float4*>(G) = sgx_ld4(g + i);
#pragma unroll
        for (int j = 0; j < Op::NS; ++j) *reinterpret_cast<float4*>(S[j]) = sgx_ld4(st.s[j] + i);
        const float4 W = seg_wd4(i, seg_end, seg_wd, nseg);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float wk = k == 0 ? W.x : (k == 1 ? W.y : (k == 2 ? W.z : W.w));
            float s[Op::NS];
#pragma unroll
            for (int j = 0; j < Op::NS; ++j) s[j] = S[j][k];
            op.one(P[k], G[k] * gs, s, wk);
#pragma unroll
            for (int j = 0; j < Op::NS; ++j) S[j][k] = s[j];
        }
        sgx_st4(p + i, *reinterpret_cast<float4*>(P));
#pragma unroll
        for (int j = 0; j < Op::NS; ++j) sgx_st4(st.s[j] + i, *reinterpret_cast<float4*>(S[j]));
    }
    for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {  // (n % 4 trailing elements)
        float pi = p[i], s[Op::NS];
#pragma unroll
        for (int j = 0; j < Op::NS; ++j) s[j] = st.s[j][i];
        op.one(pi, g[i] * gs, s, seg_wd_of(i, seg_end, seg_wd, nseg));
        p[i] = pi;
#pragma unroll
        for (int j = 0; j < Op::NS; ++j) st.s[j][i] = s[j];
    }
}
static inline unsigned sweep_grid(long n) {
    const long blocks = (n / 4 + 255) / 256 + 1;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}
static inline bool aligned16(const void* a) { return ((uintptr_t)a % 16) == 0; }

// torch.lerp(a, b, w) as ATen evaluates it
__device__ __forceinline__ float lerp_aten(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w); }

// torch.optim.Adam (amsgrad=False): g += wd*p;  m.lerp_(g, 1-b1);  v = v*b2 + (1-b2)*g*g;  p += -(lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
struct adam_op {
    static const int NS = 2;
    float b2, omb1, omb2, eps, step_size, bc2s;
    __device__ __forceinline__ void one(float& p, float g, float* s, float wd) const {
        g = g + wd * p;
        s[0] = lerp_aten(s[0], g, omb1);
        s[1] = s[1] * b2 + (omb2 * g) * g;
        const float denom = sqrtf(s[1]) / bc2s + eps;
        p = p + (-step_size * s[0]) / denom;
    }
};
extern "C" int32_t sgx_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps, int32_t step,
                                 const int64_t* seg_end, const float* seg_wd, int32_t nseg, const float* grad_scale, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(p && g && m && v && step >= 1 && (nseg == 0 || (seg_end && seg_wd)), "adam: bad args");
    SGX_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "adam: arenas must be 16-byte aligned");
    adam_op op;
    op.b2 = (float)beta2, op.omb1 = (float)(1.0 - beta1), op.omb2 = (float)(1.0 - beta2), op.eps = (float)eps;
    op.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    op.bc2s = (float)sqrt(1.0 - pow(beta2, (double)step));
    sweep_state st = {{m, v, nullptr}};
    SGX_LAUNCH(sweep_kernel<adam_op>, dim3(sweep_grid(n)), dim3(256), 0, stream, op, p, g, st, (long)n, (const long long*)seg_end, seg_wd, nseg, grad_scale);
    SGX_CHECK_LAUNCH("adam");
    return SGX_OK;
}

// torch.optim.RMSprop and the reference's RMSpropTF (training/utils/optimizers/rmsprop_tf.py:89-151) in one update:
//   torch: g += wd*p;  sq = sq*a + (1-a)*g*g;  [ga.lerp_(g, 1-a)];  avg = sqrt(sq [- ga*ga]) + eps
//   TF   : p -= wd*p (decoupled) | g += wd*p;  sq += (1-a)*(g*g - sq);  [ga += (1-a)*(g - ga)];  avg = sqrt(sq [- ga*ga] + eps)
//   momentum: buf = buf*mu + g/avg, p -= lr*buf   |  TF with lr_in_momentum: buf = buf*mu + lr*g/avg, p -= buf   |  none: p -= lr*g/avg
// State order: square_avg, then grad_avg (CENTERED), then momentum_buffer (MOM).
template <bool CENTERED, bool MOM>
struct rmsprop_op {
    static const int NS = 1 + (CENTERED ? 1 : 0) + (MOM ? 1 : 0);
    float lr, alpha, oma, eps, mu;
    int tf, decoupled, lr_in_mom;
    __device__ __forceinline__ void one(float& p, float g, float* s, float wd) const {
        if (wd != 0.f) {
            if (decoupled) p = p + (-wd) * p;
            else g = g + wd * p;
        }
        float& sq = s[0];
        if (tf) sq = sq + oma * (g * g - sq);
        else sq = sq * alpha + (oma * g) * g;
        float var = sq;
        if (CENTERED) {
            float& ga = s[1];
            ga = tf ? ga + oma * (g - ga) : lerp_aten(ga, g, oma);
            var = sq + (-ga) * ga;
        }
        const float avg = tf ? sqrtf(var + eps) : sqrtf(var) + eps;
        if (MOM) {
            float& buf = s[NS - 1];
            if (lr_in_mom) {
                buf = buf * mu + (lr * g) / avg;
                p = p - buf;
            } else {
                buf = buf * mu + g / avg;
                p = p + (-lr) * buf;
            }
        } else p = p + ((-lr) * g) / avg;
    }
};
template <bool CENTERED, bool MOM>
static int32_t rmsprop_launch(float* p, const float* g, float* sq, float* gavg, float* mom, long n, double lr, double alpha, double eps, double momentum,
                              int32_t flags, const int64_t* seg_end, const float* seg_wd, int32_t nseg, const float* grad_scale, void* stream) {
    typedef rmsprop_op<CENTERED, MOM> op_t;
    op_t op;
    op.lr = (float)lr, op.alpha = (float)alpha, op.oma = (float)(1.0 - alpha), op.eps = (float)eps, op.mu = (float)momentum;
    op.tf = (flags & SGX_RMSPROP_TF) != 0, op.decoupled = (flags & SGX_RMSPROP_DECOUPLED_DECAY) != 0;
    op.lr_in_mom = op.tf && (flags & SGX_RMSPROP_LR_IN_MOMENTUM) != 0;
    sweep_state st = {{sq, CENTERED ? gavg : mom, mom}};
    SGX_LAUNCH(sweep_kernel<op_t>, dim3(sweep_grid(n)), dim3(256), 0, stream, op, p, g, st, n, (const long long*)seg_end, seg_wd, nseg, grad_scale);
    SGX_CHECK_LAUNCH("rmsprop");
    return SGX_OK;
}
extern "C" int32_t sgx_rmsprop_step(float* p, const float* g, float* square_avg, float* grad_avg, float* momentum_buffer, int64_t n, double lr, double alpha,
                                    double eps, double momentum, int32_t flags, const int64_t* seg_end, const float* seg_wd, int32_t nseg,
                                    const float* grad_scale, void* stream) {
    if (n <= 0) return SGX_OK;
    const bool centered = (flags & SGX_RMSPROP_CENTERED) != 0, mom = momentum > 0.0;
    SGX_CHECK_ARG(p && g && square_avg && (nseg == 0 || (seg_end && seg_wd)), "rmsprop: bad args");
    SGX_CHECK_ARG((grad_avg != nullptr) == centered, "rmsprop: grad_avg goes with SGX_RMSPROP_CENTERED and only with it");
    SGX_CHECK_ARG((momentum_buffer != nullptr) == mom, "rmsprop: momentum_buffer goes with momentum > 0 and only with it");
    SGX_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(square_avg) && aligned16(grad_avg) && aligned16(momentum_buffer), "rmsprop: arenas must be 16-byte aligned");
#define SGX_RMS_ARGS p, g, square_avg, grad_avg, momentum_buffer, (long)n, lr, alpha, eps, momentum, flags, seg_end, seg_wd, nseg, grad_scale, stream
    if (centered) return mom ? rmsprop_launch<true, true>(SGX_RMS_ARGS) : rmsprop_launch<true, false>(SGX_RMS_ARGS);
    return mom ? rmsprop_launch<false, true>(SGX_RMS_ARGS) : rmsprop_launch<false, false>(SGX_RMS_ARGS);
#undef SGX_RMS_ARGS
}

// Lion (training/utils/optimizers/lion.py:45-79), in the reference's order:  p *= 1 - lr*wd;  u = m*b1 + g*(1-b1);  p -= lr*sign(u);
// m = m*b2 + g*(1-b2).  Whether an element moves up or down is the SIGN of u: u is formed as rounded product + rounded product, one add -
// no contraction in this update (an fma keeps one product unrounded and can turn a u of exactly zero, or of one ulp, the other way).
struct lion_op {
    static const int NS = 1;
    float lr, b1, omb1, b2, omb2;
    __device__ __forceinline__ void one(float& p, float g, float* s, float wd) const {
#pragma clang fp contract(off)
        p = p * (1.f - lr * wd);
        const float a = s[0] * b1, b = g * omb1;
        const float u = a + b;
        p = p - lr * (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f));
        const float c = s[0] * b2, d = g * omb2;
        s[0] = c + d;
    }
};
extern "C" int32_t sgx_lion_step(float* p, const float* g, float* m, int64_t n, double lr, double beta1, double beta2, const int64_t* seg_end,
                                 const float* seg_wd, int32_t nseg, const float* grad_scale, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(p && g && m && (nseg == 0 || (seg_end && seg_wd)), "lion: bad args");
    SGX_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m), "lion: arenas must be 16-byte aligned");
    lion_op op;
    op.lr = (float)lr, op.b1 = (float)beta1, op.omb1 = (float)(1.0 - beta1), op.b2 = (float)beta2, op.omb2 = (float)(1.0 - beta2);
    sweep_state st = {{m, nullptr, nullptr}};
    SGX_LAUNCH(sweep_kernel<lion_op>, dim3(sweep_grid(n)), dim3(256), 0, stream, op, p, g, st, (long)n, (const long long*)seg_end, seg_wd, nseg, grad_scale);
    SGX_CHECK_LAUNCH("lion");
    return SGX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Lamb (training/utils/optimizers/lamb.py:123-216) over the arena, no host synchronisation, no float atomics:
//   sgx_lamb_moments : (a) lamb_gnorm_kernel - per-workgroup fp64 partials of |gs*g|^2, workgroup b owns tiles b, b + G, ... (G a function
//                          of n alone); (b) lamb_clip_kernel - one workgroup folds them in index order and writes the device scalar
//                          clip = |g| > max_grad_norm ? |g| / max_grad_norm : 1; (c) lamb_moments_kernel - m, v from g / clip, the update
//                          u = (m/bc1) / (sqrt(v)/sqrt(bc2) + eps) + wd*p, and the sums of p^2 and u^2 PER SLOT.
//   sgx_lamb_finalize: one wave per slot folds that slot's partials in tile order in fp64 and writes trust[slot].
//   sgx_lamb_apply   : recomputes u from (m, v, p) and applies p -= lr * trust[slot] * u.  u is never stored.
// Reduction layout: the arena is cut into TILES of 1024 elements (one float4 per lane of a 256-lane workgroup); tile t's sums go to
// tile_part[t] whichever workgroup computes it, so the result does not depend on the grid.  A tile inside one slot (all but ~one per
// slot) is reduced lane -> wave (shuffle tree) -> workgroup (4 waves in order) in fp64.  A tile that touches several slots stages its 1024
// squares in LDS and wave w folds slots first + w, first + w + 4, ...: the slot that owns the tile's first element goes to the HEAD entry
// of tile_part[t], the slot that owns its last element to the TAIL entry, and a slot that begins and ends inside the tile is complete
// there and goes to direct[slot].  Which entry belongs to which slot is a function of the slot table alone, and so is the fold order.
#define LAMB_TILE 1024
struct lamb_consts {
    float b1, b2, beta3, omb2, eps, bc1, bc2s;
};
__device__ __forceinline__ float lamb_update(float p, float m, float v, float wd, const lamb_consts& c) {
    const float denom = sqrtf(v) / c.bc2s + c.eps;
    float u = (m / c.bc1) / denom;
    if (wd != 0.f) u = u + wd * p;
    return u;
}
// slot that owns element i: first slot whose end is beyond i (clamped: elements past the last end belong to the last slot)
__device__ __forceinline__ int slot_of(long i, const long long* slot_end, int nslot) {
    int lo = 0, hi = nslot - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i < (long)slot_end[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ double wave_sum(double v) {  // fixed shuffle tree: the same order on every run
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__global__ __launch_bounds__(256) void lamb_gnorm_kernel(const float* g, long n, long ntile, const float* grad_scale, double* gpart) {
    __shared__ double red[4];
    const float gs = grad_scale ? grad_scale[0] : 1.f;
    double acc = 0.0;
    for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
        const long i = t * LAMB_TILE + 4 * (long)threadIdx.x;
        float s = 0.f;
        if (i + 3 < n) {
            const float4 G = sgx_ld4(g + i);
            const float a = G.x * gs, b = G.y * gs, c = G.z * gs, d = G.w * gs;
            s = (a * a + b * b) + (c * c + d * d);
        } else
            for (long j = i; j < n; ++j) s += (g[j] * gs) * (g[j] * gs);
        acc += (double)s;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) gpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(256) void lamb_clip_kernel(const double* gpart, int npart, float max_norm, float* clip) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += 256) acc += gpart[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
        clip[0] = norm > max_norm ? norm / max_norm : 1.f;
    }
}
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* p, const float* g, float* m, float* v, long n, long ntile, lamb_consts c, const float* clip,
                                                           const float* grad_scale, const long long* seg_end, const float* seg_wd, int nseg,
                                                           const long long* slot_end, int nslot, double* tile_part, double* direct) {
    __shared__ float sq[2][LAMB_TILE];
    __shared__ double red[2][2][4];
    const float gs = grad_scale ? grad_scale[0] : 1.f, cl = clip[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int par = 0;
    for (long t = blockIdx.x; t < ntile; t += gridDim.x, par ^= 1) {
        const long base = t * LAMB_TILE, tend = base + LAMB_TILE < n ? base + LAMB_TILE : n, i = base + 4 * (long)threadIdx.x;
        float pp[4] = {0.f, 0.f, 0.f, 0.f}, uu[4] = {0.f, 0.f, 0.f, 0.f};
        if (i + 3 < n) {
            alignas(16) float P[4], G[4], M[4], V[4];
            *reinterpret_cast<float4*>(P) = sgx_ld4(p + i);
            *reinterpret_cast<float4*>(G) = sgx_ld4(g + i);
            *reinterpret_cast<float4*>(M) = sgx_ld4(m + i);
            *reinterpret_cast<float4*>(V) = sgx_ld4(v + i);
            const float4 W = seg_wd4(i, seg_end, seg_wd, nseg);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wk = k == 0 ? W.x : (k == 1 ? W.y : (k == 2 ? W.z : W.w));
                const float gk = (G[k] * gs) / cl;
                M[k] = M[k] * c.b1 + c.beta3 * gk;
                V[k] = V[k] * c.b2 + (c.omb2 * gk) * gk;
                const float u = lamb_update(P[k], M[k], V[k], wk, c);
                pp[k] = P[k] * P[k], uu[k] = u * u;
            }
            sgx_st4(m + i, *reinterpret_cast<float4*>(M));
            sgx_st4(v + i, *reinterpret_cast<float4*>(V));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // (the arena's last, partly filled group of four)
                const long j = i + k;
                if (j < n) {
                    const float gk = (g[j] * gs) / cl, pj = p[j];
                    const float mj = m[j] * c.b1 + c.beta3 * gk, vj = v[j] * c.b2 + (c.omb2 * gk) * gk;
                    m[j] = mj, v[j] = vj;
                    const float u = lamb_update(pj, mj, vj, seg_wd_of(j, seg_end, seg_wd, nseg), c);
                    pp[k] = pj * pj, uu[k] = u * u;
                }
            }
        }
        const int hs = slot_of(base, slot_end, nslot), es = slot_of(tend - 1, slot_end, nslot);  // (the same in every lane)
        if (hs == es) {
            const double a = wave_sum((double)((pp[0] + pp[1]) + (pp[2] + pp[3]))), b = wave_sum((double)((uu[0] + uu[1]) + (uu[2] + uu[3])));
            if (lane == 0) red[par][0][wave] = a, red[par][1][wave] = b;
            __syncthreads();  // (red[] alternates between tiles: a wave is at most one barrier ahead of the lane that reads it)
            if (threadIdx.x == 0) {
                double* o = tile_part + 4 * t;
                o[0] = ((red[par][0][0] + red[par][0][1]) + red[par][0][2]) + red[par][0][3];
                o[1] = ((red[par][1][0] + red[par][1][1]) + red[par][1][2]) + red[par][1][3];
                o[2] = o[3] = 0.0;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) sq[0][4 * threadIdx.x + k] = pp[k], sq[1][4 * threadIdx.x + k] = uu[k];
            __syncthreads();
            for (int s = hs + wave; s <= es; s += 4) {
                const long s0 = s > 0 ? (long)slot_end[s - 1] : 0, s1 = s == nslot - 1 ? n : (long)slot_end[s];
                const int lo = (int)((s0 > base ? s0 : base) - base), hi = (int)((s1 < tend ? s1 : tend) - base);
                double a = 0.0, b = 0.0;
                for (int j = lo + lane; j < hi; j += 64) a += (double)sq[0][j], b += (double)sq[1][j];
                a = wave_sum(a), b = wave_sum(b);
                if (lane == 0) {
                    double* o = s == hs ? tile_part + 4 * t : (s == es ? tile_part + 4 * t + 2 : direct + 2 * (long)s);
                    o[0] = a, o[1] = b;
                }
            }
            __syncthreads();
        }
    }
}
__global__ __launch_bounds__(64) void lamb_trust_kernel(const long long* slot_end, int nslot, long n, const long long* seg_end, const float* seg_wd, int nseg,
                                                        int trust_clip, int always_adapt, const double* tile_part, const double* direct, float* trust) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const long s0 = s > 0 ? (long)slot_end[s - 1] : 0, s1 = s == nslot - 1 ? n : (long)slot_end[s];
    double P = 0.0, U = 0.0;
    if (s1 > s0) {
        const long t0 = s0 / LAMB_TILE, t1 = (s1 - 1) / LAMB_TILE;
        for (long t = t0 + lane; t <= t1; t += 64) {
            const long base = t * LAMB_TILE, tend = base + LAMB_TILE < n ? base + LAMB_TILE : n;
            const double* o = s0 <= base ? tile_part + 4 * t : (s1 >= tend ? tile_part + 4 * t + 2 : direct + 2 * (long)s);
            P += o[0], U += o[1];
        }
    }
    P = wave_sum(P), U = wave_sum(U);
    if (lane == 0) {
        float r = 1.f;
        if (s1 > s0 && (always_adapt || seg_wd_of(s0, seg_end, seg_wd, nseg) != 0.f)) {
            const float pn = (float)sqrt(P), un = (float)sqrt(U);
            if (pn > 0.f && un > 0.f) r = pn / un;
            if (trust_clip && r > 1.f) r = 1.f;
        }
        trust[s] = r;
    }
}
__global__ void lamb_apply_kernel(float* p, const float* m, const float* v, long n, float lr, lamb_consts c, const long long* seg_end, const float* seg_wd,
                                  int nseg, const long long* slot_end, int nslot, const float* trust) {
    const long n4 = n / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
        const long i = 4 * q;
        alignas(16) float P[4], M[4], V[4];
        *reinterpret_cast<float4*>(P) = sgx_ld4(p + i);
        *reinterpret_cast<float4*>(M) = sgx_ld4(m + i);
        *reinterpret_cast<float4*>(V) = sgx_ld4(v + i);
        const float4 W = seg_wd4(i, seg_end, seg_wd, nseg);
        const int s = slot_of(i, slot_end, nslot);
        const float t0 = trust[s];
        float4 T = make_float4(t0, t0, t0, t0);
        if (s != nslot - 1 && i + 3 >= (long)slot_end[s])
            T = make_float4(t0, trust[slot_of(i + 1, slot_end, nslot)], trust[slot_of(i + 2, slot_end, nslot)], trust[slot_of(i + 3, slot_end, nslot)]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float wk = k == 0 ? W.x : (k == 1 ? W.y : (k == 2 ? W.z : W.w)), tk = k == 0 ? T.x : (k == 1 ? T.y : (k == 2 ? T.z : T.w));
            P[k] = P[k] + (-lr) * (lamb_update(P[k], M[k], V[k], wk, c) * tk);
        }
        sgx_st4(p + i, *reinterpret_cast<float4*>(P));
    }
    for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float u = lamb_update(p[i], m[i], v[i], seg_wd_of(i, seg_end, seg_wd, nseg), c);
        p[i] = p[i] + (-lr) * (u * trust[slot_of(i, slot_end, nslot)]);
    }
}
// workspace: gpart[LAMB_GPARTS] doubles | tile_part[ntile][4] doubles | direct[nslot][2] doubles | clip (one float, 16 bytes reserved)
#define LAMB_GPARTS 1024
static inline long lamb_ntile(long n) { return (n + LAMB_TILE - 1) / LAMB_TILE; }
extern "C" int64_t sgx_lamb_workspace(int64_t n, int32_t nslot) {
    if (n <= 0 || nslot <= 0) return 16;
    return (int64_t)sizeof(double) * (LAMB_GPARTS + 4 * lamb_ntile(n) + 2 * (long)nslot) + 16;
}
static inline lamb_consts lamb_make_consts(double beta1, double beta2, double eps, int32_t step, int32_t grad_averaging) {
    lamb_consts c;
    c.b1 = (float)beta1, c.b2 = (float)beta2, c.beta3 = grad_averaging ? (float)(1.0 - beta1) : 1.f, c.omb2 = (float)(1.0 - beta2), c.eps = (float)eps;
    c.bc1 = step > 0 ? (float)(1.0 - pow(beta1, (double)step)) : 1.f;  // step = 0: bias_correction=False
    c.bc2s = step > 0 ? (float)sqrt(1.0 - pow(beta2, (double)step)) : 1.f;
    return c;
}
struct lamb_ws {
    double *gpart, *tile_part, *direct;
    float* clip;
};
static inline lamb_ws lamb_carve(void* ws, long n, int nslot) {
    lamb_ws w;
    w.gpart = (double*)ws, w.tile_part = w.gpart + LAMB_GPARTS, w.direct = w.tile_part + 4 * lamb_ntile(n), w.clip = (float*)(w.direct + 2 * (long)nslot);
    return w;
}
extern "C" int32_t sgx_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2, double eps, int32_t step,
                                    int32_t grad_averaging, double max_grad_norm, const int64_t* seg_end, const float* seg_wd, int32_t nseg,
                                    const int64_t* slot_end, int32_t nslot, const float* grad_scale, void* ws, int64_t ws_bytes, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(p && g && m && v && step >= 0 && (nseg == 0 || (seg_end && seg_wd)) && slot_end && nslot >= 1 && ws, "lamb_moments: bad args");
    SGX_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ws), "lamb_moments: arenas and workspace must be 16-byte aligned");
    SGX_CHECK_ARG(ws_bytes >= sgx_lamb_workspace(n, nslot), "lamb_moments: workspace of %ld bytes, %ld needed", (long)ws_bytes, (long)sgx_lamb_workspace(n, nslot));
    const lamb_ws w = lamb_carve(ws, n, nslot);
    const long ntile = lamb_ntile(n);
    const int gparts = (int)(ntile < LAMB_GPARTS ? ntile : LAMB_GPARTS);
    SGX_LAUNCH(lamb_gnorm_kernel, dim3(gparts), dim3(256), 0, stream, g, (long)n, ntile, grad_scale, w.gpart);
    SGX_LAUNCH(lamb_clip_kernel, dim3(1), dim3(256), 0, stream, (const double*)w.gpart, gparts, (float)max_grad_norm, w.clip);
    SGX_LAUNCH(lamb_moments_kernel, dim3((unsigned)(ntile < 4096 ? ntile : 4096)), dim3(256), 0, stream, p, g, m, v, (long)n, ntile,
               lamb_make_consts(beta1, beta2, eps, step, grad_averaging), (const float*)w.clip, grad_scale, (const long long*)seg_end, seg_wd, nseg,
               (const long long*)slot_end, nslot, w.tile_part, w.direct);
    SGX_CHECK_LAUNCH("lamb_moments");
    return SGX_OK;
}
extern "C" int32_t sgx_lamb_finalize(int64_t n, const int64_t* seg_end, const float* seg_wd, int32_t nseg, const int64_t* slot_end, int32_t nslot,
                                     int32_t trust_clip, int32_t always_adapt, const void* ws, int64_t ws_bytes, float* trust, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG((nseg == 0 || (seg_end && seg_wd)) && slot_end && nslot >= 1 && ws && trust, "lamb_finalize: bad args");
    SGX_CHECK_ARG(ws_bytes >= sgx_lamb_workspace(n, nslot), "lamb_finalize: workspace of %ld bytes, %ld needed", (long)ws_bytes, (long)sgx_lamb_workspace(n, nslot));
    const lamb_ws w = lamb_carve(const_cast<void*>(ws), n, nslot);
    SGX_LAUNCH(lamb_trust_kernel, dim3(nslot), dim3(64), 0, stream, (const long long*)slot_end, nslot, (long)n, (const long long*)seg_end, seg_wd, nseg, trust_clip,
               always_adapt, (const double*)w.tile_part, (const double*)w.direct, trust);
    SGX_CHECK_LAUNCH("lamb_finalize");
    return SGX_OK;
}
extern "C" int32_t sgx_lamb_apply(float* p, const float* m, const float* v, int64_t n, double lr, double beta1, double beta2, double eps, int32_t step,
                                  const int64_t* seg_end, const float* seg_wd, int32_t nseg, const int64_t* slot_end, int32_t nslot, const float* trust,
                                  void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(p && m && v && step >= 0 && (nseg == 0 || (seg_end && seg_wd)) && slot_end && nslot >= 1 && trust, "lamb_apply: bad args");
    SGX_CHECK_ARG(aligned16(p) && aligned16(m) && aligned16(v), "lamb_apply: arenas must be 16-byte aligned");
    SGX_LAUNCH(lamb_apply_kernel, dim3(sweep_grid(n)), dim3(256), 0, stream, p, m, v, (long)n, (float)lr, lamb_make_consts(beta1, beta2, eps, step, 1),
               (const long long*)seg_end, seg_wd, nseg, (const long long*)slot_end, nslot, trust);
    SGX_CHECK_LAUNCH("lamb_apply");
    return SGX_OK;
}

// ema = ema*decay + (1-decay)*p      (training/utils/ema.py:139-141)
__global__ void ema_kernel(float* ema, const float* p, long n, float decay) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) ema[i] = ema[i] * decay + (1.f - decay) * p[i];
}
extern "C" int32_t sgx_ema_update(float* ema, const float* p, int64_t n, float decay, void* stream) {
    if (n <= 0) return SGX_OK;
    SGX_CHECK_ARG(ema && p, "ema: null pointer");
    long blocks = (n + 255) / 256;
    SGX_LAUNCH(ema_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, stream, ema, p, (long)n, decay);
    SGX_CHECK_LAUNCH("ema");
    return SGX_OK;
}
