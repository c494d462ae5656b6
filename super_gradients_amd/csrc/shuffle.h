// ShuffleNetV2 kernels (classification_models/shufflenetv2.py) - included by bn.hip, built on its sweep skeleton and BatchNorm-backward functors.
//
// The block's `cat((left, right), 1) -> channel_shuffle(2)` is no pass here: the sweep that applies the last BatchNorm -> ReLU of a branch
// anyway carries the other half along and stores both, interleaved, as the block's output:  y[:, 2i] = L[:, i],  y[:, 2i + 1] = R[:, i].
// h is the half width - the sweep's channel count; a lane owns channels c .. c+3 of EACH half and the eight output channels 2c .. 2c+7.
// Each side is a copy (scale / shift NULL: the stride-1 block's pass-through half; both sides after the eval fold) - its bits are moved, never
// computed with - or affine, act(scale * x + shift): a branch's last BatchNorm -> activation.
//   sgx_shuffle_merge_fwd          one float4 load per side, two float4 stores at 2c and 2c + 4
//   sgx_shuffle_merge_bwd_reduce   sgx_bn_bwd_reduce of the affine side(s) on the de-interleaved gradient; two affine sides: ONE sweep, four planes
//   sgx_shuffle_merge_bwd_apply    sgx_bn_bwd_apply of the affine side(s); a copy side's gradient elements go, as they are, to its own target
// No atomics; every sum has the skeleton's fixed order, so every output repeats bit for bit.
#pragma once

// the lane's eight gradient elements at 2c -> the four of the left half (even positions) and the four of the right half (odd positions)
__device__ __forceinline__ void shuffle_split(const float* dy, long dy_ld, long r, int c, float4& l, float4& rt) {
    const float* p = dy + r * dy_ld + 2 * c;
    const float4 u = sgx_ld4(p), v = sgx_ld4(p + 4);
    l = make_float4(u.x, u.z, v.x, v.z);
    rt = make_float4(u.y, u.w, v.y, v.w);
}

// ---------------------------------------------------------------------------------------------
struct ShuffleMergeF {
    const float* l; long l_ld; const float* ls; const float* lt; int lact;
    const float* rt; long r_ld; const float* rs; const float* rsh; int ract;
    float* y; long y_ld;
    struct In { float4 a, b; };
    __device__ In load(long r, int c) const { return In{sgx_ld4(l + r * l_ld + c), sgx_ld4(rt + r * r_ld + c)}; }
    struct Cst { float4 ls, lt, rs, rt; };
    __device__ Cst consts(int c) const {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        return Cst{ls ? sgx_ld4(ls + c) : z, ls ? sgx_ld4(lt + c) : z, rs ? sgx_ld4(rs + c) : z, rs ? sgx_ld4(rsh + c) : z};
    }
    static __device__ __forceinline__ float4 side(const float4& v, const float4& s, const float4& t, int act) {
        return make_float4(sgx_act6(s.x * v.x + t.x, act), sgx_act6(s.y * v.y + t.y, act), sgx_act6(s.z * v.z + t.z, act), sgx_act6(s.w * v.w + t.w, act));
    }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        // (a copy side is never 1 * x + 0: -0.0, NaN payloads and denormals pass as they are)
        const float4 a = ls ? side(in.a, k.ls, k.lt, lact) : in.a;
        const float4 b = rs ? side(in.b, k.rs, k.rt, ract) : in.b;
        float* p = y + r * y_ld + 2 * c;
        sgx_st4(p, make_float4(a.x, b.x, a.y, b.y));
        sgx_st4(p + 4, make_float4(a.z, b.z, a.w, b.w));
    }
};
extern "C" int32_t sgx_shuffle_merge_fwd(const float* left, int64_t left_ld, const float* lscale, const float* lshift, int32_t lact, const float* right,
                                         int64_t right_ld, const float* rscale, const float* rshift, int32_t ract, float* y, int64_t y_ld, int64_t M,
                                         int32_t h, void* stream) {
    SGX_CHECK_ARG(left && right && y, "shuffle_merge_fwd: null pointer");
    SGX_CHECK_ARG((lscale == nullptr) == (lshift == nullptr) && (rscale == nullptr) == (rshift == nullptr), "shuffle_merge_fwd: scale and shift go together");
    SGX_CHECK_ACT4(lact, "shuffle_merge_fwd");
    SGX_CHECK_ACT4(ract, "shuffle_merge_fwd");
    SW_CHECK_VEC(h, SW_LD4(left_ld) && SW_LD4(right_ld) && SW_LD4(y_ld) && SW_ALIGNED(left) && SW_ALIGNED(right) && SW_ALIGNED(y) && SW_ALIGNED(lscale) &&
                        SW_ALIGNED(lshift) && SW_ALIGNED(rscale) && SW_ALIGNED(rshift),
                 "shuffle_merge_fwd");
    ShuffleMergeF f{left, left_ld, lscale, lshift, lact, right, right_ld, rscale, rshift, ract, y, y_ld};
    return run_sweep<ShuffleMergeF, 0, 4>(f, M, h, nullptr, stream, "shuffle_merge_fwd");
}

// ---------------------------------------------------------------------------------------------
// backward, stage 1.  One affine side: BnBwdReduceF on that side's elements of dy - sgx_bn_bwd_reduce's [2][sgx_stats_blocks(M)][h] rows.
// Two affine sides: both in one sweep (dy is read once), partials [4][sgx_stats_blocks(M)][h] - planes 0-1 the left side's rows, planes 2-3
// (2 * sgx_stats_blocks(M) * h floats further) the right side's; each pair is what sgx_bn_bwd_finalize / sgx_bn_reduce_sums read.
struct ShuffleBwdReduce1F : BnBwdReduceF {
    int odd;  // 0: the left side's elements of dy (even positions), 1: the right side's
    __device__ In load(long r, int c) const {
        float4 a, b;
        shuffle_split(dy, dy_ld, r, c, a, b);
        return In{odd ? b : a, sgx_ld4(x + r * x_ld + c)};
    }
};
struct ShuffleBwdReduce2F {
    BnBwdReduceF a, b;  // (a.dy == b.dy: the interleaved gradient)
    struct In { BnBwdReduceF::In a, b; };
    __device__ In load(long r, int c) const {
        In in;
        shuffle_split(a.dy, a.dy_ld, r, c, in.a.d, in.b.d);
        in.a.v = sgx_ld4(a.x + r * a.x_ld + c);
        in.b.v = sgx_ld4(b.x + r * b.x_ld + c);
        return in;
    }
    struct Cst { BnBwdReduceF::Cst a, b; };
    __device__ Cst consts(int c) const { return Cst{a.consts(c), b.consts(c)}; }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&q)[4]) const {
        float4 qa[2] = {q[0], q[1]}, qb[2] = {q[2], q[3]};
        a.apply(r, c, in.a, k.a, qa);
        b.apply(r, c, in.b, k.b, qb);
        q[0] = qa[0]; q[1] = qa[1]; q[2] = qb[0]; q[3] = qb[1];
    }
};
#define SHUF_SIDE_OK(x, ld, s, t, m) (SW_LD4(ld) && SW_ALIGNED(x) && SW_ALIGNED(s) && SW_ALIGNED(t) && SW_ALIGNED(m))
extern "C" int32_t sgx_shuffle_merge_bwd_reduce(const float* dy, int64_t dy_ld, const float* xl, int64_t xl_ld, const float* lscale, const float* lshift,
                                                const float* lmean, int32_t lact, const float* xr, int64_t xr_ld, const float* rscale, const float* rshift,
                                                const float* rmean, int32_t ract, int64_t M, int32_t h, float* partials, void* stream) {
    const bool la = xl != nullptr, ra = xr != nullptr;
    SGX_CHECK_ARG(dy && partials && (la || ra), "shuffle_merge_bwd_reduce: null pointer (dy, partials, and the x of at least one affine side)");
    SGX_CHECK_ARG((!la || (lscale && lshift && lmean)) && (!ra || (rscale && rshift && rmean)), "shuffle_merge_bwd_reduce: an affine side needs scale, shift and mean");
    SGX_CHECK_ACT4(lact, "shuffle_merge_bwd_reduce");
    SGX_CHECK_ACT4(ract, "shuffle_merge_bwd_reduce");
    SW_CHECK_VEC(h, SW_LD4(dy_ld) && SW_ALIGNED(dy) && SW_ALIGNED(partials) && (!la || SHUF_SIDE_OK(xl, xl_ld, lscale, lshift, lmean)) &&
                        (!ra || SHUF_SIDE_OK(xr, xr_ld, rscale, rshift, rmean)),
                 "shuffle_merge_bwd_reduce");
    const BnBwdReduceF fl{dy, dy_ld, xl, xl_ld, lscale, lshift, lmean, lact}, fr{dy, dy_ld, xr, xr_ld, rscale, rshift, rmean, ract};
    if (la && ra) {
        ShuffleBwdReduce2F f{fl, fr};
        return run_sweep<ShuffleBwdReduce2F, 4, 2>(f, M, h, partials, stream, "shuffle_merge_bwd_reduce");
    }
    ShuffleBwdReduce1F f{ra ? fr : fl, ra ? 1 : 0};
    return run_sweep<ShuffleBwdReduce1F, 2, 4>(f, M, h, partials, stream, "shuffle_merge_bwd_reduce");
}

// ---------------------------------------------------------------------------------------------
// backward, stage 3.  An affine side (coef != NULL) stores BnBwdApplyF's dx - in place over its saved convolution output where the caller
// says so: a row is completely read before it is written; a copy side stores its elements of dy, as they are, into its own target (the left
// channel slice of the block's input gradient).  Three or four loads per row: two rows in flight.
template <bool LA, bool RA>
struct ShuffleBwdApplyF {
    BnBwdApplyF a, b;  // (a.dy == b.dy: the interleaved gradient; a copy side uses dy, dx and dx_ld alone)
    struct In { float4 dl, dr, vl, vr; };
    __device__ In load(long r, int c) const {
        In in;
        shuffle_split(a.dy, a.dy_ld, r, c, in.dl, in.dr);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        in.vl = z, in.vr = z;
        if constexpr (LA) in.vl = sgx_ld4(a.x + r * a.x_ld + c);
        if constexpr (RA) in.vr = sgx_ld4(b.x + r * b.x_ld + c);
        return in;
    }
    struct Cst { BnBwdApplyF::Cst a, b; };
    __device__ Cst consts(int c) const {
        Cst k{};
        if constexpr (LA) k.a = a.consts(c);
        if constexpr (RA) k.b = b.consts(c);
        return k;
    }
    __device__ void apply(long r, int c, const In& in, const Cst& k, float4 (&)[1]) const {
        float4 g, ol = in.dl, orr = in.dr;
        if constexpr (LA) ol = a.dx_of(in.dl, in.vl, k.a, g);
        if constexpr (RA) orr = b.dx_of(in.dr, in.vr, k.b, g);
        sgx_st4(a.dx + r * a.dx_ld + c, ol);
        sgx_st4(b.dx + r * b.dx_ld + c, orr);
    }
};
extern "C" int32_t sgx_shuffle_merge_bwd_apply(const float* dy, int64_t dy_ld, const float* xl, int64_t xl_ld, const float* lscale, const float* lshift,
                                               const float* lcoef, int32_t lact, float* d_left, int64_t dl_ld, const float* xr, int64_t xr_ld,
                                               const float* rscale, const float* rshift, const float* rcoef, int32_t ract, float* d_right, int64_t dr_ld,
                                               int64_t M, int32_t h, void* stream) {
    const bool la = lcoef != nullptr, ra = rcoef != nullptr;
    SGX_CHECK_ARG(dy && d_left && d_right && (la || ra), "shuffle_merge_bwd_apply: null pointer (dy, both targets, and the coef of at least one affine side)");
    SGX_CHECK_ARG((!la || (xl && lscale && lshift)) && (!ra || (xr && rscale && rshift)), "shuffle_merge_bwd_apply: an affine side needs x, scale and shift");
    SGX_CHECK_ACT4(lact, "shuffle_merge_bwd_apply");
    SGX_CHECK_ACT4(ract, "shuffle_merge_bwd_apply");
    SW_CHECK_VEC(h, SW_LD4(dy_ld) && SW_ALIGNED(dy) && SW_LD4(dl_ld) && SW_ALIGNED(d_left) && SW_LD4(dr_ld) && SW_ALIGNED(d_right) &&
                        (!la || SHUF_SIDE_OK(xl, xl_ld, lscale, lshift, lcoef)) && (!ra || SHUF_SIDE_OK(xr, xr_ld, rscale, rshift, rcoef)),
                 "shuffle_merge_bwd_apply");
    const BnBwdApplyF fl{dy, dy_ld, xl, xl_ld, lscale, lshift, lcoef, h, d_left, dl_ld, nullptr, 0, lact};
    const BnBwdApplyF fr{dy, dy_ld, xr, xr_ld, rscale, rshift, rcoef, h, d_right, dr_ld, nullptr, 0, ract};
    if (la && ra) return run_sweep<ShuffleBwdApplyF<true, true>, 0, 2>(ShuffleBwdApplyF<true, true>{fl, fr}, M, h, nullptr, stream, "shuffle_merge_bwd_apply");
    if (ra) return run_sweep<ShuffleBwdApplyF<false, true>, 0, 2>(ShuffleBwdApplyF<false, true>{fl, fr}, M, h, nullptr, stream, "shuffle_merge_bwd_apply");
    return run_sweep<ShuffleBwdApplyF<true, false>, 0, 2>(ShuffleBwdApplyF<true, false>{fl, fr}, M, h, nullptr, stream, "shuffle_merge_bwd_apply");
}
#undef SHUF_SIDE_OK
