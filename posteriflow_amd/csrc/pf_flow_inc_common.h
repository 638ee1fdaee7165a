// pf_flow_inc_common.h -- what the two incremental-inverse kernels share (pf_flow_inc.hip: H <= 256, K <= 16;
// pf_flow_inc_wide.hip: H <= 512, K <= 32): the kernel parameters, the MFMA / math wrappers and the lane-parallel
// spline inversion with one 16-lane DPP row per draw.  Device code only, included once per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_flow_fwd_kernel.h"

namespace pf {
namespace {
constexpr int kParS = kParStride;          // floats per row in the spline-parameter transpose (52)

struct IncParams {
    FwdParams sp;              // spline scalars only: tail_bound, min_w, min_h, min_d, deriv_const
    const char* w;             // L layer blocks (see pf_hip.h, pf_flow_inverse_inc)
    const float* proj;         // [ctx_rows][L][3][H] fp32 in sorted-unit order, or null when C = 0: slot 0 = the MADE-level context
                               // layer, slots 1 / 2 = the blocks' gates (GLU) or additive projections (kAdd, masked context)
    const float* z;            // [batch][D]
    float* x;                  // [batch][D]
    float* logdet;             // [batch] or null
    uint32_t* fail;            // [batch] or null
    const int32_t* inv_perm;   // [D] or null
    int64_t batch, ctx_rows, layer_bytes;
    int64_t off_w1[2], off_w2[2], off_wf, off_bias;      // byte offsets inside a layer block (W0 at 0)
    int D, H, K, L;
    int u1[17];                // number of hidden units (sorted order) with degree <= i
    unsigned long long* trace; // $PF_INC_TRACE: stage timestamps of workgroup 0 / wave 0 (debug)
};

// MFMA operands travel as four dwords: a <8 x bfloat> that lives across a branch is split into halves and re-packed
// (v_bfi) right behind its load, which makes the load synchronous
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ bf16x4 bf16_of(f32x4 v) {
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
    return o;
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    return v;
}
// (math helpers: pf_flow_fwd_kernel.h -- bare instructions in bf16 mode, corrected to ~1 ulp in the fp32 parity mode)
template <bool FAST> __device__ __forceinline__ float exp_m(float v) { return FAST ? pf_exp<true>(v) : pf_exp_acc(v); }
template <bool FAST> __device__ __forceinline__ float log_m(float v) { return FAST ? pf_log<true>(v) : pf_log_acc(v); }
template <bool FAST> __device__ __forceinline__ float div_m(float a, float b) { return FAST ? pf_div<true>(a, b) : pf_div_acc(a, b); }
template <bool FAST> __device__ __forceinline__ float sqrt_m(float v) { return __builtin_amdgcn_sqrtf(v); }
template <bool FAST> __device__ __forceinline__ float softplus_m(float u) { return FAST ? pf_softplus<true>(u) : pf_softplus_acc(u); }
template <bool FAST> __device__ __forceinline__ f32x4 sigmoid4(f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        v[e] = FAST ? __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v[e] * -1.44269504f)) : pf_div_acc(1.f, 1.f + pf_exp_acc(-v[e]));
    return v;
}

// ---- lane-parallel spline inverse: 16 lanes (one DPP row) per draw, lane j = bin j ------------------------
// With one lane per draw the inversion is ~600 dependent instructions on a single wave while the other seven
// wait (28 % of the kernel); with a lane per bin the softmax sums, the knot prefix sums and the bin selection
// are 4-step DPP row operations and the chain is ~5x shorter.  Same formulas as rqs_pair_inverse; the prefix
// sums associate as a scan instead of left to right (fp32 rounding only).
template <int CTRL>
__device__ __forceinline__ float row_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_sum(float v) {
    v += row_dpp<0xB1>(v); v += row_dpp<0x4E>(v); v += row_dpp<0x141>(v); v += row_dpp<0x140>(v);
    return v;
}
// max over the 16 lanes of a row for two values at once: v_max_f32_dpp directly (through fmaxf every step costs a DPP
// move plus two NaN-quieting v_max); a VGPR written by a VALU instruction needs two wait states before a DPP read
__device__ __forceinline__ void row_max2(float& a, float& b) {
    asm volatile(
        "s_nop 1\n"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
        "v_max_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
        "s_nop 0\n"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
        "v_max_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
        "s_nop 0\n"
        "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n"
        "v_max_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n"
        "s_nop 0\n"
        "v_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n"
        "v_max_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n"
        "s_nop 1\n"
        : "+v"(a), "+v"(b));
}
// raw transcendental instructions (1 ulp, no denormal-range fix-ups: every argument here is a normal number)
__device__ __forceinline__ float row_scan(float v) {            // inclusive prefix sum over the 16 lanes of a row
    v += row_dpp<0x111>(v); v += row_dpp<0x112>(v); v += row_dpp<0x114>(v); v += row_dpp<0x118>(v);
    return v;
}
template <bool FAST>
__device__ __forceinline__ void rqs_row16_inverse(const float* par, float yin, int K, const FwdParams& p, int j,
                                                  float& x, float& ld, bool& bad) {
    const bool live = j < K;
    const float uw = live ? par[j] : -INFINITY, uh = live ? par[16 + j] : -INFINITY;
    const float ud = par[32 + j];                                   // raw derivative at the RIGHT knot of bin j (j < K - 1)
    const float tb = p.tail_bound, span = 2.f * tb;
    // (every DPP reduction is evaluated OUTSIDE conditionals: inside `live ? ... : ...` the compiler may run it with
    // the non-live lanes masked off, and a DPP read of a disabled lane is not the lane's value)
    float mw = uw, mh = uh;
    row_max2(mw, mh);
    const float ew = live ? exp_m<FAST>(uw - mw) : 0.f, eh = live ? exp_m<FAST>(uh - mh) : 0.f;
    const float cw = div_m<FAST>(1.f - p.min_w * (float)K, row_sum(ew));
    const float ch = div_m<FAST>(1.f - p.min_h * (float)K, row_sum(eh));
    const float wj = live ? p.min_w + cw * ew : 0.f, hj = live ? p.min_h + ch * eh : 0.f;
    const float cumw = row_scan(wj), cumh = row_scan(hj);
    const bool last = j == K - 1;
    const float kr = last ? tb : span * cumw - tb, hr = last ? tb : span * cumh - tb;       // right knots of bin j
    const float dr_raw = last ? p.deriv_const : ud;
    // left knots / derivative = the right ones of bin j - 1 (row_shr:1), the interval's ends for bin 0
    float kl = row_dpp<0x111>(kr), hl = row_dpp<0x111>(hr), dl_raw = row_dpp<0x111>(dr_raw);
    if (j == 0) { kl = -tb; hl = -tb; dl_raw = p.deriv_const; }
    // searchsorted on the heights: bin j holds y if y >= its left knot and not >= its right knot (last knot + 1e-6)
    const bool ge_r = yin >= (last ? tb + 1e-6f : hr);
    const bool ge_l = j == 0 ? true : yin >= hl;
    const bool sel = live && ge_l && !ge_r;
    const float w = kr - kl, hh = hr - hl;
    const float dl = p.min_d + softplus_m<FAST>(dl_raw), dr = p.min_d + softplus_m<FAST>(dr_raw);
    const float delta = div_m<FAST>(hh, w);
    const float dy = yin - hl, s2 = dl + dr - 2.f * delta;
    const float a = dy * s2 + hh * (delta - dl), b = hh * dl - dy * s2, c0 = -delta * dy;
    const float disc = b * b - 4.f * a * c0;
    const float root = div_m<FAST>(2.f * c0, -b - sqrt_m<FAST>(fmaxf(disc, 0.f)));
    const float tt = root * (1.f - root), den = delta + s2 * tt, omt = 1.f - root;
    const float dnum = delta * delta * (dr * root * root + 2.f * delta * tt + dl * omt * omt);
    const bool inside = (yin >= -tb) && (yin <= tb);
    // exactly one bin is selected inside the interval: its values reach every lane of the row through a sum
    const float xsel = sel ? root * w + kl : 0.f;
    const float lsel = sel ? -(log_m<FAST>(dnum) - 2.f * log_m<FAST>(den)) : 0.f;
    const float bsel = (sel && !(disc >= 0.f)) ? 1.f : 0.f;
    const float xs = row_sum(xsel), ls = row_sum(lsel), bs = row_sum(bsel);
    x = inside ? xs : yin;
    ld = inside ? ls : 0.f;
    bad = inside && bs > 0.f;
}
}  // namespace
}  // namespace pf
