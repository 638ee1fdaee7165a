// pf_flow_inc_wide.hip -- incremental inverse of the masked-autoregressive spline flow for the wide heads:
// hidden widths up to 512 and up to 32 spline bins (FlowHead(12, 384, 24) of experiments/frozen_context_heads.py:159-163),
// the shapes pf_flow_inc.hip refuses.  Same algorithm and arithmetic as that kernel (read its header first): hidden units
// sorted by degree, pass i computes only the sixteen-unit tiles that hold units of degree i through the five hidden
// stages, reductions run over the units of degree <= i, activations of all five stages stay in LDS across the D passes,
// transposed MFMA form (bf16 operands / fp32 accumulation, or v_mfma_f32_16x16x4_f32 in the parity mode), x enters the
// first masked layer as a bf16 hi | lo pair, context arrives as per-row projections.  What differs is sized for the rows:
//
// Work split.  One workgroup = 16 draws, 8 waves.  A wave owns one new tile of a pass through stages a-e (up to 8 new
// tiles: the 384 head at D = 11 has 3-4, H = 512 at D = 6 has 7-8).  The tail stage (spline parameters of feature i) is
// three 16-row tiles on three waves for K <= 16 and SIX tiles -- 32 width, 32 height, 32 derivative rows, zero padded --
// on six waves for K > 16.
//
// LDS.  The activation-row stride is the template parameter kUnits (256, 384 or 512 units; the smallest that holds H), so
// operand addresses stay one VGPR + an instruction immediate.  A row is kUnits * 2 (bf16) or * 4 (fp32) bytes = a whole
// number of 256-byte bank windows, and the 16-byte-chunk XOR swizzle of pf_flow_inc.hip is applied inside every window:
// chunk q of row r sits at window q >> 4, slot (q ^ r) & 15.  Bytes of the five stages (+ 7-10 KB of x / y / spline rows):
//   bf16: 40 KB (256), 60 KB (384), 80 KB (512);   fp32: 80 KB (256), 120 KB (384; 512 would be the whole 160 KB: refused).
//
// Register budget.  A tile row is up to 12 (H = 384) / 16 (H = 512) bf16 fragments, 24 fp32 ones at H = 384; the two
// fragment buffers that alternate between stages hold a full row each (96 / 128 / 192 VGPRs).  Chosen: ONE workgroup per
// CU = two waves per SIMD with the 256-register budget, not half-rows streamed through smaller buffers -- the rules that
// make the existing kernel fast (a fixed number of loads per stage issued a stage ahead, one uninterrupted MFMA chain per
// stage) carry over unchanged, and the 60 KB the H = 384 instantiation would leave for a second workgroup could only be
// used at <= 128 VGPRs, which two 12-fragment buffers do not fit.  Reported by the compiler (gfx950, without / with
// context): bf16 147 / 161 (256), 185 / 199 (384), 231 / 245 (512) VGPRs, fp32 233 / 247 (256), none of them with scratch;
// fp32 at 384 does NOT fit -- 256 VGPRs and 86 / 88 more spilled (204 / 260 bytes of scratch per lane).  It is the parity
// mode and stays correct; half-row streaming for that one instantiation is the open improvement.
//
// Spline inversion for K > 16: two 16-lane DPP rows per draw (32 lanes, lane = bin, two draws per wave, all 16 draws in
// one sweep of the 8 waves).  Softmax max and sum, the knot prefix scans and the selected-bin sums are the four DPP steps
// of the 16-lane form plus ONE cross-row step (ds_swizzle inside the 32-lane group): the other row's value for max and
// sums, lane 15 of the lower row for the scan's carry and for bin 16's left knot.  Parameter rows are 96 floats padded to
// 100, so that the 16 rows of a tile written by one instruction start four banks apart.
#include <hip/hip_runtime.h>

#include "pf_status.h"

#include <algorithm>
#include <cstdint>

#include "pf_flow_inc_common.h"

namespace pf {
namespace {
// ---- 32 lanes per draw ------------------------------------------------------------------------------------------
// ds_swizzle, bit mode (and | or << 5 | xor << 10, inside groups of 32 lanes): no memory access, a crossbar move
__device__ __forceinline__ float other_row(float v) {            // the value of lane ^ 16
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
}
__device__ __forceinline__ float lower_row_last(float v) {       // the value of lane 15 of the draw's lower row, in all 32 lanes
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x01E0));
}
constexpr int kParS32 = 100;               // floats per parameter row for K > 16: 32 widths | 32 heights | 32 derivatives | pad

// rqs_row16_inverse's formulas over two DPP rows, j = 0 .. 31.  Every cross-lane operation (DPP and swizzle) stays outside
// conditionals, as that function's comment explains: all 64 lanes are active at each of them.
template <bool FAST>
__device__ __forceinline__ void rqs_row32_inverse(const float* par, float yin, int K, const FwdParams& p, int j,
                                                  float& x, float& ld, bool& bad) {
    const bool live = j < K, upper = j >= 16;
    const float uw = live ? par[j] : -INFINITY, uh = live ? par[32 + j] : -INFINITY;
    const float ud = par[64 + j];                                   // raw derivative at the RIGHT knot of bin j (j < K - 1)
    const float tb = p.tail_bound, span = 2.f * tb;
    float mw = uw, mh = uh;
    row_max2(mw, mh);
    const float mw2 = other_row(mw), mh2 = other_row(mh);
    mw = fmaxf(mw, mw2); mh = fmaxf(mh, mh2);
    const float ew = live ? exp_m<FAST>(uw - mw) : 0.f, eh = live ? exp_m<FAST>(uh - mh) : 0.f;
    float sw = row_sum(ew), sh = row_sum(eh);
    const float sw2 = other_row(sw), sh2 = other_row(sh);
    sw += sw2; sh += sh2;                                           // (a + b in one row, b + a in the other: the same float)
    const float cw = div_m<FAST>(1.f - p.min_w * (float)K, sw);
    const float ch = div_m<FAST>(1.f - p.min_h * (float)K, sh);
    const float wj = live ? p.min_w + cw * ew : 0.f, hj = live ? p.min_h + ch * eh : 0.f;
    float cumw = row_scan(wj), cumh = row_scan(hj);
    const float carry_w = lower_row_last(cumw), carry_h = lower_row_last(cumh);
    cumw += upper ? carry_w : 0.f; cumh += upper ? carry_h : 0.f;   // the scan of the upper row adds the lower row's total
    const bool last = j == K - 1;
    const float kr = last ? tb : span * cumw - tb, hr = last ? tb : span * cumh - tb;       // right knots of bin j
    const float dr_raw = last ? p.deriv_const : ud;
    // left knots / derivative = the right ones of bin j - 1: row_shr:1 inside a row, lane 15 of the lower row for bin 16
    float kl = row_dpp<0x111>(kr), hl = row_dpp<0x111>(hr), dl_raw = row_dpp<0x111>(dr_raw);
    const float k15 = lower_row_last(kr), h15 = lower_row_last(hr), d15 = lower_row_last(dr_raw);
    if (j == 16) { kl = k15; hl = h15; dl_raw = d15; }
    if (j == 0) { kl = -tb; hl = -tb; dl_raw = p.deriv_const; }
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
    const float xsel = sel ? root * w + kl : 0.f;
    const float lsel = sel ? -(log_m<FAST>(dnum) - 2.f * log_m<FAST>(den)) : 0.f;
    const float bsel = (sel && !(disc >= 0.f)) ? 1.f : 0.f;
    float xs = row_sum(xsel), ls = row_sum(lsel), bs = row_sum(bsel);
    const float xs2 = other_row(xs), ls2 = other_row(ls), bs2 = other_row(bs);
    xs += xs2; ls += ls2; bs += bs2;
    x = inside ? xs : yin;
    ld = inside ? ls : 0.f;
    bad = inside && bs > 0.f;
}

constexpr int kThreads = 512, kRows = 16;
constexpr size_t wide_lds_bytes(int units, bool f32, bool k32) {
    return (size_t)5 * kRows * units * (f32 ? 4 : 2) + kRows * 64 + kRows * (16 + 16 + (k32 ? kParS32 : kParS) + 2) * 4;
}

// kUnits: activation-row stride in units (>= H); kK32: K > 16 (six tail tiles, 32 lanes per draw); kAdd (needs kCtx): the
// masked-context conditioner, as in pf_flow_inc.hip -- projection slot 1 + j added in front of block j's inner relu (stages
// b / d, each one stage behind its request), plain residual adds in stages c / e, no ReversePermutation between layers
template <int kUnits, bool kCtx, bool kF32, bool kK32, bool kAdd = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
void flow_inverse_inc_wide_kernel(const IncParams p) {
    static_assert(kCtx || !kAdd, "the additive conditioner has context by definition");
    constexpr int NF = kF32 ? kUnits / 16 : kUnits / 32;         // fragments (k-steps of 16 / 32) per tile row, at most
    constexpr int AS = kUnits * (kF32 ? 4 : 2);                  // bytes per activation row: NF / 4 bank windows of 256 bytes
    constexpr int PS = kK32 ? kParS32 : kParS;                   // floats per spline-parameter row
    constexpr int NTAIL = kK32 ? 6 : 3;                          // 16-row tiles of the final layer per feature
    static_assert(NF % 4 == 0 && AS % 256 == 0, "rows are whole bank windows");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = p.D, H = p.H, HK = kF32 ? H / 16 : H / 32;
    char* const act = smem;                                      // 5 stages x [16][kUnits]
    char* const xb = act + (size_t)5 * kRows * AS;               // [16][32] bf16: x hi (0..15) | lo (16..31)
    float* const xs = reinterpret_cast<float*>(xb + kRows * 64); // [16][16] current layer's input, fp32
    float* const ys = xs + kRows * 16;                           // [16][16] current layer's output
    float* const par = ys + kRows * 16;                          // [16][PS] spline parameters of one feature
    float* const ldacc = par + kRows * PS;                       // [16]
    uint32_t* const badf = reinterpret_cast<uint32_t*>(ldacc + kRows);

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    auto act_of = [&](int s) { return act + (size_t)s * kRows * AS; };
    const int lane16 = lane * 16;
    // B-operand read of k-step ks (chunk 4 ks + g of row c): swz[ks & 3] + (ks >> 2) * 256
    int swz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) swz[j] = c * AS + (((c ^ g) << 4) ^ (j << 6));

    // ---- initial state: y = z (coordinates of the last layer's output), log-det 0 --------------------
    for (int s = tid; s < kRows * 16; s += kThreads) {
        const int r = s >> 4, d = s & 15;
        int64_t row = row0 + r;
        if (row >= p.batch) row = p.batch - 1;
        ys[s] = d < D ? p.z[row * D + d] : 0.f;
    }
    if (tid < kRows) { ldacc[tid] = 0.f; badf[tid] = 0u; }
    // activations of units not computed yet are read through zero (masked) weights: they must be finite
    for (int s = tid * 16; s < 5 * kRows * AS; s += kThreads * 16) *reinterpret_cast<f32x4*>(act + s) = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    // this lane's context row is fixed for the whole kernel: byte offset of its projection block relative to the
    // workgroup's first context row (32-bit, through a buffer resource)
    const int64_t per = p.proj ? p.batch / p.ctx_rows : 1;
    const int64_t crow_first = p.proj ? (row0 < p.batch ? row0 : p.batch - 1) / per : 0;
    const int proj_row_bytes = p.L * 3 * H * 4;
    int poff;
    {
        int64_t row = row0 + c;
        if (row >= p.batch) row = p.batch - 1;
        poff = (int)(row / per - crow_first) * proj_row_bytes;
    }
    const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.proj ? p.proj + crow_first * (int64_t)(p.L * 3 * H) : nullptr), 0, kCtx ? kRows * proj_row_bytes : 0, 0x00020000);
    auto proj_load = [&](int l, int which, int u) {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prsrc, poff + u * 4, ((l * 3 + which) * H) * 4, 0));
    };
    for (int l = p.L - 1; l >= 0; --l) {
        const char* lw = p.w + (size_t)l * p.layer_bytes;
        const float* bias = reinterpret_cast<const float*>(lw + p.off_bias);   // b0 | b1_0 | b2_0 | b1_1 | b2_1 | bf[D][16 NTAIL]
        // x estimate of this layer starts at zero (only solved features are ever read through non-zero weights)
        for (int s = tid; s < kRows * 32; s += kThreads) reinterpret_cast<__bf16*>(xb)[s] = (__bf16)0.f;
        for (int s = tid; s < kRows * 16; s += kThreads) xs[s] = 0.f;
        __syncthreads();

        // The load rules of pf_flow_inc.hip: every global load is issued one stage before its value is used, in
        // straight-line code with a FIXED number of loads per stage (NF per fetch); fragments beyond the units of degree
        // <= i are requested through a buffer resource that ends before them (zeros, no traffic); two fragment buffers
        // X / Y alternate, and the head of pass i + 1 is requested under the spline of pass i.
        auto fetch = [&](u32x4 (&buf)[NF], int64_t off, int tile, int kmax) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<char*>(lw) + off + (int64_t)tile * HK * 1024, 0, kmax * 1024, 0x00020000);
#pragma unroll
            for (int ks = 0; ks < NF; ++ks)
                buf[ks] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane16 + 1024 * ks, 0, 0);
        };
        // one reduction over the row: four k-steps (64 bytes of the row each: one 256-byte window) per group; a whole
        // group of masked-zero fragments costs no LDS reads and no MFMAs (one uniform branch per group, never per k-step)
        auto gemm = [&](const u32x4 (&a)[NF], const char* src, int kmax) {
            f32x4 v0{0.f, 0.f, 0.f, 0.f}, v1{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k0 = 0; k0 < NF; k0 += 4) {
                if (k0 > 0 && k0 >= kmax) continue;
                if constexpr (kF32) {
                    f32x4 b[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const f32x4*>(src + swz[q] + (k0 >> 2) * 256);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 af = __builtin_bit_cast(f32x4, a[k0 + q]);
                        v0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0], b[q][0], v0, 0, 0, 0);
                        v1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1], b[q][1], v1, 0, 0, 0);
                        v0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[2], b[q][2], v0, 0, 0, 0);
                        v1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[3], b[q][3], v1, 0, 0, 0);
                    }
                    // In the 384-unit instantiation (register-starved) the compiler reuses a finished accumulator for the
                    // next group's LDS address 9 wait states behind the group's last-but-one MFMA, across the group
                    // branch; scripts/audit_accvgpr.py asks for the 10 of an 8-pass f32 MFMA.  Two explicit states, which
                    // the compiler's own hazard count does not see (inline assembly), behind each group.
                    __builtin_amdgcn_sched_barrier(0);
                    asm volatile("s_nop 1");
                } else {
                    u32x4 b[4];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) b[ks] = *reinterpret_cast<const u32x4*>(src + swz[ks] + (k0 >> 2) * 256);
                    v0 = mfma_bf16(a[k0], b[0], v0);
                    v1 = mfma_bf16(a[k0 + 1], b[1], v1);
                    v0 = mfma_bf16(a[k0 + 2], b[2], v0);
                    v1 = mfma_bf16(a[k0 + 3], b[3], v1);
                }
            }
            return v0 + v1;
        };
        // activation values of this lane (4 consecutive units u .. u + 3 of row c) into stage s
        auto put = [&](int s, int u, f32x4 val) {
            char* row = act_of(s) + c * AS;
            if constexpr (kF32) {
                const int q = u >> 2;                                               // 16-byte chunk of units u .. u + 3
                *reinterpret_cast<f32x4*>(row + (((q ^ c) & 15) << 4) + (q >> 4) * 256) = val;
            } else {
                const int q = u >> 3;                                               // 8 units per chunk
                *reinterpret_cast<bf16x4*>(row + (((q ^ c) & 15) << 4) + (q >> 4) * 256 + (u & 4) * 2) = bf16_of(val);
            }
        };
        auto kfrag = [&](int i) { return kF32 ? (p.u1[i] + 15) / 16 : (p.u1[i] + 31) / 32; };   // fragments holding the units of degree <= i
        // head registers of the coming pass (a stage's bias travels with its weights: bA / bB belong to bufA / bufB)
        f32x4 b0, bA, bB, pr0, pg0, pg1;
        u32x4 a0;
        const int wf = wave < NTAIL ? wave : NTAIL - 1;

        // stage f of pass i (spline parameters of feature i from the last hidden state) + the spline inversion;
        // X holds the stage's weights, Y receives the first hidden matrix of pass i + 1
        auto tail = [&](int i, u32x4 (&X)[NF], f32x4& bX, u32x4 (&Y)[NF], f32x4& bY) {
            if (wave < NTAIL) {
                const f32x4 v = gemm(X, act_of(4), kfrag(i));
                *reinterpret_cast<f32x4*>(par + c * PS + 16 * wf + 4 * g) = v + bX;
            }
            // head of pass i + 1, requested after the stage's own operands have been consumed
            if (i + 1 < D) {
                const int t_lo = p.u1[i] / 16, ntile = (p.u1[i + 1] + 15) / 16 - t_lo;
                if (wave < ntile) {
                    const int t = t_lo + wave, u = 16 * t + 4 * g;
                    b0 = *reinterpret_cast<const f32x4*>(bias + u);
                    bY = *reinterpret_cast<const f32x4*>(bias + H + u);
                    if constexpr (kCtx) {
                        pr0 = proj_load(l, 0, u);
                        pg0 = proj_load(l, 1, u);
                    }
                    a0 = *reinterpret_cast<const u32x4*>(lw + ((size_t)t * 64 + lane) * 16);
                    fetch(Y, p.off_w1[0], t, kfrag(i + 1));
                }
            }
            __syncthreads();
            // ---- spline inversion: lane = bin; K > 16: 32 lanes per draw, the 16 draws in one sweep of the 8 waves;
            // K <= 16: 16 lanes per draw on the first four waves (uniform per wave)
            {
                const int r = kK32 ? tid >> 5 : tid >> 4, j = kK32 ? tid & 31 : tid & 15;
                if (r < kRows) {
                    float xv, ld;
                    bool bad;
                    if constexpr (kK32) rqs_row32_inverse<!kF32>(par + r * PS, ys[r * 16 + i], p.K, p.sp, j, xv, ld, bad);
                    else rqs_row16_inverse<!kF32>(par + r * PS, ys[r * 16 + i], p.K, p.sp, j, xv, ld, bad);
                    if (j == 0) {
                        xs[r * 16 + i] = xv;
                        const __bf16 hi = (__bf16)xv;
                        reinterpret_cast<__bf16*>(xb)[r * 32 + i] = hi;
                        reinterpret_cast<__bf16*>(xb)[r * 32 + 16 + i] = (__bf16)(xv - (float)hi);
                        ldacc[r] += ld;
                        if (bad) badf[r] = 1u;
                    }
                }
            }
            __syncthreads();
        };
        // pass i >= 1: the new hidden units (degree == i) through the five hidden stages, then the tail.
        // X holds the first hidden matrix on entry and stage f's weights on exit.
        auto pass = [&](int i, u32x4 (&X)[NF], f32x4& bX, u32x4 (&Y)[NF], f32x4& bY) {
            const int t_lo = p.u1[i - 1] / 16, ntile = (p.u1[i] + 15) / 16 - t_lo;
            const int kmax = kfrag(i);
            const bool mine = wave < ntile;                  // a wave owns a new tile
            const int t = t_lo + wave, u = 16 * t + 4 * g;
            f32x4 h;
            if (mine) {                                                             // ---- stage a: h0 = W0 . (x hi|lo) + b0 + relu(pc)
                f32x4 w0;
                if constexpr (kF32) {
                    const f32x4 bx = *reinterpret_cast<const f32x4*>(xs + c * 16 + 4 * g);
                    const f32x4 af = __builtin_bit_cast(f32x4, a0);
                    f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bx[e], acc, 0, 0, 0);
                    w0 = acc + b0;
                } else {
                    const u32x4 bx0 = *reinterpret_cast<const u32x4*>(xb + c * 64 + g * 16);
                    w0 = mfma_bf16(a0, bx0, f32x4{0.f, 0.f, 0.f, 0.f}) + b0;
                }
                if constexpr (kCtx) w0 = w0 + relu4(pr0);
                h = w0;
                put(0, u, relu4(w0));
            }
            __syncthreads();
            if (mine) {                                                             // ---- stage b: act1 = relu(W1 . act0 + b1 [+ pg0: kAdd])
                fetch(Y, p.off_w2[0], t, kmax);
                bY = *reinterpret_cast<const f32x4*>(bias + 2 * H + u);
                if constexpr (kAdd) put(1, u, relu4(gemm(X, act_of(0), kmax) + bX + pg0));
                else put(1, u, relu4(gemm(X, act_of(0), kmax) + bX));
            }
            __syncthreads();
            if (mine) {                                                             // ---- stage c: h1 = h0 + (W2 . act1 + b2) sigmoid(pg0)  (kAdd: no gate)
                fetch(X, p.off_w1[1], t, kmax);
                bX = *reinterpret_cast<const f32x4*>(bias + 3 * H + u);
                if constexpr (kCtx) pg1 = proj_load(l, 2, u);
                f32x4 d = gemm(Y, act_of(1), kmax) + bY;
                if constexpr (kCtx && !kAdd) d = d * sigmoid4<!kF32>(pg0);
                h = h + d;
                put(2, u, relu4(h));
            }
            __syncthreads();
            if (mine) {                                                             // ---- stage d  (kAdd: + pg1, requested in stage c)
                fetch(Y, p.off_w2[1], t, kmax);
                bY = *reinterpret_cast<const f32x4*>(bias + 4 * H + u);
                if constexpr (kAdd) put(3, u, relu4(gemm(X, act_of(2), kmax) + bX + pg1));
                else put(3, u, relu4(gemm(X, act_of(2), kmax) + bX));
            }
            __syncthreads();
            // stage f's weights, one stage ahead; unconditional (an empty resource for waves without a tail tile): it sits
            // between the fetch of Y and its use
            fetch(X, p.off_wf, NTAIL * i + wf, wave < NTAIL ? kmax : 0);
            bX = *reinterpret_cast<const f32x4*>(bias + 5 * H + 16 * NTAIL * i + 16 * wf + 4 * g);
            if (mine) {                                                             // ---- stage e: h2 = h1 + (W2 . act3 + b2) sigmoid(pg1)  (kAdd: no gate)
                f32x4 d = gemm(Y, act_of(3), kmax) + bY;
                if constexpr (kCtx && !kAdd) d = d * sigmoid4<!kF32>(pg1);
                h = h + d;
                put(4, u, h);
            }
            __syncthreads();
            tail(i, X, bX, Y, bY);
        };
        u32x4 bufA[NF], bufB[NF];
        // feature 0 depends on no hidden unit: its parameters are the bias (+ masked zeros)
        fetch(bufA, p.off_wf, wf, 0);
        bA = *reinterpret_cast<const f32x4*>(bias + 5 * H + 16 * wf + 4 * g);
        tail(0, bufA, bA, bufB, bB);
        for (int i = 1; i < D; i += 2) {
            pass(i, bufB, bB, bufA, bA);
            if (i + 1 < D) pass(i + 1, bufA, bA, bufB, bB);
        }
        // this layer's input is the previous layer's output, reversed (ReversePermutation precedes every layer; the
        // masked-context flow has none)
        for (int s = tid; s < kRows * 16; s += kThreads) {
            const int r = s >> 4, d = s & 15;
            ys[s] = d < D ? xs[r * 16 + (kAdd ? d : D - 1 - d)] : 0.f;
        }
        __syncthreads();
    }
    // ---- ys now holds x[:, ar_perm]; undo the autoregressive order and store ------------------------------
    if (tid < kRows) {
        const int64_t row = row0 + tid;
        if (row < p.batch) {
            for (int d = 0; d < D; ++d) {
                const int src = p.inv_perm ? p.inv_perm[d] : d;
                p.x[row * D + d] = ys[tid * 16 + src];
            }
            if (p.logdet) p.logdet[row] = ldacc[tid];
            if (p.fail && badf[tid]) atomicOr(p.fail + row, 1u);
        }
    }
}

using WideKern = void (*)(const IncParams);
struct WideVariant { WideKern k; size_t lds; };
template <int kUnits, bool kF32, bool kK32>
WideVariant wide_variant(bool ctx, bool add) {
    return {add ? flow_inverse_inc_wide_kernel<kUnits, true, kF32, kK32, true>
                : ctx ? flow_inverse_inc_wide_kernel<kUnits, true, kF32, kK32> : flow_inverse_inc_wide_kernel<kUnits, false, kF32, kK32>,
            wide_lds_bytes(kUnits, kF32, kK32)};
}
}  // namespace

// layer block of the wide kernel: the section order of pf_flow_inverse_inc, 16 * tail_tiles final-layer rows per feature
// (tail_tiles = 3 for K <= 16, 6 above)
int64_t inc_wide_layer_bytes(int D, int H, int K, bool f32) {
    const int64_t NT = H / 16, HK = f32 ? H / 16 : H / 32, NTAIL = K > 16 ? 6 : 3;          // 1 KB fragments per tile row
    return (NT + 4 * NT * HK + NTAIL * (int64_t)D * HK) * 1024 + (5 * (int64_t)H + 16 * NTAIL * (int64_t)D) * 4;
}

// PF_ERR_UNSUPPORTED: fp32 at H > 384 (five fp32 stages of 16 rows x 512 units are the whole 160 KB of LDS), or more than
// 8 sixteen-unit tiles holding the units of one degree (a wave owns one new tile per pass).  The caller (pf_api.hip) has
// checked H, K and D.
int flow_inverse_inc_wide(const PfFlowDesc& d, bool additive, float deriv_const, const int32_t* u1, const void* packed, const float* proj,
                          int64_t ctx_rows, const float* z, const int32_t* inv_perm, int64_t batch, float* x, float* logdet,
                          uint32_t* fail, hipStream_t s) {
    IncParams p{};
    p.sp.tail_bound = d.tail_bound; p.sp.min_w = d.min_bin_width; p.sp.min_h = d.min_bin_height;
    p.sp.min_d = d.min_derivative; p.sp.deriv_const = deriv_const;
    p.w = static_cast<const char*>(packed); p.proj = proj; p.z = z; p.x = x; p.logdet = logdet; p.fail = fail;
    p.inv_perm = inv_perm; p.batch = batch; p.ctx_rows = ctx_rows;
    p.D = d.features; p.H = d.hidden_features; p.K = d.num_bins; p.L = d.num_layers;
    const bool f32 = d.precision == PF_PREC_F32, k32 = p.K > 16, ctx = proj != nullptr, add = additive;
    if (add && !ctx) return PF_ERR_BAD_ARG;                      // (the additive instantiations read the projections)
    if (f32 && p.H > 384) return PF_ERR_UNSUPPORTED;
    int max_tiles = 0;
    for (int i = 1; i < p.D; ++i) max_tiles = std::max(max_tiles, (u1[i] + 15) / 16 - u1[i - 1] / 16);
    if (max_tiles > 8) return PF_ERR_UNSUPPORTED;
    if (p.H <= 256 && !k32) return PF_ERR_UNSUPPORTED;           // (served by pf_flow_inc.hip)
    const int64_t NT = p.H / 16, HK = f32 ? p.H / 16 : p.H / 32;
    p.off_w1[0] = NT * 1024;
    p.off_w2[0] = p.off_w1[0] + NT * HK * 1024;
    p.off_w1[1] = p.off_w2[0] + NT * HK * 1024;
    p.off_w2[1] = p.off_w1[1] + NT * HK * 1024;
    p.off_wf = p.off_w2[1] + NT * HK * 1024;
    p.off_bias = p.off_wf + (k32 ? 6 : 3) * (int64_t)p.D * HK * 1024;
    p.layer_bytes = inc_wide_layer_bytes(p.D, p.H, p.K, f32);
    for (int i = 0; i <= p.D; ++i) p.u1[i] = u1[i];
    // the row stride is the smallest instantiated one that holds H; H <= 256 comes here only with K > 16
    WideVariant v;
    if (p.H <= 256) v = f32 ? wide_variant<256, true, true>(ctx, add) : wide_variant<256, false, true>(ctx, add);
    else if (p.H <= 384)
        v = f32 ? (k32 ? wide_variant<384, true, true>(ctx, add) : wide_variant<384, true, false>(ctx, add))
                : (k32 ? wide_variant<384, false, true>(ctx, add) : wide_variant<384, false, false>(ctx, add));
    else v = k32 ? wide_variant<512, false, true>(ctx, add) : wide_variant<512, false, false>(ctx, add);
    // the opt-in to > 64 KB of dynamic LDS is a per-device function attribute: set before every launch, as the forward
    // kernels' launch_variant does
    if (v.lds > 64 * 1024 && !opt_in_lds(reinterpret_cast<const void*>(v.k), (int)v.lds)) return PF_ERR_HIP;
    const dim3 grid(static_cast<unsigned>((batch + 15) / 16));
    v.k<<<grid, dim3(kThreads), v.lds, s>>>(p);
    return launch_status();
}
}  // namespace pf
