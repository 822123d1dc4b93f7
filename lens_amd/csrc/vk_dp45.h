// Dormand-Prince 5(4) core shared by every adaptive integrator kernel:
// k_dopri5_thread / k_dopri5_wave (vk_kinetics.hip), k_kremling_dopri5
// (vk_kremling.hip) and the hiprtc templates vk_dopri5_spec.hip.in /
// vk_dopri5_wave_spec.hip.in, into which lens_amd/codegen.py pastes this text
// at their DP45 slot.  It is the one definition of the tableau, the cheap
// division, the step-factor power, the stage combinations, the step
// controller, the initial-step rule and the wavefront reduction, so the
// kernels agree bit for bit where they compute the same thing.
//
// Plain device code for both hipcc (after <hip/hip_runtime.h>) and hiprtc: no
// #include, builtin types only (plus HIP's int2, which both predeclare), and
// an include guard instead of #pragma once because the text also lands in a
// main file.  The units are built with -ffp-contract=off: the explicit fma()s
// below are all the fusing there is, and their nesting and operand order are
// part of the kernels' results.

#ifndef VK_DP45_H
#define VK_DP45_H

// Per-agent status bits: the public enum of include/vk_kinetics.h where that
// header is present, the same values for the hiprtc modules.
#ifndef VK_KINETICS_H
#define VK_AGENT_MAX_STEPS 1
#define VK_AGENT_H_UNDERFLOW 2
#define VK_AGENT_NONFINITE 4
#endif
static_assert(VK_AGENT_MAX_STEPS == 1 && VK_AGENT_H_UNDERFLOW == 2 && VK_AGENT_NONFINITE == 4, "status bits");

namespace dp45 {

constexpr double a21 = 1.0 / 5.0;
constexpr double a31 = 3.0 / 40.0, a32 = 9.0 / 40.0;
constexpr double a41 = 44.0 / 45.0, a42 = -56.0 / 15.0, a43 = 32.0 / 9.0;
constexpr double a51 = 19372.0 / 6561.0, a52 = -25360.0 / 2187.0, a53 = 64448.0 / 6561.0,
                 a54 = -212.0 / 729.0;
constexpr double a61 = 9017.0 / 3168.0, a62 = -355.0 / 33.0, a63 = 46732.0 / 5247.0,
                 a64 = 49.0 / 176.0, a65 = -5103.0 / 18656.0;
constexpr double b1 = 35.0 / 384.0, b3 = 500.0 / 1113.0, b4 = 125.0 / 192.0,
                 b5 = -2187.0 / 6784.0, b6 = 11.0 / 84.0;
// e = b - bhat (4th-order embedded), scipy RK45's E up to sign
constexpr double e1 = 71.0 / 57600.0, e3 = -71.0 / 16695.0, e4 = 71.0 / 1920.0,
                 e5 = -17253.0 / 339200.0, e6 = 22.0 / 525.0, e7 = -1.0 / 40.0;
// scipy RK45's step controller
constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;

// The adaptive kernels are tolerance-parity (within 1e-6 of odeint, SURVEY
// 8a), not bit-parity, so they use the cheap forms of their two costliest
// operations, this division and step_pow below.
// a/b by the hardware reciprocal plus one Newton step (~1e-15 relative; a
// second step bought nothing the 1e-6 odeint bar sees and cost 6 % of the
// Kremling step, profiles/r06/r06t/; a zero divisor gives NaN instead of inf --
// flagged non-finite either way).  The generated rate laws call it by this name.
__device__ __forceinline__ double vk_div(double a, double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    return a * r;
}

// en^-0.2 for the step-size factor (scipy RK45's error_norm ** (-1/5)) without
// libm's exp2 / log2: a single-precision estimate from the hardware v_log_f32 /
// v_exp_f32 (~1e-6 relative), then two Newton steps on en * y^5 = 1 in double
// (quadratic: ~1e-11, then rounding).  en is clamped to [1e-30, 1e30] so the
// float stays normal; outside that range the factor is capped anyway (at 10
// for en < 1e-30, at 0.2 for en > 1e30, by accept_factor / reject_factor).
// exp2(log2()) kept its polynomial constants in VGPRs across the attempt loop:
// the C5 wavefront kernel spilled them and reloaded eight in series per attempt
// (round 6).  tests/test_step_factor.py checks a numpy restatement of this.
__device__ __forceinline__ double step_pow(double en) {
    const double e = fmin(fmax(en, 1e-30), 1e30);
    double y = (double)__builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf((float)e));
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double y2 = y * y;
        const double r = fma(-e, y2 * y2 * y, 1.0);   // 1 - e y^5
        y = fma(0.2 * y, r, y);
    }
    return y;
}

// Stage inputs y + hs * sum_j a_ij k_j for one component (b2 = 0, so stage7 is
// also the 5th-order solution), and the embedded error hs * sum_j e_j k_j.  A
// kernel whose component feeds no stage (a flux integral) may instead build
// the b / e sums as the stages arrive: b1 * k1, then fma(b3, k3, .) ... in this
// same order gives the same bits.
__device__ __forceinline__ double stage2(double hs, double y, double k1) { return fma(hs, a21 * k1, y); }
__device__ __forceinline__ double stage3(double hs, double y, double k1, double k2) {
    return fma(hs, fma(a32, k2, a31 * k1), y);
}
__device__ __forceinline__ double stage4(double hs, double y, double k1, double k2, double k3) {
    return fma(hs, fma(a43, k3, fma(a42, k2, a41 * k1)), y);
}
__device__ __forceinline__ double stage5(double hs, double y, double k1, double k2, double k3, double k4) {
    return fma(hs, fma(a54, k4, fma(a53, k3, fma(a52, k2, a51 * k1))), y);
}
__device__ __forceinline__ double stage6(double hs, double y, double k1, double k2, double k3, double k4,
                                         double k5) {
    return fma(hs, fma(a65, k5, fma(a64, k4, fma(a63, k3, fma(a62, k2, a61 * k1)))), y);
}
__device__ __forceinline__ double stage7(double hs, double y, double k1, double k3, double k4, double k5,
                                         double k6) {
    return fma(hs, fma(b6, k6, fma(b5, k5, fma(b4, k4, fma(b3, k3, b1 * k1)))), y);
}
__device__ __forceinline__ double err_term(double hs, double k1, double k3, double k4, double k5, double k6,
                                           double k7) {
    return hs * fma(e7, k7, fma(e6, k6, fma(e5, k5, fma(e4, k4, fma(e3, k3, e1 * k1)))));
}
// one component's error over its tolerance; the norm is the RMS of these
__device__ __forceinline__ double err_ratio(double err, double y_old, double y_new, double rtol, double atol) {
    return vk_div(err, fma(fmax(fabs(y_old), fabs(y_new)), rtol, atol));
}

// Step controller: the factor on the attempted step hs, from the attempt's
// error norm en.  Accepted (en < 1): the next step is hs * factor; rejected:
// retry with hs * factor.  Three lines of the rule stay in the kernels' loops:
//     if (rejected) factor = fmin(1.0, factor);   // no growth right after a rejection
//     h = hs * factor;
//     h_keep = last ? fmax(h, hs * factor) : hs * factor;   // a step clipped to land on
//                                     // the interval's end does not shrink the carried step
// With any of them inside these functions the compiler if-converts the tail of
// the attempt loop differently (vk_dopri5_wspec: 61 instead of 63 VGPRs and
// another instruction stream; Kremling: another register assignment), and
// this header is not to change what the kernels compile to.
__device__ __forceinline__ double accept_factor(double en) {
    return (en == 0.0) ? MAX_FACTOR : fmin(MAX_FACTOR, SAFETY * step_pow(en));
}
__device__ __forceinline__ double reject_factor(double en) { return fmax(MIN_FACTOR, SAFETY * step_pow(en)); }

// scipy select_initial_step (order 4).  d0, d1: RMS norms of y and f(y) over
// the tolerance scale.  The trial step
//     h0 = min((d0 < 1e-5 || d1 < 1e-5) ? 1e-6 * scale : 0.01 * d0 / d1, interval)
// is written out in each kernel (as a function here it costs vk_dopri5_wspec
// one more exec-mask instruction); d2 is the norm of f(y + h0 f(y)) - f(y)
// over h0.  scale is the unit the absolute 1e-6 floor is measured in: 1.0,
// exact, where time runs in the caller's own unit; the Kremling kernel passes
// its grid interval.
__device__ __forceinline__ double initial_h1(double d1, double d2, double h0, double scale) {
    return (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6 * scale, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 0.2);
}
__device__ __forceinline__ double initial_step(double h0, double h1) { return fmin(100.0 * h0, h1); }

// Python int(x) truncates toward zero; out-of-range / non-finite -> flagged.
__device__ __forceinline__ long long trunc_count(double x, int &st) {
    if (!(fabs(x) < 9.2e18)) {
        st |= VK_AGENT_NONFINITE;
        return 0;
    }
    return (long long)x;
}

// LDS communication between the lanes of ONE wave: a wave's LDS operations
// execute in order, so only the compiler must be kept from reordering.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wavefront sum, identical in every lane: a butterfly from the smallest
// distance up.  Distances 1 and 2 are quad_perm DPP moves; once quads (then
// 8-lane groups) hold equal values, row_half_mirror / row_mirror pair them
// exactly as distances 4 / 8 would; distances 16 and 32 use the gfx950 row
// swaps (v_permlane16/32_swap), after which each lane holds v[l] and
// v[l ^ d] and adds them (FP addition commutes, so every lane gets the same
// bits).  No LDS round trip, unlike __shfl_xor (ds_bpermute).
__device__ __forceinline__ double dpp_pair(double v, int ctrl) {
    int2 x = __builtin_bit_cast(int2, v);
    int2 y;
    switch (ctrl) {   // the DPP control must be a compile-time constant
        case 0xB1:
            y.x = __builtin_amdgcn_mov_dpp(x.x, 0xB1, 0xf, 0xf, false);
            y.y = __builtin_amdgcn_mov_dpp(x.y, 0xB1, 0xf, 0xf, false);
            break;
        case 0x4E:
            y.x = __builtin_amdgcn_mov_dpp(x.x, 0x4E, 0xf, 0xf, false);
            y.y = __builtin_amdgcn_mov_dpp(x.y, 0x4E, 0xf, 0xf, false);
            break;
        case 0x141:
            y.x = __builtin_amdgcn_mov_dpp(x.x, 0x141, 0xf, 0xf, false);
            y.y = __builtin_amdgcn_mov_dpp(x.y, 0x141, 0xf, 0xf, false);
            break;
        default:
            y.x = __builtin_amdgcn_mov_dpp(x.x, 0x140, 0xf, 0xf, false);
            y.y = __builtin_amdgcn_mov_dpp(x.y, 0x140, 0xf, 0xf, false);
            break;
    }
    return v + __builtin_bit_cast(double, y);
}

__device__ __forceinline__ double wave_sum(double v) {
    v = dpp_pair(v, 0xB1);    // quad_perm [1,0,3,2]: lane ^ 1
    v = dpp_pair(v, 0x4E);    // quad_perm [2,3,0,1]: lane ^ 2
    v = dpp_pair(v, 0x141);   // row_half_mirror: the other quad of the 8-lane group
    v = dpp_pair(v, 0x140);   // row_mirror: the other 8-lane group of the row
    int2 x = __builtin_bit_cast(int2, v);
    auto lo = __builtin_amdgcn_permlane16_swap(x.x, x.x, false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(x.y, x.y, false, false);
    v = __builtin_bit_cast(double, make_int2(lo[0], hi[0])) + __builtin_bit_cast(double, make_int2(lo[1], hi[1]));
    x = __builtin_bit_cast(int2, v);
    lo = __builtin_amdgcn_permlane32_swap(x.x, x.x, false, false);
    hi = __builtin_amdgcn_permlane32_swap(x.y, x.y, false, false);
    return __builtin_bit_cast(double, make_int2(lo[0], hi[0])) + __builtin_bit_cast(double, make_int2(lo[1], hi[1]));
}

}  // namespace dp45

#endif  // VK_DP45_H
