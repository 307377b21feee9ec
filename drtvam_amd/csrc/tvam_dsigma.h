// tvam_dsigma.h -- the visit weight of the extinction derivative, shared by
// the kernels of tvam_dsigma.hip and the host entry tvam_dsigma_weights.
//
// A visit that starts at in-medium path length T0 and lasts dt >= 0 deposits
// e^{-s T0} - e^{-s (T0 + dt)} per unit emission (s = sigma_t, albedo 0).  Its derivative in s:
//   w'(T0, dt) = (T0 + dt) e^{-s (T0 + dt)} - T0 e^{-s T0}
//              = e^{-s T0} (dt (1 - q) - T0 q),   q = 1 - e^{-s dt}
// evaluated in the second form: q without cancellation (tvam_omexp), so the two products cancel
// only where the derivative itself changes sign (s T0 ~ 1).
#pragma once
#include "tvam_common.h"

TVAM_HD float tvam_dsig_exp2(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(x);
#else
    return exp2f(x);
#endif
}

// e^{-s T0} as cn_dda forms it: exp2(nsig2 T0) with nsig2 = -s log2(e) (TvamConsts::nsig2's
// expression).  q is tvam_omexp(s dt) on the device; the host takes the same polynomial below 0.05
// and exp2f above.  1 - q is e^{-s dt} itself on the direct branch (1 - (1 - e) would lose e's low
// bits once s dt > ln 2).
TVAM_HD float tvam_dsig_weight(float sig_t, float T0, float dt) {
    const float nsig2 = -sig_t * 1.44269504088896340736f;
    dt = fmaxf(dt, 0.0f);
    const float x = sig_t * dt;
    const bool small = x < 0.05f;
#if defined(__HIP_DEVICE_COMPILE__)
    const float q = tvam_omexp(x);
#else
    const float q = small ? x * fmaf(x, fmaf(x, fmaf(x, -4.1666668e-2f, 0.16666667f), -0.5f), 1.0f)
                          : 1.0f - tvam_dsig_exp2(TVAM_NLOG2E * x);
#endif
    const float omq = small ? 1.0f - q : tvam_dsig_exp2(TVAM_NLOG2E * x);
    return tvam_dsig_exp2(nsig2 * T0) * (dt * omq - T0 * q);
}
