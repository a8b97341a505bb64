// lsx_voigt.h -- the library's Voigt function, shared by the profile set-up (lsx_hip.hip: k_voigt_block, k_voigt_wphi) and the
// final-pass formal solution at arbitrary angles (lsx_rays.hip), so that both evaluate a profile to the same bits.
#pragma once
#include <math.h>

// ---- Voigt function H(a, v) = Re w(v + i a), a > 0 (utils.py:13-15 calls scipy's wofz) ----
// Trapezoid rule with step h = 1/2 on w(z) = (i/pi) int exp(-t^2)/(z - t) dt plus the residue of the pole the
// contour crosses (Chiarella & Reichel 1968; Matta & Reichel 1971):
//   H = (h a/pi) sum_n exp(-g_n^2) / ((v - g_n)^2 + a^2) + Re[ 2 exp(-z^2) / (1 -+ exp(-2 pi i z/h)) ]
// on the grid g_n = n h (sign -) or (n + 1/2) h (sign +), whichever keeps v at least h/4 away from a node; error
// ~ exp(-pi^2/h^2) = 7e-18.  Every term of the sum is positive (no cancellation in the far wings).
// W: [2][28] = exp(-g_n^2) for n = -14 .. 13 on the two grids (host-computed); WP: where the caller keeps it (global memory, or
// a copy in LDS: `const lds_f64*` of lsx_dev.h) -- the same values either way.
template <typename WP>
__device__ __forceinline__ double dev_voigt(double a, double v, WP W)
{
    const double h = 0.5;
    const double x = fabs(v);
    const double t = x * 2.0, fr = t - floor(t);
    const bool half = !(fr >= 0.25 && fr < 0.75);
    const double shift = half ? 0.5 : 0.0;
    const WP w = W + (half ? 28 : 0);
    const double a2 = a * a;
    double s = 0.0;
#pragma unroll 4
    for (int n = -14; n <= 13; ++n) {
        const double d = x - ((double)n + shift) * h;
        s += w[n + 14] / (d * d + a2);
    }
    double H = (h / M_PI) * a * s;
    if (x < 27.0 && a < 2.0 * M_PI) {
        // exp(-z^2) = exp(a^2 - x^2) (cos 2xa - i sin 2xa);  exp(-2 pi i z/h) = exp(4 pi a) (cos - i sin)(4 pi x)
        double s1, c1, st, ct;
        sincos(2.0 * x * a, &s1, &c1);
        sincospi(4.0 * x, &st, &ct);
        const double er = exp(a2 - x * x), E = exp(4.0 * M_PI * a), sg = half ? 1.0 : -1.0;
        const double dr = 1.0 + sg * E * ct, di = -sg * E * st;
        H += 2.0 * er * (c1 * dr - s1 * di) / (dr * dr + di * di);
    }
    return H;
}
