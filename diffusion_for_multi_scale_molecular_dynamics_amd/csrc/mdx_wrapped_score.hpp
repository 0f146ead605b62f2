// The wrapped-Gaussian functions shared by the analytical score units (mdx_analytical.hip, mdx_transport.hip): the wrap into
// [0, 1) and the reference's score / log-density formulas with its truncation (score/wrapped_gaussian_score.py).  Binary64.
// Header-only with internal linkage: each unit compiles its own copy, no device symbol crosses a unit.
#pragma once
#include <hip/hip_runtime.h>

namespace mdx {
namespace {

constexpr double kPi = 3.14159265358979323846;
// The reference compares sigma with the BINARY32 constant 1 / sqrt(2 pi) (score/wrapped_gaussian_score.py:37), in either precision.
constexpr double kSigmaThreshold = 0x1.988454p-2;
// ... and normalises the Gaussian with sqrt(2 pi) taken in binary32 (:78: torch.tensor(2 * torch.pi).sqrt()), in either precision.
constexpr double kSqrtTwoPi32 = 0x1.40d932p+1;

// y - floor(y) in binary64, with a result that rounds to 1 mapped to 0 (utils/basis_transformations.py:117-118)
__device__ __forceinline__ double wrap01(double y)
{
    const double r = y - floor(y);
    return (r == 1.0) ? 0.0 : r;
}

// sigma x score of one wrapped Gaussian (:131-419): 1a / 1b for sigma <= 1 / sqrt(2 pi), the Ewald form above it, each with
// the reference's truncation k in [-kmax, kmax] (the three are different truncations: at small kmax they differ).
__device__ double sigma_normalized_score(double u, double s, int kmax)
{
    if (s <= kSigmaThreshold) {
        const bool small_u = u < 0.5;
        const double inv = 1.0 / (s * s);
        double numerator = 0.0, denominator = 0.0;
        for (int k = -kmax; k <= kmax; ++k) {
            const double kd = (double)k;
            const double arg = small_u ? (kd * kd + 2.0 * u * kd) : ((kd * kd - 1.0) + 2.0 * u * (kd + 1.0));
            const double e = exp(-0.5 * arg * inv);
            numerator += kd * e;
            denominator += e;
        }
        return (-u - numerator / denominator) / s;
    }
    const double root = sqrt(2.0 * kPi);
    double z_real = 0.0, z_fourier = 0.0, d_real = 0.0, d_fourier = 0.0;
    for (int k = -kmax; k <= kmax; ++k) {
        const double kd = (double)k;
        const double upk = u + kd, sg = s * kd;
        const double e_upk = exp(-kPi * upk * upk);
        const double combination = root * s * exp(-2.0 * kPi * kPi * sg * sg) - exp(-kPi * kd * kd);
        const double angle = 2.0 * kPi * (u * kd);
        z_real += e_upk;
        z_fourier += combination * cos(angle);
        d_real += upk * e_upk;
        d_fourier += kd * combination * sin(angle);
    }
    return s * (-2.0 * kPi * (d_real + d_fourier)) / (z_real + z_fourier);
}

// log of one wrapped Gaussian (:41-92): logsumexp_k(-(u + k)^2 / 2 sigma^2) - log(sqrt(2 pi) sigma)
__device__ double log_wrapped_gaussian(double u, double s, int kmax)
{
    const double inv = 1.0 / (s * s);
    double largest = -__builtin_huge_val();
    for (int k = -kmax; k <= kmax; ++k) {
        const double upk = u + (double)k;
        const double e = -0.5 * upk * upk * inv;
        largest = e > largest ? e : largest;
    }
    double sum = 0.0;
    for (int k = -kmax; k <= kmax; ++k) {
        const double upk = u + (double)k;
        sum += exp(-0.5 * upk * upk * inv - largest);
    }
    return (largest + log(sum)) - log(kSqrtTwoPi32 * s);
}

}  // namespace
}  // namespace mdx
