// rate_taps.h -- the windowed-sinc polyphase design of resample.cpp's header, as functions of the rate pair alone: the shape of a pair's tap
// table and the taps themselves.  No HIP header: its two users are rate_filter (resample.cpp, k_resample's filters) and the true-peak meter
// (true_peak.cpp, the pair 24000 -> 192000), which a plain C++ compiler builds.  The limits on public rates are rate_pair_error's, not this file's.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <numeric>

namespace ptts {

constexpr double kKaiserBeta = 8.6;

inline double bessel_i0(double x) {   // power series; converges quickly for the arguments here (<= beta)
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0

// L phases of K taps; tap k of a phase weighs input d = dlo + k relative to the output's own; A = 80 max(L, M) is the integer support bound
struct RateShape { int L, M, K, dlo; int64_t A; };
inline RateShape rate_shape(int in_rate, int out_rate) {
    const int g = std::gcd(in_rate, out_rate);
    RateShape s;
    s.L = out_rate / g; s.M = in_rate / g;
    s.A = 80 * (int64_t)std::max(s.L, s.M);
    // d of phase p runs over (3p - A) / (3L) < d < (3p + A) / (3L); the widest range over the phases is from p = 0 to p = L - 1
    s.dlo = (int)(floor_div(-s.A, 3 * (int64_t)s.L) + 1);
    const int64_t p = s.L - 1, num = 3 * p + s.A, den = 3 * (int64_t)s.L;
    const int64_t dhi = (num + den - 1) / den - 1;
    s.K = (int)(dhi - s.dlo + 1);
    return s;
}

// taps[p * K + k] of the shape, float64 rounded once to f32; taps outside the support stay as they are (the caller zeroes the table)
inline void rate_taps(const RateShape& sh, float* taps) {
    const double rho = std::min(1.0, (double)sh.L / sh.M), fc = 0.5 * rho * 0.9, W = 24.0 / (2.0 * fc), i0b = bessel_i0(kKaiserBeta);
    for (int p = 0; p < sh.L; p++)
        for (int k = 0; k < sh.K; k++) {
            const int64_t d = sh.dlo + k;
            if (3 * std::llabs((int64_t)p - d * sh.L) >= sh.A) continue;   // outside |t| < W: 0
            const double t = (double)p / sh.L - (double)d;
            const double x = 2.0 * fc * t;
            const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
            const double r = t / W, win = bessel_i0(kKaiserBeta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            taps[(size_t)p * sh.K + k] = (float)(2.0 * fc * sinc * win);
        }
}

}  // namespace ptts
