// wf_loudness_tables.hpp -- the loudness producer's per-rate constants, designed on the host (wf_loudness_tables.cpp) and
// handed to its kernels (wf_loudness.hpp) by value.  Plain C++: shared by the host and device translation units.
#pragma once
#include <cstdint>

namespace wf {

constexpr uint32_t LOUD_PHASES = 4;    // true peak: 4x oversampling
constexpr uint32_t LOUD_TAPS = 12;     // taps per phase (48 in all)
constexpr uint32_t LOUD_HISTORY = LOUD_TAPS - 1; // input samples a packet needs from before it
constexpr uint32_t LOUD_BINS = 800;    // gating histograms: 0.1 LU bins from -70 LUFS to +10 LUFS
constexpr float LOUD_BIN_LU = 0.1f;
constexpr float LOUD_GATE_ABS = -70.0f;
constexpr uint32_t LOUD_SUBS = 30;     // 100 ms sub-blocks kept: the short-term window

struct LoudCoefs {
    // K-weighting, direct form II transposed, a0 = 1: the shelf (b0, b1, b2, a1, a2), then the RLB high-pass
    double shelf[5];
    double hpf[5];
    float fir[LOUD_PHASES][LOUD_TAPS]; // y[4m + r] = sum_k fir[r][k] x[m - k]
    uint32_t sub_frames;               // sample_rate / 10
};

namespace host {
// the K-weighting biquads for `sample_rate`, in float64: {b0, b1, b2, a1, a2} of the shelf, then of the high-pass
void k_weighting(uint32_t sample_rate, double shelf[5], double hpf[5]);
// the true-peak interpolator, in float64, [LOUD_PHASES][LOUD_TAPS] as LoudCoefs::fir
void true_peak_fir(double fir[LOUD_PHASES][LOUD_TAPS]);
// both (the biquads in float64, the taps rounded to float32), with sub_frames = sample_rate / 10
LoudCoefs loudness_coefs(uint32_t sample_rate);
} // namespace host

} // namespace wf
