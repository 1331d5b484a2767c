// wf_loudness_tables.cpp -- host-side design of the loudness producer's filters (include/wf_hip.h, "loudness").
//
// K-weighting (ITU-R BS.1770-4, Annex 1): the analogue prototypes of the pre-filter (a high shelf) and of the RLB high-pass,
// sampled by the bilinear transform with pre-warping at the batch's rate.  The prototype parameters below reproduce Tables 1
// and 2 of the recommendation at 48 kHz to float64 rounding (tests/test_loudness_cpu.py checks them to 1e-6).
//
// True peak (Annex 2): 4x oversampling by a 48-tap linear-phase FIR, 4 phases of 12 taps.  This is a windowed sinc
// (Kaiser, beta 7) with its cut-off at the input's Nyquist frequency; each phase is scaled to unit DC gain.  Its passband is
// flat within 0.005 dB up to a quarter of the sample rate.
#include "wf_loudness_tables.hpp"

#include <cmath>

namespace wf::host {

namespace {

constexpr double PI = 3.14159265358979323846;

// shelf: centre 1681.97 Hz, +4.0 dB, Q 0.7072; high-pass: 38.135 Hz, Q 0.5003
constexpr double SHELF_F0 = 1681.974450955533, SHELF_GAIN_DB = 3.999843853973347, SHELF_Q = 0.7071752369554196;
constexpr double SHELF_VB_EXP = 0.4996667741545416; // band gain = Vh ^ this (the shelf's mid-band weighting)
constexpr double HPF_F0 = 38.13547087602444, HPF_Q = 0.5003270373238773;

// modified Bessel function of the first kind, order 0 (series; converges fast for the betas used here)
double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    for(int k = 1; k < 64; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if(term < 1e-17 * sum)
            break;
    }
    return sum;
}

} // namespace

void k_weighting(uint32_t sample_rate, double shelf[5], double hpf[5])
{
    const double fs = sample_rate;
    {
        const double K = std::tan(PI * SHELF_F0 / fs);
        const double Vh = std::pow(10.0, SHELF_GAIN_DB / 20.0);
        const double Vb = std::pow(Vh, SHELF_VB_EXP);
        const double a0 = 1.0 + K / SHELF_Q + K * K;
        shelf[0] = (Vh + Vb * K / SHELF_Q + K * K) / a0;
        shelf[1] = 2.0 * (K * K - Vh) / a0;
        shelf[2] = (Vh - Vb * K / SHELF_Q + K * K) / a0;
        shelf[3] = 2.0 * (K * K - 1.0) / a0;
        shelf[4] = (1.0 - K / SHELF_Q + K * K) / a0;
    }
    {
        const double K = std::tan(PI * HPF_F0 / fs);
        const double a0 = 1.0 + K / HPF_Q + K * K;
        hpf[0] = 1.0; // (the table's unnormalised numerator: 1, -2, 1)
        hpf[1] = -2.0;
        hpf[2] = 1.0;
        hpf[3] = 2.0 * (K * K - 1.0) / a0;
        hpf[4] = (1.0 - K / HPF_Q + K * K) / a0;
    }
}

void true_peak_fir(double fir[LOUD_PHASES][LOUD_TAPS])
{
    constexpr uint32_t n_taps = LOUD_PHASES * LOUD_TAPS;
    constexpr double beta = 7.0;
    const double centre = (n_taps - 1) / 2.0, i0b = bessel_i0(beta);
    double h[n_taps];
    for(uint32_t n = 0; n < n_taps; ++n) {
        const double t = (n - centre) / LOUD_PHASES; // in input samples
        const double sinc = t == 0.0 ? 1.0 : std::sin(PI * t) / (PI * t);
        const double r = (n - centre) / centre;
        h[n] = sinc * bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
    }
    for(uint32_t p = 0; p < LOUD_PHASES; ++p) {
        double sum = 0.0;
        for(uint32_t k = 0; k < LOUD_TAPS; ++k)
            sum += h[k * LOUD_PHASES + p];
        for(uint32_t k = 0; k < LOUD_TAPS; ++k)
            fir[p][k] = h[k * LOUD_PHASES + p] / sum;
    }
}

LoudCoefs loudness_coefs(uint32_t sample_rate)
{
    LoudCoefs c{};
    double shelf[5], hpf[5], fir[LOUD_PHASES][LOUD_TAPS];
    k_weighting(sample_rate, shelf, hpf);
    true_peak_fir(fir);
    for(int i = 0; i < 5; ++i) {
        c.shelf[i] = shelf[i];
        c.hpf[i] = hpf[i];
    }
    for(uint32_t p = 0; p < LOUD_PHASES; ++p)
        for(uint32_t k = 0; k < LOUD_TAPS; ++k)
            c.fir[p][k] = (float)fir[p][k];
    c.sub_frames = sample_rate / 10;
    return c;
}

} // namespace wf::host
