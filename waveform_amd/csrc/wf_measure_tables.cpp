// wf_measure_tables.cpp -- the host tables of the measurement outputs (wf_measure_tables.hpp).  Plain C++.
#include "wf_measure_tables.hpp"

#include <algorithm>
#include <cassert>
#include <cmath>

namespace wf::host {

namespace {
// The sine of an argument whose cosine is taken beside it.  g++ turns such a pair into one sincos call, and the C library's
// sincos does not give its sin in every last bit (2 pi 1955 / 4096 is one argument where it does not); the device's results
// depend on every bit of these tables, so the two stay the two calls they are written as, whichever compiler builds this.
template<class T> [[gnu::noinline]] T sin_alone(T x) { return std::sin(x); }

constexpr long double TWO_PI_L = 2.0L * 3.14159265358979323846264338327950288L;

// e^(-j 2 pi m / p), m < p / 2, as [re im] pairs of float64 rounded from long double arguments (the sonogram's and the
// distortion analyser's transforms)
void twiddles_from_long_double(double *tw, uint32_t p)
{
    for(uint32_t m = 0; m < p / 2; ++m) {
        const long double x = TWO_PI_L * (long double)m / (long double)p;
        tw[2 * (size_t)m] = (double)std::cos(x);
        tw[2 * (size_t)m + 1] = (double)-sin_alone(x);
    }
}
} // namespace

uint32_t third_octave_edges(uint32_t sample_rate, uint32_t n, uint32_t m, double edges[WF_HIP_NUM_BANDS + 1])
{
    for(int j = 0; j <= WF_HIP_NUM_BANDS; ++j)
        edges[j] = 1000.0 * std::pow(10.0, (double)(2 * (j - 17) - 1) / 20.0) * (double)n / (double)sample_rate;
    uint32_t covered = 0;
    for(int j = 0; j < WF_HIP_NUM_BANDS; ++j)
        if(edges[j] >= 0.5 && edges[j + 1] <= (double)m - 0.5)
            covered |= 1u << j;
    return covered;
}

BandsTables bands_tables(uint32_t sample_rate, uint32_t N, uint32_t M, const std::vector<float> &window)
{
    BandsTables b;
    b.edges.resize(WF_HIP_NUM_BANDS + 1);
    b.covered = third_octave_edges(sample_rate, N, M, b.edges.data());
    b.enbw = 1.0;
    if(!window.empty()) {
        double s1 = 0.0, s2 = 0.0;
        for(const float w : window) {
            s1 += (double)w;
            s2 += (double)w * (double)w;
        }
        b.enbw = (double)N * s2 / (s1 * s1);
    }
    // (R(f) / R(1000))^2 of IEC 61672-1's RA and RC at every bin's frequency
    const auto ra = [](double f) {
        const double f2 = f * f;
        return 12194.0 * 12194.0 * f2 * f2 /
               ((f2 + 20.6 * 20.6) * std::sqrt((f2 + 107.7 * 107.7) * (f2 + 737.9 * 737.9)) * (f2 + 12194.0 * 12194.0));
    };
    const auto rc = [](double f) {
        const double f2 = f * f;
        return 12194.0 * 12194.0 * f2 / ((f2 + 20.6 * 20.6) * (f2 + 12194.0 * 12194.0));
    };
    b.weights.resize((size_t)M * 2);
    for(uint32_t k = 0; k < M; ++k) {
        const double f = (double)k * (double)sample_rate / (double)N;
        const double a = ra(f) / ra(1000.0), c = rc(f) / rc(1000.0);
        b.weights[2 * (size_t)k] = a * a;
        b.weights[2 * (size_t)k + 1] = c * c;
    }
    return b;
}

uint32_t stereo_window(uint32_t fft_size)
{
    uint32_t p = 1;
    while(2 * p <= std::min<uint32_t>(fft_size, WF_HIP_STEREO_MAX_WINDOW))
        p *= 2;
    return p;
}

StereoTables stereo_tables(uint32_t sample_rate, uint32_t N)
{
    StereoTables s;
    const uint32_t P = stereo_window(N);
    std::vector<double> &tab = s.tab;
    tab.resize((size_t)2 * P + WF_HIP_NUM_BANDS + 1);
    for(uint32_t i = 0; i < P; ++i)
        tab[i] = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)P);
    for(uint32_t m = 0; m < P / 2; ++m) {
        const double x = 2.0 * M_PI * (double)m / (double)P;
        tab[P + 2 * (size_t)m] = std::cos(x);
        tab[P + 2 * (size_t)m + 1] = -sin_alone(x);
    }
    s.covered = third_octave_edges(sample_rate, P, P / 2, tab.data() + 2 * (size_t)P);
    s.P = P;
    s.log2p = 0;
    while((1u << s.log2p) < P)
        ++s.log2p;
    return s;
}

// (2^x is exp2 throughout: pow(2.0, x) is not the same function in every last bit -- 2^(11/12) is one value where the C
// library's two differ -- and exp2 is what these tables have always been made with)
CqTables cq_tables(uint32_t sample_rate, uint32_t ring_cap)
{
    CqTables q;
    const double sr = (double)sample_rate;
    const double Q = 1.0 / (std::exp2(1.0 / 12.0) - 1.0);
    const uint32_t Lmax = std::min<uint32_t>(ring_cap, WF_HIP_CQ_MAX_WINDOW); // (a power of two >= 128: a multiple of 64)
    uint32_t L[WF_HIP_CQ_BINS];
    q.max_window = Lmax;
    q.end_covered = 0;
    q.first_resolved = WF_HIP_CQ_BINS;
    for(uint32_t b = 0; b < WF_HIP_CQ_BINS; ++b) {
        const double f = 440.0 * std::exp2(((double)b - 57.0) / 12.0);
        if(f * std::exp2(1.0 / 24.0) < sr / 2.0 && q.end_covered == b)
            q.end_covered = b + 1;
        const double full = std::ceil(Q * sr / f);
        if(full <= (double)Lmax && q.first_resolved == WF_HIP_CQ_BINS)
            q.first_resolved = b;
        L[b] = full <= (double)Lmax ? (uint32_t)full : Lmax;
    }
    std::vector<double> &tab = q.tab;
    tab.assign((size_t)q.end_covered * WF_CQ_BIN_DOUBLES, 0.0);
    const long double two_pi = 2.0L * 3.14159265358979323846264338327950288L;
    for(uint32_t b = 0; b < q.end_covered; ++b) {
        const long double wc = -two_pi * 440.0L * std::exp2(((long double)b - 57.0L) / 12.0L) / (long double)sample_rate;
        const long double wh = two_pi / (long double)L[b];
        double *t = tab.data() + (size_t)b * WF_CQ_BIN_DOUBLES;
        t[0] = (double)std::cos(64.0L * wc);
        t[1] = (double)sin_alone(64.0L * wc);
        t[2] = (double)std::cos(64.0L * wh);
        t[3] = (double)sin_alone(64.0L * wh);
        t[4] = 4.0 / (double)L[b];
        t[5] = (double)L[b];
        for(uint32_t l = 0; l < 64; ++l) {
            double *v = t + WF_CQ_BIN_HEAD + 4 * (size_t)l;
            v[0] = (double)std::cos((long double)l * wc);
            v[1] = (double)sin_alone((long double)l * wc);
            v[2] = (double)std::cos((long double)l * wh);
            v[3] = (double)sin_alone((long double)l * wh);
        }
    }
    // the longest bin first, each to the wave with the least work so far (ties: the lower bin, the lower wave); a bin costs its
    // iterations plus a constant for its table, its reduction and its logarithm
    std::vector<uint32_t> lists[WF_CQ_WAVES];
    uint32_t load[WF_CQ_WAVES] = {};
    std::vector<uint32_t> by_cost(q.end_covered);
    for(uint32_t b = 0; b < q.end_covered; ++b)
        by_cost[b] = b;
    std::stable_sort(by_cost.begin(), by_cost.end(), [&](uint32_t x, uint32_t y) { return L[x] > L[y]; });
    for(const uint32_t b : by_cost) {
        const uint32_t w = (uint32_t)(std::min_element(load, load + WF_CQ_WAVES) - load);
        lists[w].push_back(b);
        load[w] += (L[b] + 63u) / 64u + 8u;
    }
    std::vector<uint32_t> &sched = q.sched;
    sched.reserve(WF_CQ_SCHED_WORDS);
    uint32_t at = 0;
    for(uint32_t w = 0; w < WF_CQ_WAVES; ++w) {
        sched.push_back(at);
        at += (uint32_t)lists[w].size();
    }
    sched.push_back(at);
    for(uint32_t w = 0; w < WF_CQ_WAVES; ++w)
        sched.insert(sched.end(), lists[w].begin(), lists[w].end());
    sched.resize(WF_CQ_SCHED_WORDS, 0u);
    return q;
}

SonoTables sono_tables(uint32_t sample_rate, uint32_t ring_cap)
{
    SonoTables s;
    constexpr uint32_t P = WF_HIP_SONO_WINDOW, H = WF_HIP_SONO_HOP, B = WF_HIP_SONO_BANDS;
    s.columns = ring_cap > P ? std::min<uint32_t>(WF_HIP_SONO_COLUMNS, (ring_cap - P) / H) : 0u;
    std::vector<double> &tab = s.tab;
    tab.resize((size_t)2 * P + B + 1);
    const long double two_pi = 2.0L * 3.14159265358979323846264338327950288L;
    for(uint32_t i = 0; i < P; ++i)
        tab[i] = (double)(0.5L - 0.5L * std::cos(two_pi * (long double)i / (long double)P));
    twiddles_from_long_double(tab.data() + P, P);
    double *edges = tab.data() + 2 * (size_t)P;
    for(uint32_t j = 0; j <= B; ++j)
        edges[j] = 62.5 * std::exp2((double)j / 8.0) * (double)P / (double)sample_rate;
    s.first_covered = B;
    s.end_covered = 0;
    for(uint32_t b = 0; b < B; ++b) {
        if(edges[b] >= 0.5 && s.first_covered == B)
            s.first_covered = b;
        if(edges[b + 1] <= (double)(P / 2) - 0.5)
            ++s.end_covered;
    }
    return s;
}

uint32_t thd_window(uint32_t fft_size)
{
    uint32_t p = 1;
    while(2 * p <= std::min<uint32_t>(fft_size, WF_HIP_THD_MAX_WINDOW))
        p *= 2;
    return p;
}

ThdTables thd_tables(uint32_t /*sample_rate*/, uint32_t N)
{
    ThdTables t;
    const uint32_t P = thd_window(N);
    static const long double a[7] = {0.27105140069342L, 0.43329793923448L, 0.21812299954311L, 0.06592544638803L,
                                     0.01081174209837L, 0.00077658482522L, 0.00001388721735L};
    std::vector<double> &tab = t.tab;
    tab.resize((size_t)2 * P);
    const long double two_pi = 2.0L * 3.14159265358979323846264338327950288L;
    // (the terms cancel down to 6e-8 at the ends: summed in long double, m ascending, the argument reduced as an integer first)
    long double s2 = 0.0L;
    for(uint32_t i = 0; i < P; ++i) {
        long double w = a[0];
        for(uint32_t m = 1; m < 7; ++m) {
            const long double c = a[m] * std::cos(two_pi * (long double)((m * i) % P) / (long double)P);
            w = (m & 1u) ? w - c : w + c;
        }
        tab[i] = (double)w;
        s2 += (long double)tab[i] * (long double)tab[i];
    }
    twiddles_from_long_double(tab.data() + P, P);
    t.S = (double)((long double)P * s2 / 4.0L);
    t.P = P;
    t.log2p = 0;
    while((1u << t.log2p) < P)
        ++t.log2p;
    return t;
}

// (WF_HIP_DELAY_MAX_WINDOW is a power of two, so the largest one <= min(fft_size, it) is the distortion analyser's, capped)
static_assert(WF_HIP_DELAY_MAX_WINDOW <= WF_HIP_THD_MAX_WINDOW && (WF_HIP_DELAY_MAX_WINDOW & (WF_HIP_DELAY_MAX_WINDOW - 1)) == 0);
uint32_t delay_window(uint32_t fft_size) { return std::min<uint32_t>(thd_window(fft_size), WF_HIP_DELAY_MAX_WINDOW); }

DelayTables delay_tables(uint32_t N)
{
    DelayTables t;
    const uint32_t P = delay_window(N);
    std::vector<double> &tab = t.tab;
    tab.resize((size_t)2 * P);
    // (in long double, the argument reduced as an integer first, as thd_tables builds its taper)
    for(uint32_t i = 0; i < P; ++i)
        tab[i] = (double)(0.5L - 0.5L * std::cos(TWO_PI_L * (long double)(i % P) / (long double)P));
    twiddles_from_long_double(tab.data() + P, P);
    t.P = P;
    t.log2p = 0;
    while((1u << t.log2p) < P)
        ++t.log2p;
    return t;
}

static_assert(WF_HIP_XFER_MAX_WINDOW <= WF_HIP_DELAY_MAX_WINDOW && (WF_HIP_XFER_MAX_WINDOW & (WF_HIP_XFER_MAX_WINDOW - 1)) == 0);
uint32_t xfer_window(uint32_t fft_size, uint32_t ring_cap)
{
    return delay_window(std::min<uint32_t>(std::min<uint32_t>(fft_size, WF_HIP_XFER_MAX_WINDOW), ring_cap / 8));
}

uint32_t xfer_segments(uint32_t P, uint32_t ring_cap) { return std::min<uint32_t>(WF_HIP_XFER_MAX_SEGMENTS, 2 * ring_cap / P - 3); }

static_assert(2 * WF_HIP_TEMPO_MAX_LAG + 2 == WF_HIP_TEMPO_LAGS, "acf[0 .. 2 lag_hi + 1] fits the entry");
TempoPlan tempo_plan(uint32_t sample_rate, uint32_t ring_cap)
{
    constexpr uint64_t P = WF_HIP_TEMPO_WINDOW, H = WF_HIP_TEMPO_HOP;
    TempoPlan t;
    if(ring_cap < WF_HIP_TEMPO_MIN_RING || sample_rate == 0)
        return t;
    t.columns = (uint32_t)std::min<uint64_t>(WF_HIP_TEMPO_COLUMNS, (ring_cap - P) / H - 1);
    const uint64_t beats = 60ull * sample_rate; // frames per minute: lag = beats / (bpm H)
    const uint64_t lo = (beats + 240 * H - 1) / (240 * H);
    t.lag_lo = (uint32_t)std::min<uint64_t>(lo, 0xFFFFFFFFu);
    t.lag_hi = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(beats / (40 * H), t.columns / 4), WF_HIP_TEMPO_MAX_LAG);
    return t;
}

TempoTables tempo_tables(uint32_t sample_rate, uint32_t ring_cap)
{
    TempoTables t;
    t.plan = tempo_plan(sample_rate, ring_cap);
    t.prior.assign(WF_HIP_TEMPO_MAX_LAG + 1, 0.0);
    for(uint32_t L = 1; L <= WF_HIP_TEMPO_MAX_LAG; ++L) {
        const double bpm = 60.0 * (double)sample_rate / ((double)WF_HIP_TEMPO_HOP * (double)L);
        const double octaves = std::log2(bpm / 120.0);
        t.prior[L] = std::exp(-0.5 * (octaves * octaves));
    }
    return t;
}

static_assert(WF_HIP_HUM_MAX_WINDOW == 32768 && (WF_HIP_HUM_MAX_WINDOW & (WF_HIP_HUM_MAX_WINDOW - 1)) == 0, "the hum detector's largest window");
HumPlan hum_plan(uint32_t sample_rate, uint32_t ring_cap)
{
    HumPlan p;
    const uint64_t sr = sample_rate;
    if(sr < 1280 || ring_cap == 0)
        return p;
    uint64_t D = 1;
    while(1280 * 2 * D <= sr)
        D *= 2;
    const uint64_t N = std::min<uint64_t>(std::min<uint64_t>(ring_cap, WF_HIP_HUM_MAX_WINDOW), 1024 * D);
    p.D = (uint32_t)D;
    p.N = (uint32_t)N;
    p.M = (uint32_t)(N / D);
    while((2u << p.log2m) <= p.M)
        ++p.log2m;
    p.hz = (double)sample_rate / (double)p.N;
    p.K = (uint32_t)((484 * N + sr - 1) / sr) + 22u;
    p.noise_lo = (uint32_t)((20 * N + sr - 1) / sr);
    p.noise_hi = (uint32_t)(484 * N / sr);
    p.any_ring = D >= 2 && sr <= 3ull * WF_HIP_HUM_MAX_WINDOW;
    p.fits = D >= 2 && sr <= 3 * N && p.M >= 64; // (hz <= 3.0; a ring that is a power of two gives M = 512 or 1024 here)
    if(!p.fits)
        return p;
    for(uint32_t i = 0; i < 2 * WF_HIP_HUM_HARMONICS; ++i) {
        const uint64_t fam = i < WF_HIP_HUM_HARMONICS ? 50 : 60, h = 1 + i % WF_HIP_HUM_HARMONICS;
        // ceil((h (2 fam - 1) N - sr) / (2 sr)) and floor((h (2 fam + 1) N + sr) / (2 sr)): 99 N >= 33 sr, so nothing is negative
        const uint64_t lo = (h * (2 * fam - 1) * N - sr + 2 * sr - 1) / (2 * sr);
        p.lo[i] = (uint32_t)std::max<uint64_t>(lo, 6);
        p.hi[i] = (uint32_t)((h * (2 * fam + 1) * N + sr) / (2 * sr));
    }
    return p;
}

HumTables hum_tables(uint32_t sample_rate, uint32_t ring_cap)
{
    HumTables t;
    t.plan = hum_plan(sample_rate, ring_cap);
    const HumPlan &p = t.plan;
    if(!p.served())
        return t;
    assert(p.K + 1 < p.M / 2 && p.hi[2 * WF_HIP_HUM_HARMONICS - 1] + WF_HIP_HUM_FLOOR_SPAN < p.K);
    t.tw.resize(p.M);
    twiddles_from_long_double(t.tw.data(), p.M);
    const size_t bins = (size_t)p.K + 2;
    t.comb.resize((size_t)p.D * bins * 2);
    for(uint32_t r = 0; r < p.D; ++r)
        for(size_t i = 0; i < bins; ++i) {
            // r k modulo N, k = i - 1 (k = -1: N - r)
            const uint64_t rk = i == 0 ? (p.N - r) % p.N : ((uint64_t)r * (i - 1)) % p.N;
            const long double x = TWO_PI_L * (long double)rk / (long double)p.N;
            t.comb[2 * (r * bins + i)] = (double)std::cos(x);
            t.comb[2 * (r * bins + i) + 1] = (double)-sin_alone(x);
        }
    t.ranges.assign(p.lo, p.lo + 2 * WF_HIP_HUM_HARMONICS);
    t.ranges.insert(t.ranges.end(), p.hi, p.hi + 2 * WF_HIP_HUM_HARMONICS);
    return t;
}

} // namespace wf::host
