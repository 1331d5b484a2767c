// wf_measure_tables.hpp -- what the measurement outputs WF_HIP_OUT_BANDS, _STEREO, _CQ, _SONO, _THD, _DELAY, _XFER, _IMPULSE, _TEMPO and _HUM derive from the configuration alone,
// built on the host (wf_measure_tables.cpp) at the output's first read and uploaded by wf_hip_measure.hip.  Plain C++: no HIP
// and no handle, so the arithmetic also compiles into a program of its own (tests/test_measure_tables_cpu.py).  The sizes of
// the constant-Q tables are in wf_cq_sizes.hpp, shared with the kernel (wf_cq.hpp).
#pragma once
#include <cstdint>
#include <vector>

#include "wf_hip.h"
#include "wf_cq_sizes.hpp"

namespace wf::host {

// the third-octave band edges (IEC 61260-1, base ten) in bins of an n-point transform; returns the mask of the bands that lie
// wholly inside a spectrum of m bins (wf_hip_bands::covered, wf_hip_stereo::covered)
uint32_t third_octave_edges(uint32_t sample_rate, uint32_t n, uint32_t m, double edges[WF_HIP_NUM_BANDS + 1]);

// WF_HIP_OUT_BANDS (wf_bands.hpp) of an N-point transform with M bins per row
struct BandsTables {
    std::vector<double> edges;   // [WF_HIP_NUM_BANDS + 1] the band edges in bins
    std::vector<double> weights; // [M][2] the squared A and C weights of every bin (IEC 61672-1)
    uint32_t covered = 0;
    double enbw = 1.0;           // the window's equivalent noise bandwidth in bins (an empty window: none, 1)
};
BandsTables bands_tables(uint32_t sample_rate, uint32_t N, uint32_t M, const std::vector<float> &window);

// the stereo image's window: the largest power of two <= min(fft_size, WF_HIP_STEREO_MAX_WINDOW) (<= ring_cap)
uint32_t stereo_window(uint32_t fft_size);

// WF_HIP_OUT_STEREO (wf_stereo.hpp): the periodic Hann window and the twiddles e^(-j 2 pi m / P) in float64, the band edges in
// bins of P and which bands lie wholly inside the spectrum
struct StereoTables {
    uint32_t P = 0, log2p = 0;
    uint32_t covered = 0;
    std::vector<double> tab; // one block [P window][P / 2 twiddles, re im][WF_HIP_NUM_BANDS + 1 edges]
};
StereoTables stereo_tables(uint32_t sample_rate, uint32_t N);

// WF_HIP_OUT_CQ (wf_cq.hpp): L_b, which bins are covered and resolved, and per covered bin the constants of the table above --
// the carrier e^(-j 2 pi f_b n / sr) and the window's phasor e^(j 2 pi n / L_b) at n = 0 .. 63 and their steps of 64 frames, from
// long double arguments so that the device's recurrence starts from correctly rounded values -- and the order in which the
// kernel's waves take the bins
struct CqTables {
    uint32_t max_window = 0; // Lmax = min(ring_cap, WF_HIP_CQ_MAX_WINDOW)
    uint32_t end_covered = 0, first_resolved = 0;
    std::vector<double> tab;     // [end_covered][WF_CQ_BIN_DOUBLES]
    std::vector<uint32_t> sched; // [WF_CQ_SCHED_WORDS]
};
CqTables cq_tables(uint32_t sample_rate, uint32_t ring_cap);

// WF_HIP_OUT_SONO (wf_sono.hpp), P = WF_HIP_SONO_WINDOW: the periodic Hann window and the twiddles e^(-j 2 pi m / P) in float64,
// from long double arguments; the edges 62.5 * 2^(j / 8) Hz of the 64 bands in bins of P; how many columns the ring holds
// (T = min(WF_HIP_SONO_COLUMNS, (ring_cap - P) / H), 0 for a ring that holds no column) and which bands the spectrum covers.
// WF_HIP_OUT_ONSET (wf_onset.hpp) runs on the same columns and takes `tab` as it is; it counts its own columns (setup_onset)
struct SonoTables {
    uint32_t columns = 0;
    uint32_t first_covered = 0, end_covered = 0;
    std::vector<double> tab; // one block [P window][P / 2 twiddles, re im][WF_HIP_SONO_BANDS + 1 edges]
};
SonoTables sono_tables(uint32_t sample_rate, uint32_t ring_cap);

// the distortion analyser's window: the largest power of two <= min(fft_size, WF_HIP_THD_MAX_WINDOW) (<= ring_cap)
uint32_t thd_window(uint32_t fft_size);

// WF_HIP_OUT_THD and WF_HIP_OUT_IMD (wf_thd.hpp, wf_imd.hpp): the periodic 7-term Blackman-Harris taper and the twiddles e^(-j 2 pi m / P) in float64, from long
// double arguments, and S = P sum w^2 / 4, the lobe power of a sine of amplitude 1 (the sample rate changes none of them)
struct ThdTables {
    uint32_t P = 0, log2p = 0;
    double S = 0.0;
    std::vector<double> tab; // one block [P taper][P / 2 twiddles, re im]
};
ThdTables thd_tables(uint32_t sample_rate, uint32_t N);

// the delay finder's window: the largest power of two <= min(fft_size, WF_HIP_DELAY_MAX_WINDOW) (<= ring_cap)
uint32_t delay_window(uint32_t fft_size);

// WF_HIP_OUT_DELAY (wf_delay.hpp): the periodic Hann taper and the twiddles e^(-j 2 pi m / P) in float64, from long double
// arguments
struct DelayTables {
    uint32_t P = 0, log2p = 0;
    std::vector<double> tab; // one block [P taper][P / 2 twiddles, re im]
};
DelayTables delay_tables(uint32_t N);

// WF_HIP_OUT_XFER (wf_xfer.hpp) and WF_HIP_OUT_IMPULSE (wf_impulse.hpp): the segment length P, the largest power of two <= min(fft_size, WF_HIP_XFER_MAX_WINDOW,
// ring_cap / 8), and the number of half-overlapped segments K = min(WF_HIP_XFER_MAX_SEGMENTS, 2 ring_cap / P - 3), at least 13: with
// the P / 4 frames of slack on either side and the up to P / 2 - 1 frames behind the anchor they span at most ring_cap - 1 frames.
// Its tables are delay_tables(P)
uint32_t xfer_window(uint32_t fft_size, uint32_t ring_cap);
uint32_t xfer_segments(uint32_t P, uint32_t ring_cap);

// WF_HIP_OUT_TEMPO (wf_tempo.hpp): how many strength columns the ring holds, T = min(WF_HIP_TEMPO_COLUMNS, (ring_cap - P) / H - 1),
// and the lags searched, lag_lo = ceil(60 sr / (240 H)) .. lag_hi = min(floor(60 sr / (40 H)), T / 4, WF_HIP_TEMPO_MAX_LAG), in
// integer arithmetic.  columns == 0: the ring holds fewer than WF_HIP_TEMPO_MIN_RING frames.  served(): the output exists
struct TempoPlan {
    uint32_t columns = 0;
    uint32_t lag_lo = 0, lag_hi = 0;
    bool served() const { return columns != 0 && lag_hi >= lag_lo + 2; }
};
TempoPlan tempo_plan(uint32_t sample_rate, uint32_t ring_cap);

// ... and the preference w[L] = exp(-0.5 log2(bpm(L) / 120)^2), bpm(L) = 60 sr / (H L), for L = 1 .. WF_HIP_TEMPO_MAX_LAG (w[0] = 0).
// The window, twiddles and band edges of its columns are sono_tables(...).tab
struct TempoTables {
    TempoPlan plan;
    std::vector<double> prior; // [WF_HIP_TEMPO_MAX_LAG + 1]
};
TempoTables tempo_tables(uint32_t sample_rate, uint32_t ring_cap);

// WF_HIP_OUT_HUM (wf_hum.hpp): the decimation D = the largest power of two with 1280 D <= sample_rate, the window N = min(ring_cap,
// WF_HIP_HUM_MAX_WINDOW, 1024 D), M = N / D points per transform, K = ceil(8 * 60.5 N / sr) + 22 bins beside bin -1, the bins
// noise_lo = ceil(20 N / sr) .. noise_hi = floor(484 N / sr) of the noise floor, and the bins lo[i] .. hi[i] searched for harmonic
// h = 1 + i % 8 of family 50 (i < 8) or 60: max(ceil(h (fam - 0.5) N / sr - 0.5), 6) .. floor(h (fam + 0.5) N / sr + 0.5), all in
// integer arithmetic.  served(): the output exists (D >= 2 and bins of at most 3 Hz); too_fast(): no ring would do
struct HumPlan {
    uint32_t D = 0, N = 0, M = 0, log2m = 0, K = 0;
    uint32_t noise_lo = 0, noise_hi = 0;
    uint32_t lo[2 * WF_HIP_HUM_HARMONICS] = {}, hi[2 * WF_HIP_HUM_HARMONICS] = {};
    double hz = 0.0;
    bool fits = false, any_ring = false;
    bool served() const { return fits; }
    bool too_fast() const { return !any_ring; }
};
HumPlan hum_plan(uint32_t sample_rate, uint32_t ring_cap);

// ... and its tables: the twiddles e^(-j 2 pi m / M) of the M-point transform, the combination twiddles W_N^(r k) =
// e^(-j 2 pi r k / N) for r < D and k = -1 .. K as comb[r (K + 2) + k + 1], both in float64 from long double arguments reduced
// modulo the period, and the search ranges as words: ranges[i] = lo[i], ranges[16 + i] = hi[i]
struct HumTables {
    HumPlan plan;
    std::vector<double> tw;       // [M / 2][2]
    std::vector<double> comb;     // [D][K + 2][2]
    std::vector<uint32_t> ranges; // [2][2 * WF_HIP_HUM_HARMONICS]
};
HumTables hum_tables(uint32_t sample_rate, uint32_t ring_cap);

} // namespace wf::host
