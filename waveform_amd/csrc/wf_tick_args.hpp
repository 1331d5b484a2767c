// wf_tick_args.hpp -- what the host and the tick kernels agree on: the mode and stream-state bits, and the argument structs of
// spectrum_tick_kernel and the large-FFT kernels (BarArgs, BarsOnlyState, MrPlan, TickArgs).  Plain data and constexpr sizes:
// no device helper and no kernel code, so every host translation unit can include it (wf_hip_internal.hpp does).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wf_fft_core.hpp" // cf

namespace wf {

enum : uint32_t {
    WF_MODE_TSMOOTH = 1u << 0,      // m_tsmoothing != NONE
    WF_MODE_FAST_PEAKS = 1u << 1,   // m_fast_peaks
    WF_MODE_STEREO = 1u << 2,       // m_stereo
    WF_MODE_NORMALIZE = 1u << 3,    // m_normalize_volume
    WF_MODE_ROLLOFF = 1u << 4,      // m_rolloff_q > 0 && m_rolloff_rate > 0
    WF_MODE_SLOPE = 1u << 5,        // m_slope > 0
    WF_MODE_WINDOW = 1u << 6,       // m_window_func != NONE
    WF_MODE_MONO_MIX = 1u << 7,     // !m_stereo && m_capture_channels > 1
};

// per-stream state bits kept in HBM between ticks
enum : uint32_t {
    WF_STREAM_LAST_SILENT = 1u << 0, // m_last_silent
    WF_STREAM_HIDDEN = 1u << 1,      // !m_show or capture timed out (host sets it)
    WF_STREAM_TIMEOUT = 1u << 2,     // set with HIDDEN when the cause is the capture timeout: tick_meter treats the two differently
    WF_STREAM_PAUSED = 1u << 4,      // the host did not tick this source in this video frame (WF_HIP_PAUSED): the stream is left exactly as it is
    WF_STREAM_STARVED = 1u << 5,     // the host found fewer samples than window + A/V-sync delay in the source's own buffer (WF_HIP_STARVED):
                                     // the tick takes the kernel's underflow path (no channel processed, the end-of-tick dB pass still runs)
    WF_STREAM_WRAPPED = 1u << 3,     // wpos has wrapped past 2^32 since the last reset: "fewer samples than the A/V-sync delay yet" is over for good
};

// bars or curve (render_bars / render_curve interpolation, filter, dB -> pixel mapping); out == nullptr: neither
struct BarArgs {
    // Per bar b the reference computes (1/count_b) * sum over the band's samples k of sum_t dB[ix_k - r + 1 + t] * W[k][t]
    // (src/filter.hpp:194-211; POINT mode: plain band mean, src/source.cpp:1525-1532).  The samples of a band sit on
    // consecutive bins, so the double sum collapses into ONE dot product per bar over a contiguous bin range, with
    // coefficient = the sum of all tap weights that land on that bin (built on the host in double from the reference's
    // own weight table, taps outside [0, M) dropped as kernel_convolve does): 8x fewer multiplies, 7x smaller table.
    // Flattened over all bars: entry e multiplies dB[bin[e]] by coef[e]; bar b owns entries [off[b], off[b+1]).
    const float *coef;         // [entries]
    const int *bin;            // [entries]
    const int *off;            // [num_bars + 1]
    const int *count;          // [num_bars] m_band_widths
    const int *chunk;          // [num_chunks + 1] bar ranges whose entries fit the LDS scratch together
    // big_outputs_kernel (wf_big.hpp): the entries cut into tasks of at most 2048, one wavefront each -- a bar at the top of a log
    // axis owns half the row, and one wavefront walking it alone was the kernel's whole duration
    const int *big_task;       // [num_tasks][4] bar, first entry, one past the last entry, the first entry's bin where the entries walk consecutive bins (else -1)
    const int *big_bar_task;   // [num_bars + 1] the tasks of bar b: [big_bar_task[b], big_bar_task[b + 1])
    int big_num_tasks;
    // Usual case (bars <= threads per spectrum): every thread owns one segment of the entries -- near-equal lengths,
    // never straddling a bar (the bars' own lengths differ by two orders of magnitude on a log axis) -- with its
    // coefficients laid lane-major: block c of thread s at [(c*T + s)*4, +4), zero-padded, for 4 * lane_blocks consecutive
    // bins from lane_base[s].  Bar b owns
    // segments [bar_seg[b], bar_seg[b+1]).  num_segs == 0: not built, the flat tables above are used chunk by chunk.
    const float *lane_coef;    // [lane_blocks][T][4]
    const int *lane_base;      // [T] first of the segment's 4 * lane_blocks consecutive bins (a multiple of 4: 16-byte LDS reads)
    const int *bar_seg;        // [num_bars + 1]
    const int *seg_group;      // [T] > 0: this segment starts a group of that many (<= 8) consecutive segments of one bar
    // wave-local layout (T > 64, no filter): every bar's segments lie inside one wavefront, so the partials are added with
    // wave-level ordering only -- no workgroup barrier between the dot products and the stores
    const int *lead_bar;       // [T] the bar whose first segment this thread owns, or -1
    const int *lead_end;       // [T] one past that bar's last segment
    int wave_local;
    // wave-private layout (BarPieceTables, wf_host_tables.hpp): seg_group = its `info` words, bar_seg = its `bar_piece`; the
    // segments of a thread read bins its own wavefront parked -- no barrier between parking the row and reading it --, pieces
    // are summed by a DPP prefix scan and the last wavefront to arrive adds the pieces of every bar
    int piece_mode;
    // prefix-sum layout (BarPsTables, wf_host_tables.hpp): every wavefront leaves its part of the row and its four-bin group sums;
    // the first wavefront of the spectrum forms a float64 prefix sum over 16-bin quads and evaluates the sub-bands, two lanes each
    // (one look-up and one 7-tap edge window per lane).  ps_tab: [3][64][4]; ps_lanes: 64, or 0: off
    const float *ps_tab;
    int ps_lanes;
    int num_segs;
    int lane_blocks;
    // Curve display (render_curve, reference src/source.cpp:1360-1425): num_bars = m_width points per row, point
    // o = k*T + s is the dot product of 8 consecutive dB bins starting at cur_base[o] with cur_coef[o][0..8) (the
    // Lanczos / Catmull-Rom taps of that point, clipped to [0, M) as kernel_convolve does; POINT mode: one tap).
    const float *cur_coef;     // [out_steps][T][8]
    const int *cur_base;       // [out_steps][T]
    // Catmull-Rom curve (the plugin's default interpolation, reference src/source.cpp:141): the four weights of a point are
    // a cubic in u = x - floor(x) (make_catrom_kernel, src/filter.hpp:67-104), so the table is the point's position alone --
    // 4 bytes per point instead of 36 -- and the weights are evaluated on the fly in the reference's own operation order.
    const float *cur_x;        // [out_steps rounded up to 4][T] m_interp_indices, lane-major; padding entries hold 1.0f
    int curve;                 // 2: Catmull-Rom curve from cur_x; 1: curve tables above; 0: bar tables
    int out_steps;             // ceil(num_bars / T) when the outputs are finished one per thread and step, else 0
    int both_subs;             // != 0 (curve, mono mixdown, two spectra per workgroup): the threads of both spectra finish the
                               // one displayed row; the tables are laid out for 2 * T threads
    int stream_steps;          // != 0: more steps than a thread's registers hold (wide curves): points are finished as they
                               // are produced -- mapped and stored at once, or staged behind the dB row for the filter
    // Gaussian filter across the outputs before the dB -> pixel mapping (apply_filter / weighted_avg,
    // reference src/filter.hpp:133-157,171-180; kernel make_gauss_kernel :40-65); gauss_radius == 0: off
    const float *gauss;        // [2 * gauss_radius - 1]
    const float *gauss_wsum;   // [num_bars] the sum of the weights whose taps fall inside the row (weighted_avg's divisor)
    int gauss_radius;
    int stage_off;             // chunked bars + filter: float offset (from the dB row in LDS) of the staging area [pad | bars | pad | weights]
#ifdef WF_PHASE_TIMING
    unsigned long long *clk;   // development aid: this workgroup's stamp slots
#endif
    float *out;                // [n_streams][disp_ch][num_bars]
    // mirrored frequency axis (reference src/source.cpp:1559-1564): outputs above the middle are replaced by images of the lower ones
    // AFTER render_bars / render_curve have taken the row's smallest y for the shader (miny / minpos, :1548-1557).  Above the middle
    // every output sits on the clamped top position and has the same value: output num_bars / 2 + 1's goes here, one float per
    // displayed row, so that the host finds the reference's miny without drawing the row itself.  nullptr: not kept
    float *pre_out;            // [n_streams][disp_ch]; inside the kernel's display phase: the entry of the row being finished
    // > 0 (wf_hip_set_bars_mirrors): every tick also leaves the batch's bars -- the ones it finishes and, copied over, the
    // ones it does not touch (paused, hidden or silent streams) -- in out2_n more buffers of the same shape, buffer j starting
    // out2_delta[j] floats behind `out`: the send buffer of the all-gather of BASELINE configs[4] (or, with peer access, this shard's
    // slice of every device's gathered result) written by the kernel instead of by copies behind it
    int out2_n;
    long long out2_delta[8];
    int num_bars;
    int num_chunks;
    int entries;               // total number of entries (= off[num_bars])
    int lanes_per_bar;         // power of two <= 64: threads that share one bar in the segmented sum
    int mirror;
    float border_top, border_bottom;
    float ceiling, dbrange;    // m_ceiling, m_ceiling - m_floor
    float inv_dbrange;         // 1 / dbrange
    int lerp_mixed;            // border_top and border_bottom have opposite signs or one is 0: std::lerp's first form
    uint32_t disp_ch;
};

// State of a handle that runs bars-only ticks, in device memory.  From the first such tick on every wavefront leaves "my
// slice of the row I produced has a value > floor - 10" in row_verdict[spec * (T/64) + wave] and the silence test reads those
// words instead of the rows (use_verdict; 0 on the first such tick, whose rows are still current).  Split mode has its own
// rotating verdict words (TickArgs::verdict_*) and leaves row_verdict null.  stale_row: M values of DB_MIN that stand in for
// the stale row of a skipped channel (wf_kernels.hpp).
struct BarsOnlyState {
    uint32_t *row_verdict;
    const float *stale_row;
    uint32_t use_verdict;
};

// FFT sizes with no prime factor above 5 (wf_mixed.hpp): the passes of the direct n/2-point transform
constexpr int MR_MAX_PASSES = 4;
struct MrPlan {
    int passes;                 // 0: no plan (Bluestein runs)
    int radix[MR_MAX_PASSES];
    int tw_off[MR_MAX_PASSES];  // pass s >= 1: its twiddles start at tw + tw_off[s]
    const cf *wp;               // radix[0] a prime above 25 (mr_pass_prime): [radix[0]] W_p^m in device memory (the tick kernel finds it in
                                // its LDS twiddle area, staged with the other tables; the large-FFT rows kernel copies it there itself)
    const cf *tw;               // per pass [R][Ns]: W_(Ns R)^(k jm), Ns = product of the radices before it (coalesced across a wavefront's butterflies)
    // The spectrum's exchange buffer, sized by the TRANSFORM rather than by the container geometry (wf::mr_exchange_cf): the passes
    // work between its two halves of `half` >= n/2 points, the finished Z[k] sits at (k & 3) * s3 + (k >> 2) -- ex3_addr's
    // four planes with a plane stride that fits n/2 points -- and spectrum s of a workgroup starts at s * lds_cf.  N = 800 on
    // the 2048-sample container: 6.5 instead of 8.7 KB per spectrum.
    int half, s3, lds_cf;
};

struct TickArgs {
    // audio rings: one per (stream, captured channel), ring_cap samples each (power of two)
    const float *ring;
    const uint32_t *wpos;      // [n_streams] samples written so far, modulo 2^32
    uint32_t ring_mask;        // ring_cap - 1
    uint32_t ring_cap;
    uint32_t ring_stride;      // floats between the rings of consecutive (stream, channel) rows (>= ring_cap)
    uint32_t delay;            // frames between the end of the window and wpos (A/V sync, reference :50-51)
    const uint32_t *delay_stream; // [n_streams] added to `delay` per stream (wf_hip_set_stream_delay), or nullptr
    // per-configuration tables (read-only, shared by every stream)
    const float *window;       // [N]; all ones when FFTWindow::NONE
    const cf *tw1;             // [R1][M/R1]   W_M^(n' k1)
    const cf *tw2;             // [R2][R3]     W_(R2 R3)^(n3 k2)
    const cf *tws;             // [M]          W_N^k
    const float *slope;        // [M]; all ones when m_slope <= 0
    const float *rolloff;      // [M]
    // per-spectrum state and outputs
    float *tsmooth;            // [n_streams * cap_ch][M]   m_tsmooth_buf
    float *decibels;           // [n_streams][out_ch][M]    m_decibels
    uint32_t *stream_flags;    // [n_streams] read at the start of the tick; written at its end unless flags_out is set
    // split mode (the channels of a stereo stream in different workgroups, see spectrum_tick_kernel<.., SPLIT>): the words a
    // workgroup writes must not be the ones its partner reads in the same tick, so they rotate through three buffers
    uint32_t *flags_out;       // [n_streams] the flags the next tick reads
    const uint32_t *verdict_in; // [n_streams * cap_ch] != 0: the row left by the previous tick has a value > floor - 10
    uint32_t *verdict_out;     // the same for the rows as this tick leaves them (zero on entry; waves OR into it)
    uint32_t *verdict_clear;   // the buffer the next tick ORs into
    // scalars
    float half_coef;           // 0.5f * (2.0f / m_window_sum)
    float slope_step;          // 3 * m_slope / (M - 1): the slope factor of bin k is 1 + k * slope_step (0: slope off), Policy<G>::SLOPE_LINEAR
    float g, g2;               // get_gravity(seconds), 1 - g
    float vol_comp;            // min(m_volume_target - dbfs(m_input_rms), m_max_gain)
    const float *vol_comp_stream; // [n_streams] the same per stream (wf_hip_set_input_rms), or nullptr: vol_comp for all
    float db_min;              // DB_MIN
    float silent_floor;        // (float)(m_floor - 10)
    uint32_t n_streams;
    uint32_t stream_base, stream_count; // the slice of the batch this launch runs (wf_hip_tick issues the batch as lanes)
    uint32_t cap_ch;           // m_capture_channels (1 or 2)
    uint32_t out_ch;           // m_output_channels
    uint32_t mode;
    uint32_t skip_decibels;    // WF_HIP_TICK_NO_DECIBELS: bars-only batch mode
    // Mono mixdown on a geometry that holds one spectrum per workgroup (N = 32768 and its Bluestein sizes): the tick is two
    // launches of the split kernel -- channel 1 of every stream first (its smoothed magnitudes go to m_decibels[1], where
    // the reference keeps them too, src/source_generic.cpp:134), then channel 0, which mixes them in.  split_ch = the
    // channel this launch runs; 0xffffffff: all channels in one launch.
    uint32_t split_ch;
    // Once a tick of a handle has skipped the row store (WF_HIP_TICK_NO_DECIBELS), m_decibels in HBM is no longer what the
    // silence state machine must inspect (reference :78-86): see BarsOnlyState.  nullptr: rows are always stored (the usual
    // case; one pointer here instead of its fields keeps the kernel's scalar registers free).
    const BarsOnlyState *bars_only;
    const float *stale_row;   // BarsOnlyState::stale_row again, as a kernel argument: a pointer read from memory is a generic one,
                              // and a FLAT load anywhere on a path makes every later wait a wait for everything (see wf_kernels.hpp)
    // FFT sizes that are not powers of two (Bluestein, spectrum_tick_kernel<.., BLU>): the geometry's M is the padded
    // convolution length L, the transform the host asked for has blu_n points and row_bins = blu_n / 2 output bins
    const cf *blu_q;           // [blu_n / 2] conj(w_k) / L: Z_k = blu_q[k] * conj(R_k) for the twice-transformed R
    const cf *blu_qr;          // [blu_n / 2] blu_q[(blu_n / 2 - k) mod (blu_n / 2)]
    const cf *blu_w;           // [blu_n / 2] W_blu_n^k, the real-split twiddles
    MrPlan mr;                 // blu_n = 2^a 3^b 5^c: the transform is computed directly (blu_a, blu_b, blu_q, blu_qr unused)
    uint32_t big_c, big_r;     // big_mr_rows_kernel (wf_big.hpp): the n/2 points as big_c rows of big_r (mr plans a row)
    uint32_t big_rs;           // big_br_*_kernel: the stride of a row in the scratch buffer (big_r rounded up to even)
    const cf *big_wc;          // [8][8] W_big_c^(c k1): the column step of row k1
    const cf *blu_a;           // [2 M] the factors of x_2j and x_2j+1 in point j of the chirped, windowed, packed input; zero from point blu_n / 2 on
    const cf *blu_b;           // [M] FFT_M of the chirp
    uint32_t blu_n;
    uint32_t row_bins;         // bins per output / state row (M >> DEC for the power-of-two paths)
    // transforms beyond a CU's LDS (wf_big.hpp): the finished transform in device memory and what the epilogue needs with it
    const cf *big_z;           // [n_spec][big_l] rows' output, natural order
    const cf *big_tws;         // [big_m] W_(2 big_m)^k (real split of the 65536-sample transform)
    const cf *big_tw;          // [L1][16384] W_L^(n2 k1): the column twiddles (big_whole_kernel / big_mr_rows_kernel fold the column step into their fetch)
    uint32_t *big_nz_out;      // big_nz, writable (row 0 of big_mr_rows_kernel ORs "the window has a non-zero sample" into it)
    const uint32_t *big_nz;    // [n_spec] != 0: the window has a non-zero sample
    uint32_t big_m, big_l;     // complex points of the packed real transform; complex points per transform (scratch stride)
    BarArgs bar;
    unsigned long long *phase_clock; // development aid (builds with -DWF_PHASE_TIMING): s_memtime stamps per workgroup
};

// floats of LDS a spectrum needs in the display's prefix-sum layout (its map: wf_tick_display.hpp, "bars, prefix-sum layout")
constexpr size_t ps_lds_floats(size_t M) { return 8 + M + M / 4 + 2 * (M / 16 + 2); } // (constexpr: host and device)

} // namespace wf
