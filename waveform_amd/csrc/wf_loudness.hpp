// wf_loudness.hpp -- gfx950 kernels of the loudness producer (include/wf_hip.h, "loudness"; device code only; hipcc; included
// by wf_hip_measure.hip alone).
//
//   loudness_push_kernel<CapCh>   runs behind every push, once the write positions have advanced: measures the frames the
//                                 push appended, ring[wpos - n, wpos) of each captured channel
//   loudness_read_kernel          turns the state into wf_hip_loudness (wf_hip_read(WF_HIP_OUT_LOUDNESS))
//
// Push kernel.  One workgroup per stream, one wavefront per captured channel.  The packet goes through LDS in tiles of at most
// LOUD_TILE frames (and at most one sub-block, so a tile completes at most one).  Each tile is split into 64 contiguous chunks,
// one per lane.  The two K-weighting biquads (direct form II transposed) are one linear recurrence in 4 states,
// s' = A s + B x: every lane runs its chunk from the zero state (lane 0 from the carried state), a wave scan composes the
// chunks (v_i += A^(dL) v_(i-d), squaring A^L per step), and every lane then re-filters its chunk from its true initial
// state, adding y^2 into the (at most two) sub-blocks the chunk covers and running the 4-phase true-peak FIR over the
// LDS-resident samples.  Wave sums use a fixed butterfly; the channels are added in channel order; thread 0 closes the
// completed sub-block (ring of the last 30 energies, both histograms).  The K-weighting runs in float64: in float32 the
// high-pass (poles near z = 1) loses the output of signals whose energy lies mostly below 38 Hz to cancellation -- several
// LU on Brownian noise against the float64 reference.  Samples, y^2 sums, the FIR and the sub-block energies are float32,
// the histograms' energy sums float64.  No atomics: the same packets give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "wf_hip.h"
#include "wf_loudness_tables.hpp"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

constexpr uint32_t LOUD_TILE = 1024; // frames per LDS tile (16 per lane)

// per-stream state (device memory, zeroed by enable / reset)
struct LoudState {
    double filt[2][4];                // K-weighting state per channel: shelf s1, s2, high-pass s1, s2
    float hist[2][LOUD_TAPS];         // the last LOUD_HISTORY input samples per channel, oldest first (the last word unused)
    float sub[LOUD_SUBS];             // energy (sum over channels of sum y^2) of the last 30 completed sub-blocks, slot k % 30
    float partial;                    // energy of the sub-block in progress
    float peak;                       // largest |sample| / |oversampled value| since enable / reset
    uint32_t nsub;                    // sub-blocks completed since enable / reset
    uint32_t pos;                     // frames into the sub-block in progress
    unsigned long long frames;        // frames measured since enable / reset
};

// gating set: blocks with L in [-70 + 0.1 b, -70 + 0.1 (b + 1)) in bin b (the last bin takes everything above)
struct LoudHist {
    double energy[LOUD_BINS];         // sum of the blocks' mean-square energies
    uint32_t count[LOUD_BINS];
};

struct LoudPushArgs {
    RingView rings;                   // (wpos: already advanced past the push)
    const uint32_t *frames_per_stream; // ragged pushes: [count] (capped at `frames`), else nullptr
    LoudState *state;
    LoudHist *hist;                   // [n_streams][2]: integrated, range
    uint32_t first, frames;
    LoudCoefs k;
};

#define WF_LOUD_DEV __device__ __forceinline__

// one step of the K-weighting cascade: state s (shelf s1, s2, high-pass s1, s2), input x -> output
WF_LOUD_DEV double k_step(const LoudCoefs &k, double s[4], double x)
{
    const double y1 = __builtin_fma(k.shelf[0], x, s[0]);
    s[0] = __builtin_fma(k.shelf[1], x, __builtin_fma(-k.shelf[3], y1, s[1]));
    s[1] = __builtin_fma(k.shelf[2], x, -k.shelf[4] * y1);
    const double y = __builtin_fma(k.hpf[0], y1, s[2]);
    s[2] = __builtin_fma(k.hpf[1], y1, __builtin_fma(-k.hpf[3], y, s[3]));
    s[3] = __builtin_fma(k.hpf[2], y1, -k.hpf[4] * y);
    return y;
}

WF_LOUD_DEV float loud_lufs(float ms) { return -0.691f + 10.0f * __builtin_log10f(ms); } // log10(0) = -inf

// thread 0: sub-block energy e (sum over channels of sum y^2) completed
WF_LOUD_DEV void loud_close(LoudState &st, LoudHist *hist, uint32_t sub_frames, float e)
{
    st.sub[st.nsub % LOUD_SUBS] = e;
    const uint32_t n = ++st.nsub;
#pragma unroll
    for(int w = 0; w < 2; ++w) {
        const uint32_t len = w == 0 ? 4u : LOUD_SUBS;
        if(n < len)
            continue;
        float sum = 0.0f;
        for(uint32_t j = n - len; j < n; ++j) // oldest first
            sum += st.sub[j % LOUD_SUBS];
        const float ms = sum / (float)(len * sub_frames);
        const float L = loud_lufs(ms);
        if(!(L > LOUD_GATE_ABS))
            continue;
        const int b = (int)((L - LOUD_GATE_ABS) * (1.0f / LOUD_BIN_LU));
        const uint32_t bin = b < 0 ? 0u : b >= (int)LOUD_BINS ? LOUD_BINS - 1 : (uint32_t)b;
        hist[w].count[bin] += 1u;
        hist[w].energy[bin] += (double)ms;
    }
}

template<uint32_t CapCh>
__global__ __launch_bounds__(64 * CapCh) void loudness_push_kernel(LoudPushArgs a)
{
    __shared__ float xs[CapCh][LOUD_HISTORY + LOUD_TILE];
    __shared__ float red[CapCh][3];
    const uint32_t s = blockIdx.x, stream = a.first + s;
    const uint32_t ch = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t n = a.frames_per_stream ? min(a.frames_per_stream[s], a.frames) : a.frames;
    if(n == 0)
        return;
    LoudState &st = a.state[stream];
    LoudHist *hist = a.hist + (size_t)stream * 2;
    const float *row = channel_ring(a.rings, stream, ch, CapCh);
    const uint32_t start = window_start(a.rings, stream, n), mask = a.rings.ring_cap - 1u; // (the frames the push appended)
    const uint32_t B = a.k.sub_frames, T = B < LOUD_TILE ? B : LOUD_TILE;
    float *x = xs[ch];
    if(lane < LOUD_HISTORY)
        x[lane] = st.hist[ch][lane];
    double S[4] = {st.filt[ch][0], st.filt[ch][1], st.filt[ch][2], st.filt[ch][3]};
    uint32_t pos = st.pos;
    float partial = st.partial, peak = st.peak; // (thread 0's copies are the ones that count)

    for(uint32_t t0 = 0; t0 < n; t0 += T) {
        const uint32_t m = min(T, n - t0);
        for(uint32_t i = lane; i < m; i += 64)
            x[LOUD_HISTORY + i] = row[(start + t0 + i) & mask];
        __syncthreads();
        const uint32_t L = (m + 63u) >> 6;
        const uint32_t c0 = min(lane * L, m), c1 = min(c0 + L, m);
        // zero-state end state of the chunk (lane 0: from the carried state)
        double z[4];
#pragma unroll
        for(int j = 0; j < 4; ++j)
            z[j] = lane == 0 ? S[j] : 0.0;
        for(uint32_t i = c0; i < c1; ++i)
            (void)k_step(a.k, z, x[LOUD_HISTORY + i]);
        // P = A^L: the zero-input response of each unit state after L steps (column j)
        double P[4][4];
#pragma unroll
        for(int j = 0; j < 4; ++j) {
            double e[4] = {0.0, 0.0, 0.0, 0.0};
            e[j] = 1.0;
            for(uint32_t i = 0; i < L; ++i)
                (void)k_step(a.k, e, 0.0);
#pragma unroll
            for(int r = 0; r < 4; ++r)
                P[r][j] = e[r];
        }
        // inclusive scan over the lanes: z_i := end state of chunk i (exact for every chunk of full length L)
#pragma unroll
        for(uint32_t d = 1; d < 64; d <<= 1) {
            double u[4];
#pragma unroll
            for(int j = 0; j < 4; ++j)
                u[j] = __shfl_up(z[j], d, 64);
            if(lane >= d) {
#pragma unroll
                for(int r = 0; r < 4; ++r)
                    z[r] = __builtin_fma(P[r][0], u[0], __builtin_fma(P[r][1], u[1], __builtin_fma(P[r][2], u[2], __builtin_fma(P[r][3], u[3], z[r]))));
            }
            double Q[4][4];
#pragma unroll
            for(int r = 0; r < 4; ++r)
#pragma unroll
                for(int c = 0; c < 4; ++c)
                    Q[r][c] = __builtin_fma(P[r][0], P[0][c], __builtin_fma(P[r][1], P[1][c], __builtin_fma(P[r][2], P[2][c], P[r][3] * P[3][c])));
#pragma unroll
            for(int r = 0; r < 4; ++r)
#pragma unroll
                for(int c = 0; c < 4; ++c)
                    P[r][c] = Q[r][c];
        }
        // this chunk's initial state: the previous chunk's end state
        double v[4];
#pragma unroll
        for(int j = 0; j < 4; ++j) {
            const double prev = __shfl_up(z[j], 1, 64);
            v[j] = lane == 0 ? S[j] : prev;
        }
        // re-filter: energy split at the sub-block boundary (tile frame q), true peak over the 4 phases and the samples
        const uint32_t q = pos + m >= B ? B - pos : m;
        float ea = 0.0f, eb = 0.0f, pk = 0.0f;
        for(uint32_t i = c0; i < c1; ++i) {
            const float xi = x[LOUD_HISTORY + i];
            const float y = (float)k_step(a.k, v, (double)xi);
            if(i < q)
                ea = __builtin_fmaf(y, y, ea);
            else
                eb = __builtin_fmaf(y, y, eb);
            pk = __builtin_fmaxf(pk, __builtin_fabsf(xi));
#pragma unroll
            for(uint32_t r = 0; r < LOUD_PHASES; ++r) {
                float acc = 0.0f;
#pragma unroll
                for(uint32_t t = 0; t < LOUD_TAPS; ++t)
                    acc = __builtin_fmaf(a.k.fir[r][t], x[LOUD_HISTORY + i - t], acc);
                pk = __builtin_fmaxf(pk, __builtin_fabsf(acc));
            }
        }
        // the carried state: the end state of the lane that holds the tile's last frame
        const int last = (int)((m - 1u) / L);
#pragma unroll
        for(int j = 0; j < 4; ++j)
            S[j] = __shfl(v[j], last, 64);
        ea = wave_sum<WAVE_UP>(ea);
        eb = wave_sum<WAVE_UP>(eb);
        pk = wave_max<WAVE_UP>(pk);
        if(lane == 0) {
            red[ch][0] = ea;
            red[ch][1] = eb;
            red[ch][2] = pk;
        }
        // the next tile's history: the last LOUD_HISTORY samples so far (one wave reads before it writes)
        const float keep = lane < LOUD_HISTORY ? x[m + lane] : 0.0f;
        __syncthreads();
        if(lane < LOUD_HISTORY)
            x[lane] = keep;
        if(threadIdx.x == 0) {
            float Ea = red[0][0], Eb = red[0][1], Pk = red[0][2];
#pragma unroll
            for(uint32_t c = 1; c < CapCh; ++c) {
                Ea += red[c][0];
                Eb += red[c][1];
                Pk = __builtin_fmaxf(Pk, red[c][2]);
            }
            peak = __builtin_fmaxf(peak, Pk);
            if(pos + m >= B) {
                loud_close(st, hist, B, partial + Ea);
                partial = Eb;
            } else {
                partial += Ea;
            }
        }
        pos = pos + m >= B ? pos + m - B : pos + m;
        __syncthreads(); // red and the tile buffer are free again
    }
    if(lane == 0)
#pragma unroll
        for(int j = 0; j < 4; ++j)
            st.filt[ch][j] = S[j];
    if(lane < LOUD_HISTORY)
        st.hist[ch][lane] = x[lane];
    if(threadIdx.x == 0) {
        st.partial = partial;
        st.peak = peak;
        st.pos = pos;
        st.frames += n;
    }
}

// one wavefront per stream: state -> wf_hip_loudness
__global__ __launch_bounds__(64) void loudness_read_kernel(const LoudState *state, const LoudHist *hists, wf_hip_loudness *out,
                                                           uint32_t first, uint32_t sub_frames)
{
    constexpr uint32_t PER_LANE = (LOUD_BINS + 63) / 64;
    const uint32_t stream = first + blockIdx.x, lane = threadIdx.x;
    const LoudState &st = state[stream];
    const float ninf = -__builtin_inff();
    const uint32_t b0 = min(lane * PER_LANE, LOUD_BINS), b1 = min(b0 + PER_LANE, LOUD_BINS);
    float gated[2], pct[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    bool any_range = false;
#pragma unroll
    for(int w = 0; w < 2; ++w) {
        const LoudHist &hg = hists[(size_t)stream * 2 + w];
        double e = 0.0;
        uint32_t c = 0;
        for(uint32_t b = b0; b < b1; ++b) {
            e += hg.energy[b];
            c += hg.count[b];
        }
        e = wave_sum<WAVE_UP>(e);
        c = wave_sum<WAVE_UP>(c);
        gated[w] = ninf;
        if(c == 0)
            continue;
        // relative gate: -10 LU (integrated) / -20 LU (range) below the mean of the set; a bin passes when its centre is above
        const double gate = -0.691 + 10.0 * log10(e / c) - (w == 0 ? 10.0 : 20.0);
        double e2 = 0.0;
        uint32_t c2 = 0;
        for(uint32_t b = b0; b < b1; ++b)
            if(LOUD_GATE_ABS + LOUD_BIN_LU * (b + 0.5) > gate) {
                e2 += hg.energy[b];
                c2 += hg.count[b];
            }
        const uint32_t mine = c2;
        e2 = wave_sum<WAVE_UP>(e2);
        c2 = wave_sum<WAVE_UP>(c2);
        if(c2 == 0)
            continue;
        gated[w] = (float)(-0.691 + 10.0 * log10(e2 / c2));
        if(w == 0)
            continue;
        // range: nearest-rank P10 and P95 (rank ceil(p N)) over the gated bins, each as its bin's centre
        uint32_t incl = mine; // inclusive prefix of the lanes' gated counts
#pragma unroll
        for(uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(incl, d, 64);
            if(lane >= d)
                incl += u;
        }
        const uint32_t ranks[2] = {(uint32_t)ceil(0.10 * c2), (uint32_t)ceil(0.95 * c2)};
#pragma unroll
        for(int p = 0; p < 2; ++p) {
            const uint32_t rank = ranks[p] == 0 ? 1u : ranks[p];
            float found = 0.0f;
            if(incl - mine < rank && rank <= incl) {
                uint32_t cum = incl - mine;
                for(uint32_t b = b0; b < b1; ++b)
                    if(LOUD_GATE_ABS + LOUD_BIN_LU * (b + 0.5) > gate) {
                        cum += hg.count[b];
                        if(cum >= rank) {
                            found = LOUD_GATE_ABS + LOUD_BIN_LU * (b + 0.5f);
                            break;
                        }
                    }
            }
            pct[1][p] = wave_sum<WAVE_UP>(found); // (exactly one lane holds it)
        }
        any_range = true;
    }
    if(lane == 0) {
        wf_hip_loudness r;
        float m4 = 0.0f, m30 = 0.0f;
        const uint32_t n = st.nsub;
        if(n >= 4)
            for(uint32_t j = n - 4; j < n; ++j)
                m4 += st.sub[j % LOUD_SUBS];
        if(n >= LOUD_SUBS)
            for(uint32_t j = n - LOUD_SUBS; j < n; ++j)
                m30 += st.sub[j % LOUD_SUBS];
        r.momentary = n >= 4 ? loud_lufs(m4 / (float)(4u * sub_frames)) : ninf;
        r.short_term = n >= LOUD_SUBS ? loud_lufs(m30 / (float)(LOUD_SUBS * sub_frames)) : ninf;
        r.integrated = gated[0];
        r.range = any_range ? pct[1][1] - pct[1][0] : 0.0f;
        r.true_peak = st.peak > 0.0f ? 20.0f * __builtin_log10f(st.peak) : ninf;
        r.reserved = 0;
        r.frames = st.frames;
        out[stream] = r;
    }
}

} // namespace wf
