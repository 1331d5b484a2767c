// wf_hum.hpp -- gfx950 read kernel of WF_HIP_OUT_HUM (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the mains hum detector, per captured channel whether a 50 or a 60 Hz line and its harmonics up to the 8th
// stand above the programme, from bins -1 .. K of the N-point transform of the newest N <= 32768 frames of the rings (the
// definition is in include/wf_hip.h, "mains hum").  wf_hip_read launches it on the handle's stream, behind every push issued so
// far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_HUM_THREADS per stream and captured channel, grid (streams, captured channels).  Only K + 2 <= 412 bins of
// the N are wanted, so the transform is taken apart by decimation in time: X[k] = sum over r < D of W_N^(r k) F_r[k mod M], F_r the
// M-point transform of the branch x[r], x[r + D], ...; two branches go through one complex transform, so a channel costs D / 2
// transforms of M = 512 or 1024 points in one 16 KB region (wf_fft64_lds.hpp's, unchanged) instead of one of N.
//   stage      the newest N frames from the ring into LDS, once, in 16-byte loads of the ring's aligned groups (the window starts
//              at any alignment and may wrap: a group never straddles the ring's end, and the frames of the first and the last
//              group that lie outside the window are dropped).  Branch-major: frame n lies at (n % D) (M + 64 / D) + n / D, so
//              consecutive branches start 64 / D banks apart (M is a multiple of the 64 banks).  The 64 lanes of a load hold 256
//              consecutive frames, and each of its four words is stored by one instruction: lane l = a D / 4 + b writes frame
//              4 l + j, branch 4 b + j, place a, bank (4 b + j) 64 / D + a -- 8 b + a at D = 32 (a, b < 8), 4 b + a at D = 64
//              (a < 4, b < 16), 16 b + a at D = 16, 32 b + a at D = 8: 64 different banks.  (A window that starts o frames into
//              a group turns the pattern by o branches; where that carries a lane into the next place, two lanes may meet.)
//              A strided read of the ring per branch would fetch every 128-byte line D times; a plain copy, or a pad of one
//              word, would put several lanes of a store into one bank.
//   total      thread t adds the squares of frames t, t + 256, ... (consecutive lanes on consecutive frames: branch n % D, the
//              same 64 banks) and notes an exponent of all ones; butterflies, the four waves in order.  Taken from LDS and not
//              on the way in, so that the order of the sum follows from the frames alone and not from where the window starts
//              in the ring.  A window of zeros or one with a NaN or an infinity: the zero record, and the workgroup leaves.
//   transform  D / 2 times: fft64_load16 with a fetch that pairs branches r and r + 1 (consecutive lanes on consecutive words
//              of a branch: no conflicts), fft64_passes.  Thread t owns bins k = t - 1 and t - 1 + 256 up to K: it unpacks
//              A = F_r[k], B = F_(r+1)[k] from Z[k mod M] and Z[-k mod M], multiplies by W_N^(r k) and W_N^((r + 1) k) from the
//              host's table and keeps the running sums in registers (wf_xfer_sums.hpp's pattern).
//   window     X to LDS; H[k] = (0.5 X[k] - 0.25 (X[k - 1] + X[k + 1])) 4 / N, the periodic Hann window applied across
//              frequency; p = |H|^2 and |H| to LDS.
//   lines      the sixteen (family, harmonic) searches on sixteen lanes of wave 0: the largest bin of the range, the peak test,
//              the interpolation, the mains test, and the local floor by exact selection over at most 34 powers (for every one,
//              how many stand before it in the sorted order; the one with n / 2 before it).  Then thread 0: the consensus, the
//              family and the sums in ascending harmonic order.
//   noise      the powers of the bins of noise_db outside the lines into the slots |H| had, -1 elsewhere; every thread ranks its
//              own bins against all of them; the one of rank n / 2 is written by the thread that owns it.
// The order of every sum follows from the plan alone; there are no atomics and no scratch.  The rule runs with the float64
// contraction off (#pragma clang fp contract(off)): comparisons decide the integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_ring_stage.hpp"
#include "wf_wave_reduce.hpp"
#include "wf_fft64_lds.hpp"

namespace wf {

constexpr uint32_t WF_HUM_THREADS = 256;
constexpr uint32_t WF_HUM_WAVES = WF_HUM_THREADS / 64;
constexpr uint32_t WF_HUM_OWN = 2;         // bins per thread
constexpr uint32_t WF_HUM_MAX_BINS = 412;  // K + 2 at hz = 1.25: ceil(484 / 1.25) + 24
constexpr uint32_t WF_HUM_LINES = 2 * WF_HIP_HUM_HARMONICS;
static_assert(WF_HUM_THREADS * WF_HUM_OWN >= WF_HUM_MAX_BINS, "every bin has a thread");
static_assert(WF_HUM_LINES <= 64, "the searches fit one wavefront");

// floats between the branches of the staged window: M and a pad that puts consecutive branches 64 / D banks apart
__host__ __device__ constexpr uint32_t hum_branch_stride(uint32_t D, uint32_t M) { return M + (D <= 64u ? 64u / D : 1u); }

// dynamic LDS: the transform's region [M], X [K + 2], p [K], |H| [K], and the staged window [D][stride]
__host__ __device__ constexpr size_t hum_lds_bytes(uint32_t D, uint32_t M, uint32_t K)
{
    return (size_t)M * sizeof(double2) + ((size_t)K + 2u) * sizeof(double2) + 2u * (size_t)K * sizeof(double)
           + (size_t)D * hum_branch_stride(D, M) * sizeof(float);
}
static_assert(hum_lds_bytes(32, 1024, WF_HUM_MAX_BINS - 2) + 2048 <= WF_LDS_PER_CU, "the largest plan and the hand-overs fit a compute unit");
static_assert(hum_lds_bytes(64, 512, 216) <= hum_lds_bytes(32, 1024, WF_HUM_MAX_BINS - 2));

struct HumArgs {
    RingView rings;
    wf_hip_hum *out;         // [count] the entry of stream `first`
    const double2 *tw;       // [M / 2] e^(-j 2 pi m / M)
    const double2 *comb;     // [D][K + 2] W_N^(r k), k = -1 .. K
    const uint32_t *ranges;  // [2][16] first and last bin searched per (family, harmonic)
    double hz;               // sample_rate / N
    uint32_t first;          // first stream read
    uint32_t channels;       // captured channels: gridDim.y
    uint32_t D, log2d;       // the decimation: a power of two, 2 <= D <= 64
    uint32_t N;              // the window: D M <= min(ring_cap, WF_HIP_HUM_MAX_WINDOW)
    uint32_t M, log2m;       // points per transform: 512 or 1024
    uint32_t K;              // bins kept: hi[15] + 20 < K, K + 1 < M / 2
    uint32_t noise_lo, noise_hi;
};

__device__ __forceinline__ double hum_db(double v) { return 10.0 * log10(fmax(v, 1e-300)); }

// grid: (streams of [first, first + gridDim.x), captured channels); dynamic LDS: hum_lds_bytes(D, M, K)
__global__ __launch_bounds__(WF_HUM_THREADS) void hum_read_kernel(const HumArgs a)
{
    extern __shared__ __align__(16) double2 hum_lds[];
    // the hand-overs, each written once
    __shared__ double part_sum[WF_HUM_WAVES];
    __shared__ uint32_t part_bits[WF_HUM_WAVES];
    __shared__ double line_f[WF_HUM_LINES], line_amp[WF_HUM_LINES], line_snr[WF_HUM_LINES];
    __shared__ uint32_t line_k[WF_HUM_LINES]; // (~0: no qualified line)
    __shared__ uint32_t kept_k[WF_HIP_HUM_HARMONICS];
    __shared__ double noise_v;

    constexpr uint32_t T = WF_HUM_THREADS, NH = WF_HIP_HUM_HARMONICS;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x, c = blockIdx.y;
    const uint32_t D = a.D, N = a.N, M = a.M, K = a.K, cb = a.log2m - 4u, ld = a.log2d, dm = D - 1u;
    const uint32_t S = hum_branch_stride(D, M);
    double2 *z = hum_lds;
    double2 *xs = z + M;                                   // X[k] at xs[k + 1]
    double *pw = reinterpret_cast<double *>(xs + K + 2u);  // p[k]
    double *mag = pw + K;                                  // |H[k]|, later the noise floor's candidates
    float *stage = reinterpret_cast<float *>(mag + K);     // frame n at (n % D) S + n / D
    wf_hip_hum *out = a.out + blockIdx.x;
    const auto slot = [&](uint32_t n) { return (n & dm) * S + (n >> ld); };

    // stage: the aligned groups that cover ring positions [s, s + N), frame n = 4 i + j - o of group i
    {
        const float *ring = channel_ring(a.rings, stream, c, a.channels);
        const uint32_t mask = a.rings.ring_cap - 1u;
        const uint32_t s = window_start(a.rings, stream, N), o = s & 3u, base = s - o;
        const uint32_t groups = N / 4u + (o != 0u ? 1u : 0u);
        const auto fetch = [&](uint32_t i) { return *reinterpret_cast<const float4 *>(ring + ((base + 4u * i) & mask)); };
        const auto put = [&](uint32_t i, float4 v) {
            const uint32_t n = 4u * i - o; // (wraps below 0 for the frames in front of the window: they fail n < N)
            if(n < N)
                stage[slot(n)] = v.x;
            if(n + 1u < N)
                stage[slot(n + 1u)] = v.y;
            if(n + 2u < N)
                stage[slot(n + 2u)] = v.z;
            if(n + 3u < N)
                stage[slot(n + 3u)] = v.w;
        };
        constexpr uint32_t U = 4;
        uint32_t i = t;
        for(; i + (U - 1u) * T < groups; i += U * T) {
            float4 v[U];
#pragma unroll
            for(uint32_t u = 0; u < U; ++u)
                v[u] = fetch(i + u * T);
#pragma unroll
            for(uint32_t u = 0; u < U; ++u)
                put(i + u * T, v[u]);
        }
        for(; i < groups; i += T)
            put(i, fetch(i));
    }
    __syncthreads();

    // total: the mean square's sum, and whether any sample is a NaN or an infinity
    double total;
    bool valid;
    {
        double ss = 0.0;
        uint32_t top = 0u;
        for(uint32_t n = t; n < N; n += T) {
            const float x = stage[slot(n)];
            top |= (uint32_t)((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u);
            ss += (double)x * (double)x; // (exact: 48 bits)
        }
        ss = wave_sum(ss);
        const bool wt = __ballot(top != 0u) != 0ull;
        if(lane == 0u) {
            part_sum[wave] = ss;
            part_bits[wave] = wt ? 1u : 0u;
        }
        __syncthreads();
        total = part_sum[0];
        uint32_t bad = part_bits[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_HUM_WAVES; ++w) {
            total += part_sum[w];
            bad |= part_bits[w];
        }
        valid = bad == 0u && total > 0.0;
    }
    const auto header = [&]() {
        if(c == 0u) {
            out->window = N;
            out->decimation = D;
            out->resolution_hz = (float)a.hz;
            out->reserved = 0u;
            if(a.channels == 1u)
                out->ch[1] = wf_hip_hum_channel{};
        }
    };
    if(!valid) { // (uniform: every thread holds the same sum and bits)
        if(t == 0u) {
            out->ch[c] = wf_hip_hum_channel{};
            header();
        }
        return;
    }

    // transform: X[k] = sum over r of W_N^(r k) F_r[k mod M], the branches in pairs
    double2 acc[WF_HUM_OWN];
    uint32_t km[WF_HUM_OWN], kn[WF_HUM_OWN];
#pragma unroll
    for(uint32_t u = 0; u < WF_HUM_OWN; ++u) {
        acc[u] = make_double2(0.0, 0.0);
        km[u] = (t + u * T - 1u) & (M - 1u); // k mod M, k = t + u T - 1 (M - 1 for k = -1)
        kn[u] = (M - km[u]) & (M - 1u);      // -k mod M
    }
    const size_t bins = (size_t)K + 2u;
#pragma unroll 1
    for(uint32_t r = 0; r < D; r += 2u) {
        __syncthreads(); // whoever read the region last is done with it
        const float *b0 = stage + r * S, *b1 = b0 + S;
        fft64_load16(z, a.tw, t, M, cb, [&](uint32_t i) { return make_double2((double)b0[i], (double)b1[i]); });
        fft64_passes<T>(z, a.tw, t, M, cb, fft64_block_sync{});
#pragma unroll
        for(uint32_t u = 0; u < WF_HUM_OWN; ++u) {
            const uint32_t i = t + u * T;
            if(i < bins) {
                const double2 p = z[fft64_at(km[u], cb)], q = z[fft64_at(kn[u], cb)];
                const double2 A = make_double2(0.5 * (p.x + q.x), 0.5 * (p.y - q.y));  // (Z[k] + conj Z[-k]) / 2
                const double2 B = make_double2(0.5 * (p.y + q.y), -0.5 * (p.x - q.x)); // (Z[k] - conj Z[-k]) / 2j
                acc[u] = fft64_add(acc[u], fft64_add(fft64_mul(a.comb[r * bins + i], A), fft64_mul(a.comb[(r + 1u) * bins + i], B)));
            }
        }
    }
#pragma unroll
    for(uint32_t u = 0; u < WF_HUM_OWN; ++u)
        if(t + u * T < bins)
            xs[t + u * T] = acc[u];
    __syncthreads();

    // window: the periodic Hann window across frequency
    {
        const double scale = 4.0 / (double)N;
        for(uint32_t k = t; k < K; k += T) {
            const double2 l = xs[k], m = xs[k + 1u], h = xs[k + 2u];
            const double re = (0.5 * m.x - 0.25 * (l.x + h.x)) * scale, im = (0.5 * m.y - 0.25 * (l.y + h.y)) * scale;
            const double p = re * re + im * im;
            pw[k] = p;
            mag[k] = sqrt(p);
        }
    }
    __syncthreads();

    // lines: one (family, harmonic) per lane
    if(t < WF_HUM_LINES) {
#pragma clang fp contract(off)
        const uint32_t lo = a.ranges[t], hi = a.ranges[WF_HUM_LINES + t];
        const double h = (double)(1u + (t & (NH - 1u))), fam = t < NH ? 50.0 : 60.0;
        uint32_t found = ~0u;
        double f = 0.0, amp = 0.0, snr = 0.0;
        if(hi >= lo) {
            uint32_t k = lo;
            double peak = mag[lo];
            for(uint32_t j = lo + 1u; j <= hi; ++j) {
                const double v = mag[j];
                if(v > peak) { // (the lowest bin of equal values)
                    peak = v;
                    k = j;
                }
            }
            const double below = mag[k - 1u], above = mag[k + 1u]; // (k >= 6, k + 1 < K)
            if(peak > below && peak >= above) {
                const double alpha = fmax(below, above) / peak;
                const double d = fmin(fmax((2.0 * alpha - 1.0) / (alpha + 1.0), 0.0), 0.5);
                amp = d > 0.0 ? peak * (1.0 - d * d) * (M_PI * d) / sinpi(d) : peak;
                f = ((double)k + (below > above ? -d : d)) * a.hz / h;
                if(fabs(f - fam) <= WF_HIP_HUM_TOL_HZ) {
                    // the local floor: [max(2, k - 20), max(2, k - 3)) and [k + 4, k + 21)
                    const uint32_t l0 = k > WF_HIP_HUM_FLOOR_SPAN + 2u ? k - WF_HIP_HUM_FLOOR_SPAN : 2u;
                    const uint32_t l1 = k > WF_HIP_HUM_FLOOR_GUARD + 2u ? k - WF_HIP_HUM_FLOOR_GUARD : 2u;
                    const uint32_t n1 = l1 - l0, n = n1 + (WF_HIP_HUM_FLOOR_SPAN - WF_HIP_HUM_FLOOR_GUARD);
                    const auto at = [&](uint32_t i) { return pw[i < n1 ? l0 + i : k + WF_HIP_HUM_FLOOR_GUARD + 1u + (i - n1)]; };
                    double floor_p = 0.0;
                    for(uint32_t i = 0; i < n; ++i) {
                        const double vi = at(i);
                        uint32_t before = 0u;
                        for(uint32_t j = 0; j < n; ++j) {
                            const double vj = at(j);
                            before += (uint32_t)(vj < vi || (vj == vi && j < i));
                        }
                        if(before == n / 2u)
                            floor_p = vi;
                    }
                    floor_p = fmax(floor_p / M_LN2, 1e-300);
                    snr = 10.0 * log10(amp * amp / floor_p);
                    if(snr >= WF_HIP_HUM_MARGIN_DB)
                        found = k;
                }
            }
        }
        line_k[t] = found;
        line_f[t] = f;
        line_amp[t] = amp;
        line_snr[t] = snr;
    }
    __syncthreads();

    // family: the consensus and the sums in ascending harmonic order (thread 0; the others only learn which bins the lines hold)
    uint32_t win = ~0u, win_mask = 0u; // the winning family's first row of line_*, its remaining harmonics
    double win_f0 = 0.0, win_hum = 0.0, win_odd = 0.0, win_even = 0.0;
    if(t == 0u) {
#pragma clang fp contract(off)
#pragma unroll
        for(uint32_t fi = 0; fi < 2u; ++fi) {
            double sw = 0.0, sf = 0.0;
            for(uint32_t i = 0; i < NH; ++i) {
                const uint32_t row = fi * NH + i;
                if(line_k[row] != ~0u) {
                    const double g = (double)(i + 1u) * line_amp[row], w = g * g;
                    sw += w;
                    sf += w * line_f[row];
                }
            }
            if(sw > 0.0) {
                const double f0 = sf / sw;
                double hum = 0.0, odd = 0.0, even = 0.0;
                uint32_t m = 0u;
                for(uint32_t i = 0; i < NH; ++i) {
                    const uint32_t row = fi * NH + i;
                    if(line_k[row] != ~0u && fabs(line_f[row] - f0) * (double)(i + 1u) <= a.hz) {
                        const double v = line_amp[row] * line_amp[row] / 2.0;
                        hum += v;
                        if((i & 1u) != 0u) // h = i + 1 even
                            even += v;
                        else if(i >= 2u)
                            odd += v;
                        m |= 1u << i;
                    }
                }
                if(m != 0u && (win == ~0u || hum > win_hum)) { // (50 on a tie)
                    win = fi * NH;
                    win_mask = m;
                    win_f0 = f0;
                    win_hum = hum;
                    win_odd = odd;
                    win_even = even;
                }
            }
        }
        for(uint32_t i = 0; i < NH; ++i)
            kept_k[i] = (win_mask >> i & 1u) != 0u ? line_k[win + i] : ~0u;
    }
    __syncthreads();

    // noise: the element of rank n / 2 among the powers of [noise_lo, noise_hi] outside +-3 bins of the remaining lines
    {
        uint32_t kk[NH];
#pragma unroll
        for(uint32_t i = 0; i < NH; ++i)
            kk[i] = kept_k[i];
        uint32_t mine = 0u;
        for(uint32_t b = a.noise_lo + t; b <= a.noise_hi; b += T) {
            bool in = true;
#pragma unroll
            for(uint32_t i = 0; i < NH; ++i)
                in = in && !(kk[i] != ~0u && b + WF_HIP_HUM_FLOOR_GUARD >= kk[i] && b <= kk[i] + WF_HIP_HUM_FLOOR_GUARD);
            mag[b] = in ? pw[b] : -1.0;
            mine += in ? 1u : 0u;
        }
        mine = wave_sum(mine);
        if(lane == 0u)
            part_bits[wave] = mine; // (its readers of the total are behind three barriers)
        if(t == 0u)
            noise_v = 0.0;
        __syncthreads();
        uint32_t n = part_bits[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_HUM_WAVES; ++w)
            n += part_bits[w];
        for(uint32_t b = a.noise_lo + t; b <= a.noise_hi; b += T) {
            const double vi = mag[b];
            if(vi < 0.0)
                continue;
            uint32_t before = 0u;
            for(uint32_t j = a.noise_lo; j <= a.noise_hi; ++j) {
                const double vj = mag[j];
                before += (uint32_t)(vj >= 0.0 && (vj < vi || (vj == vi && j < b)));
            }
            if(before == n / 2u)
                noise_v = vi; // (one thread: the ranks are all different)
        }
        __syncthreads();
    }

    if(t == 0u) {
#pragma clang fp contract(off)
        wf_hip_hum_channel r{};
        r.valid = 1u;
        r.total_db = (float)hum_db(total / (double)N);
        r.noise_db = (float)hum_db(noise_v / M_LN2);
        if(win != ~0u) {
            const double hdb = hum_db(win_hum), tdb = hum_db(total / (double)N);
            r.family = win == 0u ? 50u : 60u;
            r.mask = win_mask;
            r.mains_hz = (float)win_f0;
            r.hum_db = (float)hdb;
            r.ratio_db = (float)(hdb - tdb);
            r.odd_db = win_odd > 0.0 ? (float)hum_db(win_odd) : 0.0f;
            r.even_db = win_even > 0.0 ? (float)hum_db(win_even) : 0.0f;
            uint32_t lines = 0u;
#pragma unroll
            for(uint32_t i = 0; i < NH; ++i)
                if((win_mask >> i & 1u) != 0u) {
                    const uint32_t row = win + i;
                    r.hz[i] = (float)line_f[row];
                    r.level_db[i] = (float)hum_db(line_amp[row] * line_amp[row]);
                    r.snr_db[i] = (float)line_snr[row];
                    ++lines;
                }
            r.lines = lines;
        }
        out->ch[c] = r;
        header();
    }
}

} // namespace wf
