// wf_bands.hpp -- gfx950 read kernel of WF_HIP_OUT_BANDS (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the 31 third-octave band levels (IEC 61260-1) and the Z / A / C weighted level (IEC 61672-1) of every
// m_decibels row, as float64 power sums of the row's bins (the definition is in include/wf_hip.h, "band levels").  wf_hip_read
// launches it on the handle's stream, behind every tick issued so far, and copies the result back; nothing runs while the
// output is not read.
//
// One wavefront per row.  The row streams through in chunks of 64 x float4 (256 bins), WF_BANDS_GROUP chunks loaded together
// and the next group in flight while the current one is reduced.  Every lane turns its four bins into powers (float64 exp10)
// and adds them, in the order of the chunks, into four accumulators of its own: the three totals and the band in progress.  The
// bands are contiguous bin ranges in ascending order, so the wavefront walks them with one wave-uniform cursor: a chunk adds
// to every band it overlaps (a bin an edge cuts with its two overlap lengths; a chunk that lies wholly inside a band with
// plain sums), and a band that ends inside the chunk is summed over the 64 lanes by a butterfly and handed to the lane of its
// number.  31 + 3 butterflies per row, none per chunk.  The order of every sum follows from M and the edges alone.  No
// scratch, no LDS, no atomics.
//
// The A and C weights of a bin come from a float64 table [M][2] the host builds at the first read (one 16-byte load per bin,
// resident in L2: 32 KB at FFT 4096).  Evaluating them in the kernel -- squared, both curves are rational in f^2: one float64
// division per bin -- was measured and lost by 22 % (EXPERIMENTS.md).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_wave_reduce.hpp"

namespace wf {

struct BandsArgs {
    const float *rows;     // the first row read: [n_rows][M]
    wf_hip_bands *out;     // [n_rows]
    const double *edges;   // [WF_HIP_NUM_BANDS + 1] band edges in bins, ascending
    const double *weights; // [M][2] the squared A and C weights of every bin, 1 at 1000 Hz
    uint32_t n_rows;
    uint32_t M;            // bins per row (fft_size / 2; a multiple of 8)
    uint32_t covered;      // wf_hip_bands::covered, the same for every row
    float db_min;          // wf_hip_db_min(): a bin at or below it has no power
    double enbw;           // the window's equivalent noise bandwidth in bins
};

constexpr int WF_BANDS_GROUP = 2;  // chunks loaded together (2 KiB per wavefront in flight)
constexpr int WF_BANDS_WAVES = 4;  // rows per workgroup
constexpr int WF_BANDS_OCC = 4;    // waves per SIMD asked of the compiler (it reaches 5: 92 VGPRs)

// x / 10 to the last bit or next to it, without the division: the product's residual is exact in an fma
__device__ __forceinline__ double bands_tenth(double x)
{
    const double q = x * 0.1;
    return fma(fma(-10.0, q, x), 0.1, q);
}

__global__ __launch_bounds__(64 * WF_BANDS_WAVES, WF_BANDS_OCC) void bands_read_kernel(const BandsArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * WF_BANDS_WAVES + (threadIdx.x >> 6);
    if(row >= a.n_rows)
        return; // (wave-uniform)
    const float4 *d4 = reinterpret_cast<const float4 *>(a.rows + (size_t)row * a.M);
    const uint32_t n4 = a.M / 4u;
    const uint32_t nch = (n4 + 63u) / 64u;

    double tot = 0.0, tot_a = 0.0, tot_c = 0.0;
    double acc = 0.0;  // this lane's share of band `band`
    double mine = 0.0; // lane b: the sum of band b once it has ended
    uint32_t band = 0; // the band in progress (wave-uniform); the bands below it have ended
    double lo = wave_uniform(a.edges[0]), hi = wave_uniform(a.edges[1]);

    float4 cur[WF_BANDS_GROUP], nxt[WF_BANDS_GROUP];
#pragma unroll
    for(int u = 0; u < WF_BANDS_GROUP; ++u) {
        const uint32_t i = (uint32_t)u * 64u + lane;
        cur[u] = i < n4 ? d4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for(uint32_t g = 0; g < nch; g += WF_BANDS_GROUP) {
#pragma unroll
        for(int u = 0; u < WF_BANDS_GROUP; ++u) {
            const uint32_t i = (g + WF_BANDS_GROUP + (uint32_t)u) * 64u + lane;
            nxt[u] = i < n4 ? d4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for(int u = 0; u < WF_BANDS_GROUP; ++u) {
            const uint32_t c = g + (uint32_t)u;
            if(c >= nch)
                break; // (wave-uniform)
            const uint32_t k0 = c * 256u + lane * 4u;
            const float d[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
            double p[4];
#pragma unroll
            for(int j = 0; j < 4; ++j) {
                const uint32_t k = k0 + (uint32_t)j;
                const double e = exp10(bands_tenth((double)d[j]));
                // bin 0, the bins past the row's end (loaded as zeros) and the bins at or below DB_MIN have no power
                p[j] = ((k - 1u) < (a.M - 1u) && !(d[j] <= a.db_min)) ? e : 0.0;
                const double2 w = reinterpret_cast<const double2 *>(a.weights)[k < a.M ? k : 0u]; // (A, C)
                tot += p[j];
                tot_a = fma(p[j], w.x, tot_a);
                tot_c = fma(p[j], w.y, tot_c);
            }
            // the chunk's bins cover [c_lo, c_hi] on the bin axis
            const double c_lo = (double)(c * 256u) - 0.5, c_hi = (double)(c * 256u + 256u) - 0.5;
            while(band < WF_HIP_NUM_BANDS && lo < c_hi) { // (wave-uniform) the bands that overlap the chunk, in order
                if(lo <= c_lo && hi >= c_hi) {            // the chunk lies wholly inside the band: every weight is 1
#pragma unroll
                    for(int j = 0; j < 4; ++j)
                        acc += p[j];
                } else {
#pragma unroll
                    for(int j = 0; j < 4; ++j) {
                        const double kk = (double)(k0 + (uint32_t)j);
                        const double w = fmax(fmin(kk + 0.5, hi) - fmax(kk - 0.5, lo), 0.0);
                        acc = fma(w, p[j], acc); // (w == 1: acc + p[j] exactly, as above)
                    }
                }
                if(hi > c_hi)
                    break; // the band goes on in the next chunk
                const double s = wave_sum(acc);
                if(lane == band)
                    mine = s;
                acc = 0.0;
                ++band;
                lo = hi;
                if(band < WF_HIP_NUM_BANDS)
                    hi = wave_uniform(a.edges[band + 1u]);
            }
        }
#pragma unroll
        for(int u = 0; u < WF_BANDS_GROUP; ++u)
            cur[u] = nxt[u];
    }
    if(band < WF_HIP_NUM_BANDS) { // the band the row ends in; the bands above it keep 0
        const double s = wave_sum(acc);
        if(lane == band)
            mine = s;
    }
    tot = wave_sum(tot);
    tot_a = wave_sum(tot_a);
    tot_c = wave_sum(tot_c);

    // the struct as 36 words: band_db[31], covered, total_db, a_db, c_db, reserved -- one store per lane
    const double s = lane < WF_HIP_NUM_BANDS ? mine : lane == 32u ? tot : lane == 33u ? tot_a : tot_c;
    const float db = s == 0.0 ? -INFINITY : (float)(10.0 * log10(s / a.enbw));
    const uint32_t word = lane == 31u ? a.covered : lane == 35u ? 0u : __float_as_uint(db);
    static_assert(sizeof(wf_hip_bands) == 36 * sizeof(uint32_t) && WF_HIP_NUM_BANDS == 31, "the word layout above");
    if(lane < 36u)
        reinterpret_cast<uint32_t *>(a.out + row)[lane] = word;
}

} // namespace wf
