// wf_bits.hpp -- gfx950 read kernel of WF_HIP_OUT_BITS (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the bit meter of a metering suite, per captured channel the sample-value histogram, the activity of each of
// the 32 bits of the sample on a two's-complement grid, the level histogram in bits, the word length, the over-range and
// below-the-grid counts and the longest run of identical samples of the newest P = min(fft_size, 8192) frames of the ring (the
// definition is in include/wf_hip.h, "bit statistics").  wf_hip_read launches it on the handle's stream, behind every push issued so
// far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_BITS_THREADS per stream; the ring is read once.
//   stage    wf_ring_stage.hpp's ring_stage_window<CH>: the at most two contiguous runs of the window into dynamic LDS; frame i of channel c at
//            x[c][o + i].  The BitsWork follows the windows; its image, the entry as it leaves, is zeroed meanwhile.
//   count    a wavefront per 64 consecutive frames, lane j the j-th of them.  The code v comes from the sample's sign, exponent and
//            mantissa by integer shifts (bits_code): no float operation sees the sample, so nothing depends on how the hardware
//            treats denormals.  ones[b] and mag[k] are 32 ballots and popcounts each; lane b keeps the sum of bit b (one VGPR for
//            the 32 counters, not 32 SGPRs) and adds it to the image once, behind the wave's last chunk.  over / fine / heads are
//            popcounts of ballots in wave-uniform registers; the ORs of v and of s(v) are reduced over the wave once at the end
//            (the largest m(v) is the top bit of the OR of the s(v)).  A frame is a run head if it is frame 0 or its pattern differs
//            from frame i - 1, which is in LDS whatever the chunk: there is no carry between chunks.  Every chunk's head mask goes
//            to LDS as one 64-bit word.
//   hist     integer LDS atomic adds into the image, two uint16 bins to the word (a count is at most P <= 8192 < 2^16: the halves
//            never carry into each other), with wf_gonio.hpp's hand-over: a lane whose bin equals its lower neighbour's hands its
//            count to the head of that stretch, so silence, DC and low-frequency audio cost one atomic per stretch and not 64
//            serialised ones on one word; noise costs what it would without.
//   runs     behind a barrier, a wavefront per chunk again: every head finds the next head with a count of trailing zeros in its
//            own word; the chunk's last head needs the following words, and the whole wavefront looks for them, 64 words at a
//            time with one ballot -- a run that spans the window costs two such steps, not a walk over 128 words.  Runs compete by
//            the key (length << 13 | 8191 - start): the longest wins, of equal ones the first.  A maximum per lane, one butterfly
//            per wave, the waves' partials through LDS.
//   leave    one thread per channel combines the waves' partials into the eight scalars, and the image leaves as 16-B words: no
//            memset per read, no global atomics.
// Measured on an MI355X (tools/bits_bench.py, profiles/bits_kernel_stats.json; 4096 stereo streams, the read's 5.57 MB copy into
// page-locked memory included): noise 527 us, a 100 Hz sine 523 us, silence 495 us at P = 4096; 1280, 1289 and 1167 us at P = 8192,
// against 2360 and 4709 us for copying the windows to the host.  The contention case (the sine) and the long-run case (silence) cost
// no more than noise.  The kernel's own time without the copy, and the kernel without the hand-over: unmeasured.
// No float operations at all, no static LDS, no scratch; every accumulation is an integer count, an OR or a maximum of distinct
// keys, so the same ring contents read bit-identically.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_ring_stage.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct BitsArgs {
    RingView rings;          // (ring_cap a multiple of 4)
    wf_hip_bits *out;        // [count] the entry of stream `first` (16-byte aligned: a hipMalloc'ed block of 1360-byte entries)
    uint32_t first;          // first stream read
    uint32_t P;              // window <= min(ring_cap, WF_HIP_BITS_MAX_WINDOW), >= 1
};

constexpr uint32_t WF_BITS_THREADS = 256;
constexpr uint32_t WF_BITS_WAVES = WF_BITS_THREADS / 64;
constexpr uint32_t WF_BITS_UNROLL = 4;                 // float4 loads per channel in flight per lane
constexpr int WF_BITS_OCC = 4;                         // waves per SIMD the registers allow; the LDS allows two workgroups per CU at the cap
constexpr uint32_t WF_BITS_MAX_CHUNKS = WF_HIP_BITS_MAX_WINDOW / 64;
constexpr uint32_t WF_BITS_CH_WORDS = sizeof(wf_hip_bits_channel) / 4; // words of a channel in the image
static_assert(WF_BITS_THREADS == 256 && sizeof(wf_hip_bits) % 16 == 0 && sizeof(wf_hip_bits) == 1360 && sizeof(wf_hip_bits_channel) == 672);
static_assert(offsetof(wf_hip_bits_channel, ones) == 512 && offsetof(wf_hip_bits_channel, mag) == 576);
static_assert(offsetof(wf_hip_bits_channel, word_length) == 640 && offsetof(wf_hip_bits_channel, max_run_value) == 668);
static_assert(offsetof(wf_hip_bits, window) == 2 * sizeof(wf_hip_bits_channel));
static_assert(WF_HIP_BITS_MAX_WINDOW <= 8192, "the run key holds 13 bits of start, and a uint16 count must not overflow");

// what follows the staged windows in dynamic LDS
struct BitsWork {
    uint32_t image[sizeof(wf_hip_bits) / 4];          // the entry as it leaves: two counts to the word, then the scalars
    unsigned long long heads[2][WF_BITS_MAX_CHUNKS];  // per channel and 64-frame chunk: the frames that start a run
    uint32_t or_v[2][WF_BITS_WAVES], or_s[2][WF_BITS_WAVES], over[2][WF_BITS_WAVES], fine[2][WF_BITS_WAVES];
    uint32_t n_heads[2][WF_BITS_WAVES], key[2][WF_BITS_WAVES];
};
static_assert(offsetof(BitsWork, heads) % 8 == 0);

__host__ __device__ constexpr size_t bits_lds_bytes(uint32_t channels, uint32_t P)
{
    return (size_t)channels * ring_stage_stride(P) * sizeof(float) + sizeof(BitsWork);
}
static_assert(2 * bits_lds_bytes(2, WF_HIP_BITS_MAX_WINDOW) <= WF_LDS_PER_CU, "two workgroups to a CU at the cap");

// The code of a float32 pattern u: v = clamp(floor(x 2^31)) on the int32 grid, whether x 2^31 lies outside the grid and whether
// it has bits below it.  |x| = M 2^(e - 150) with M the 24-bit significand (no hidden bit and e = 1 for a denormal), so
// |x| 2^31 = M 2^sh, sh = e - 119: an integer below 2^31 for 0 <= sh < 8, at least 2^31 from sh = 8 on (exactly 2^31 for 1.0),
// and for sh < 0 the integer part M >> -sh with the shifted-out bits as the fraction (all of M from -sh = 24 on).  floor of a
// negative value with a fraction is one below the negated integer part.  Infinities and NaNs are over by their sign.
__device__ __forceinline__ int32_t bits_code(uint32_t u, bool &over, bool &fine)
{
    const bool neg = (u >> 31) != 0u;
    const uint32_t e = (u >> 23) & 0xffu;
    const uint32_t M = e != 0u ? (u & 0x7fffffu) | 0x800000u : u & 0x7fffffu;
    const int sh = (int)(e != 0u ? e : 1u) - 119;
    over = false;
    fine = false;
    if(sh >= 8) {
        over = u != 0xbf800000u; // -1.0 alone fits
        return neg ? INT32_MIN : INT32_MAX;
    }
    if(sh >= 0) {
        const uint32_t I = M << sh; // < 2^31
        return neg ? -(int32_t)I : (int32_t)I;
    }
    const uint32_t r = (uint32_t)(-sh) < 24u ? (uint32_t)(-sh) : 24u;
    const uint32_t I = M >> r;                       // < 2^23
    const bool frac = (M & ((1u << r) - 1u)) != 0u;
    fine = frac;
    return neg ? -(int32_t)I - (frac ? 1 : 0) : (int32_t)I;
}

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: bits_lds_bytes(CH, P)
template<int CH>
__global__ __launch_bounds__(WF_BITS_THREADS, WF_BITS_OCC) void bits_read_kernel(const BitsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float bits_x[]; // [CH][S], then the BitsWork
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P;
    const uint32_t S = ring_stage_stride(P);
    BitsWork &w = *reinterpret_cast<BitsWork *>(bits_x + (size_t)CH * S);
    const uint32_t ring_cap = a.rings.ring_cap;
    const uint32_t s = window_start(a.rings, stream, P) & (ring_cap - 1u);
    const uint32_t o = s & 3u;
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = CH == 2 ? channel_ring(a.rings, stream, 1, CH) : r0;
    const uint32_t *x0 = reinterpret_cast<const uint32_t *>(bits_x) + o; // x_c[i] = x0[c S + i], as patterns
    const uint32_t chunks = (P + 63u) / 64u;

    ring_stage_window<CH, WF_BITS_THREADS, WF_BITS_UNROLL>(bits_x, S, r0, r1, s, P, ring_cap);
    for(uint32_t i = t; i < sizeof(wf_hip_bits) / 4u; i += WF_BITS_THREADS)
        w.image[i] = 0u;
    __syncthreads();

    // the count
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        const uint32_t *x = x0 + (size_t)c * S;
        uint32_t *img = w.image + c * WF_BITS_CH_WORDS;
        uint32_t ones = 0u, mag = 0u;                 // lane b < 32: frames with bit b set, frames with m(v) == b
        uint32_t or_v = 0u, or_s = 0u;                // per lane until the wave's last chunk
        uint32_t n_over = 0u, n_fine = 0u, n_heads = 0u; // wave-uniform
        for(uint32_t base = 64u * wave; base < P; base += WF_BITS_THREADS) {
            const uint32_t i = base + lane;
            const bool valid = i < P; // (the valid lanes are the lowest)
            uint32_t u = 0u, below_u = 0u;
            if(valid) {
                u = x[i];
                below_u = i != 0u ? x[i - 1u] : ~u;
            }
            const unsigned long long heads = __ballot(valid && u != below_u);
            bool over, fine;
            const int32_t v = bits_code(u, over, fine); // (an invalid lane: pattern 0, v = 0, neither over nor fine)
            const uint32_t sv = (uint32_t)(v < 0 ? ~v : v);
            const uint32_t m = valid ? (sv != 0u ? 32u - (uint32_t)__builtin_clz(sv) : 0u) : 0xffu;
            if(lane == 0u)
                w.heads[c][base / 64u] = heads;
            n_heads += (uint32_t)__popcll(heads);
            n_over += (uint32_t)__popcll(__ballot(over));
            n_fine += (uint32_t)__popcll(__ballot(fine));
            or_v |= (uint32_t)v;
            or_s |= sv;
            // (not unrolled further: 64 ballots in flight are 128 SGPRs, more than a wave has)
#pragma unroll 4
            for(uint32_t b = 0; b < 32u; ++b) {
                const uint32_t n1 = (uint32_t)__popcll(__ballot((((uint32_t)v >> b) & 1u) != 0u));
                const uint32_t nm = (uint32_t)__popcll(__ballot(m == b));
                ones += lane == b ? n1 : 0u;
                mag += lane == b ? nm : 0u;
            }
            // the histogram: a stretch of lanes of equal bin adds once
            const uint32_t bin = valid ? (uint32_t)((v >> 24) + 128) : 0xffffffffu;
            const uint32_t below = __shfl_up(bin, 1, 64);
            const bool first = valid && (lane == 0u || bin != below);
            const unsigned long long firsts = __ballot(first);
            const uint32_t n_valid = (uint32_t)__popcll(__ballot(valid));
            if(first) { // the stretch ends in front of the next first lane, or with the valid lanes
                const unsigned long long above = firsts & ~((2ull << lane) - 1ull);
                const uint32_t next = above != 0 ? (uint32_t)__builtin_ctzll(above) : n_valid;
                __hip_atomic_fetch_add(&img[bin >> 1], (next - lane) << (16u * (bin & 1u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        or_v = wave_or(or_v);
        or_s = wave_or(or_s);
        if(lane < 32u) { // (zeros from a wave that had no chunk)
            const uint32_t sh = 16u * (lane & 1u);
            __hip_atomic_fetch_add(&img[offsetof(wf_hip_bits_channel, ones) / 4u + lane / 2u], ones << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&img[offsetof(wf_hip_bits_channel, mag) / 4u + lane / 2u], mag << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if(lane == 0u) {
            w.or_v[c][wave] = or_v;
            w.or_s[c][wave] = or_s;
            w.over[c][wave] = n_over;
            w.fine[c][wave] = n_fine;
            w.n_heads[c][wave] = n_heads;
        }
    }
    __syncthreads();

    // the runs: every head's run ends in front of the next head, or with the window
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        uint32_t key = 0u; // (length << 13) | (8191 - start): every run's is different, and every window has a run
        for(uint32_t g = wave; g < chunks; g += WF_BITS_WAVES) {
            const unsigned long long H = wave_uniform(w.heads[c][g]);
            if(H == 0)
                continue;
            // where the run of the chunk's last head ends: the first head of the first later chunk that has one
            uint32_t far = P;
            for(uint32_t k0 = g + 1u; k0 < chunks; k0 += 64u) {
                const uint32_t k = k0 + lane;
                const unsigned long long Hk = k < chunks ? w.heads[c][k] : 0ull;
                const unsigned long long some = __ballot(Hk != 0);
                if(some != 0) {
                    const uint32_t kk = k0 + (uint32_t)__builtin_ctzll(some);
                    far = 64u * kk + (uint32_t)__builtin_ctzll(wave_uniform(w.heads[c][kk]));
                    break;
                }
            }
            if((H >> lane) & 1ull) {
                const uint32_t i = 64u * g + lane;
                const unsigned long long above = H & ~((2ull << lane) - 1ull);
                const uint32_t next = above != 0 ? 64u * g + (uint32_t)__builtin_ctzll(above) : far;
                const uint32_t k = ((next - i) << 13) | (WF_HIP_BITS_MAX_WINDOW - 1u - i);
                key = key > k ? key : k;
            }
        }
        key = wave_max(key);
        if(lane == 0u)
            w.key[c][wave] = key;
    }
    __syncthreads();

    if(t < (uint32_t)CH) { // thread c: channel c's scalars
        uint32_t or_v = 0u, or_s = 0u, over = 0u, fine = 0u, n_heads = 0u, key = 0u;
        for(uint32_t k = 0; k < WF_BITS_WAVES; ++k) {
            or_v |= w.or_v[t][k];
            or_s |= w.or_s[t][k];
            over += w.over[t][k];
            fine += w.fine[t][k];
            n_heads += w.n_heads[t][k];
            key = key > w.key[t][k] ? key : w.key[t][k];
        }
        const uint32_t start = WF_HIP_BITS_MAX_WINDOW - 1u - (key & (WF_HIP_BITS_MAX_WINDOW - 1u));
        uint32_t *sc = w.image + t * WF_BITS_CH_WORDS + offsetof(wf_hip_bits_channel, word_length) / 4u;
        sc[0] = or_v != 0u ? 32u - (uint32_t)__builtin_ctz(or_v) : 0u;
        sc[1] = or_s != 0u ? 32u - (uint32_t)__builtin_clz(or_s) : 0u;
        sc[2] = over;
        sc[3] = fine;
        sc[4] = P - n_heads;
        sc[5] = key >> 13;
        sc[6] = start;
        sc[7] = x0[(size_t)t * S + start];
    } else if(t == 2u)
        w.image[offsetof(wf_hip_bits, window) / 4u] = P;
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(w.image);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + blockIdx.x);
    for(uint32_t i = t; i < sizeof(wf_hip_bits) / 16u; i += WF_BITS_THREADS)
        dst[i] = src[i];
}

} // namespace wf
