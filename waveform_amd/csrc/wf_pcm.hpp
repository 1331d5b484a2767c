// wf_pcm.hpp -- gfx950 ring append for integer and interleaved PCM (wf_hip_push_pcm; device code only; hipcc; included by
// wf_hip.hip alone).
//
// What it restates (reference): WAVSource::capture_audio (src/source.cpp:1827-1828, :1842-1886) takes channels
// m_channel_base .. m_channel_base + m_capture_channels of an OBS audio packet and pushes them into its circular buffers, and
// the per-frame squared peak of those channels into m_rms_sync_buf.  The packet comes here in any libobs sample format
// (enum audio_format: u8 / s16 / s32 / float, interleaved or planar) and is widened on the device: the bus carries the
// packet's own bytes, not float32.
//
// One pass per (stream, tile of frames):
//   1. stage the tile's bytes in LDS -- 16-B loads over the 16-B aligned body of every run of bytes, one element load per
//      lane for the misaligned head and tail (a u8 or s16 block of an odd frame count starts at any byte or half-word);
//   2. one frame per lane: pick the captured channels out of LDS, convert them exactly (the full-scale mapping of
//      include/wf_hip.h), store them into the stream's cap_ch rings at its write position and, where the RMS producer
//      follows the audio, the squared peak into the RMS ring (rms_push_kernel's arithmetic on the converted floats).
// The ring stays float32; everything downstream (rms_block_kernel, wpos_advance_kernel, the tick) is unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include "wf_tick_args.hpp" // WF_STREAM_*
#include "wf_hip.h"

namespace wf {

// the sample types, by libobs' interleaved format value (the planar one is that + 4)
template<uint32_t Fmt> struct Pcm;
template<> struct Pcm<WF_HIP_PCM_U8> {
    using T = uint8_t;
    static WF_DEV float conv(T x) { return (float)((int)x - 128) * 0x1p-7f; }
};
template<> struct Pcm<WF_HIP_PCM_S16> {
    using T = int16_t;
    static WF_DEV float conv(T x) { return (float)x * 0x1p-15f; }
};
template<> struct Pcm<WF_HIP_PCM_S32> {
    using T = int32_t;
    static WF_DEV float conv(T x) { return (float)x * 0x1p-31f; } // (float)x rounds to nearest even; the scaling is exact
};
template<> struct Pcm<WF_HIP_PCM_F32> {
    using T = uint32_t; // the bits pass through untouched (no arithmetic on them: a NaN keeps its payload)
    static WF_DEV float conv(T x) { return __uint_as_float(x); }
};

constexpr uint32_t PCM_TILE = 8192;   // bytes of one run (interleaved: the tile; planar: one captured plane of it)
constexpr uint32_t PCM_THREADS = 256;

struct PcmPushArgs {
    float *ring;
    uint32_t *wpos;
    uint32_t *flags;                 // ragged: WF_STREAM_WRAPPED
    uint32_t ring_cap, ring_stride, cap_ch, first;
    const unsigned char *src;        // the (staged) packet of streams first.., one block of block_bytes per stream
    size_t block_bytes;
    uint32_t channels;               // channels of the block's layout (interleaved: per frame; planar: planes)
    uint32_t base;                   // first captured channel within the block
    uint32_t frames;                 // frames per block (ragged: max_frames)
    const uint32_t *frames_per_stream; // ragged: [count]
    float *rms_ring;                 // nullptr unless the RMS producer follows the audio
    uint32_t rms_cap;
};

// bytes [src, src + n) -> lds + (src & 15): the body in 16-B loads and stores (both sides 16-B aligned), the head before the
// first 16-B boundary and the tail after the last one element by element.  src is aligned to sizeof(U), n a multiple of it.
template<class U>
WF_DEV void pcm_stage(unsigned char *lds, const unsigned char *src, uint32_t n)
{
    const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);
    const uint32_t head = ((16u - mis) & 15u) < n ? ((16u - mis) & 15u) : n;
    const uint32_t body = (n - head) & ~15u;
    const uint32_t tail = n - head - body;
    unsigned char *dst = lds + mis;
    for(uint32_t i = threadIdx.x; i < body / 16u; i += blockDim.x)
        *reinterpret_cast<uint4 *>(dst + head + 16u * i) = *reinterpret_cast<const uint4 *>(src + head + 16u * i);
    const uint32_t nh = head / sizeof(U), nt = tail / sizeof(U); // at most 15 each
    const uint32_t t = threadIdx.x;
    if(t < nh)
        *reinterpret_cast<U *>(dst + t * sizeof(U)) = *reinterpret_cast<const U *>(src + t * sizeof(U));
    else if(t - nh < nt) {
        const uint32_t o = head + body + (t - nh) * sizeof(U);
        *reinterpret_cast<U *>(dst + o) = *reinterpret_cast<const U *>(src + o);
    }
}

// grid (tiles, streams); Ragged: grid (1, streams), every stream appends its own frame count and advances its write position
// itself (ring_push_ragged_kernel's rule); otherwise wpos_advance_kernel follows.  Tiles of one stream stride by gridDim.x.
template<uint32_t Fmt, bool Interleaved, bool Ragged>
__global__ __launch_bounds__(PCM_THREADS) void ring_push_pcm_kernel(const PcmPushArgs a)
{
    using T = typename Pcm<Fmt>::T;
    constexpr uint32_t B = sizeof(T);
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][PCM_TILE + 16];
    const uint32_t s = blockIdx.y, stream = a.first + s;
    const uint32_t n = Ragged ? (a.frames_per_stream[s] < a.frames ? a.frames_per_stream[s] : a.frames) : a.frames;
    const uint32_t w = a.wpos[stream];
    const uint32_t skip = n > a.ring_cap ? n - a.ring_cap : 0u; // a packet longer than the ring: only its tail survives
    const uint32_t mask = a.ring_cap - 1u;
    const unsigned char *blk = a.src + (size_t)s * a.block_bytes;
    float *dst = a.ring + (size_t)stream * a.cap_ch * a.ring_stride;
    float *rms = a.rms_ring ? a.rms_ring + (size_t)stream * a.rms_cap : nullptr;
    const uint32_t tile = Interleaved ? PCM_TILE / (a.channels * B) : PCM_TILE / B;
    for(uint32_t f0 = blockIdx.x * tile; f0 < n; f0 += gridDim.x * tile) {
        const uint32_t nf = n - f0 < tile ? n - f0 : tile;
        const unsigned char *run0 = Interleaved ? blk + (size_t)f0 * a.channels * B : blk + ((size_t)a.base * a.frames + f0) * B;
        const unsigned char *run1 = Interleaved ? run0 : run0 + (size_t)a.frames * B; // planar: the second captured plane
        if(Interleaved)
            pcm_stage<T>(lds[0], run0, nf * a.channels * B);
        else {
            pcm_stage<T>(lds[0], run0, nf * B);
            if(a.cap_ch > 1)
                pcm_stage<T>(lds[1], run1, nf * B);
        }
        __syncthreads();
        const unsigned char *l0 = lds[0] + ((uintptr_t)run0 & 15u), *l1 = Interleaved ? l0 : lds[1] + ((uintptr_t)run1 & 15u);
        for(uint32_t i = threadIdx.x; i < nf; i += blockDim.x) {
            const uint32_t f = f0 + i, pos = w + f;
            const float x0 = Pcm<Fmt>::conv(*reinterpret_cast<const T *>(Interleaved ? l0 + (i * a.channels + a.base) * B : l0 + i * B));
            float peak = __builtin_fabsf(x0);
            if(f >= skip)
                dst[pos & mask] = x0;
            if(a.cap_ch > 1) {
                const float x1 = Pcm<Fmt>::conv(*reinterpret_cast<const T *>(Interleaved ? l0 + (i * a.channels + a.base + 1u) * B : l1 + i * B));
                peak = __builtin_fmaxf(__builtin_fabsf(x1), peak);
                if(f >= skip)
                    dst[a.ring_stride + (pos & mask)] = x1;
            }
            if(rms)
                rms[pos & (a.rms_cap - 1u)] = peak * peak;
        }
        __syncthreads(); // the tile's LDS is free again
    }
    if(Ragged && threadIdx.x == 0 && n > 0) { // (every thread read w before the loop's barrier)
        a.wpos[stream] = w + n;
        if(w + n < w)
            a.flags[stream] |= WF_STREAM_WRAPPED;
    }
}

} // namespace wf
