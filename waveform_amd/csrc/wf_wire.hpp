// wf_wire.hpp -- gfx950 ring append for the sample formats libobs has no name for (wf_hip_wire_format: packed 24-bit in either
// byte order, big-endian int16, G.711 mu-law and A-law; device code only; hipcc; included by wf_hip.hip alone).
//
// ring_push_pcm_kernel (wf_pcm.hpp) rests on a sample of 1, 2 or 4 bytes that is naturally aligned: it stages by elements and
// reads LDS through a pointer to the sample's type.  A packed 24-bit sample is neither, so this kernel works in bytes:
//   1. stage the tile's bytes in LDS at lds + (src & 15) -- pcm_stage<uint8_t>: 16-B loads over the 16-B aligned body of the run,
//      byte loads for the up to 15 bytes before and after it (a run of 3-byte samples starts at any address and has any length);
//   2. one frame per lane: read the captured channels' bytes out of LDS (wire_u24 below), put them in order, sign-extend or
//      decode (integer VALU, no table), scale by a power of two (exact, include/wf_hip.h) and do with the floats what
//      ring_push_pcm_kernel does: the rings at the stream's write position, the squared peak into the RMS ring.
// A tile is a whole number of frames (PCM_TILE is no multiple of 3): wire_tile_frames, which the host uses too.
//
// LDS banks (a bank is a dword, 32 of them for ds_read_b32 / ds_read2_b32 / ds_read_u8 / _u16, conflicts within a half wave):
// lane i reads at byte i * stride + const, stride = sample bytes x (interleaved: channels; planar: 1).  A 3-byte sample takes the
// dwords floor(byte / 4) and the next one.  Stride 3 (s24 mono or planar): a half wave covers 96 B = 24 dwords, lanes that share
// a dword are served together -- conflict-free, as every stride up to 4.  Stride 6 (s24 stereo, 5.1 mu-law): 48 dwords on 32
// banks, 2-way on the banks the last third of the lanes shares with the first.  Stride 18 and 24 (s24 5.1 and 8 channels): 2-way
// (4.5 dwords per lane wraps onto occupied banks once; 6 dwords per lane uses every other bank).  Nothing in the wire formats is
// worse than 2-way, which is what ring_push_pcm_kernel pays for s32 stereo (stride 8); its worst case is 8-channel s16 and s32
// (stride 16 / 32: 4- / 8-way).  The reads are one or two per frame against the tile's global loads and ring stores, and the
// append is bound by those: DESIGN.md 4.4, "Wire formats".
#pragma once
#include <hip/hip_runtime.h>
#include "wf_pcm.hpp"
#include "wf_pcm_formats.hpp"

namespace wf {

// frames of one tile: interleaved, the frames whose bytes fit PCM_TILE; planar, the samples of one plane that do
__host__ __device__ constexpr uint32_t wire_tile_frames(bool interleaved, uint32_t channels, uint32_t sample_bytes)
{
    return interleaved ? PCM_TILE / (channels * sample_bytes) : PCM_TILE / sample_bytes;
}

// the three bytes at byte offset o of lds (16-B aligned; any o) in bits 0..23, the byte at the lowest address lowest; bits
// 24..31 are whatever follows.  The two aligned dwords around the sample (one ds_read2_b32) and one v_alignbyte_b32: no access
// is misaligned, and the second dword may lie up to 7 bytes past the sample (the LDS arrays are that much longer).  Three
// ds_read_u8 and two v_lshl_or_b32 give the same append time; this is one LDS instruction instead of three.
WF_DEV uint32_t wire_u24(const unsigned char *lds, uint32_t o)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(lds + (o & ~3u));
    return __builtin_amdgcn_alignbyte(w[1], w[0], o & 3u);
}

// the sample types, by the interleaved format value (the planar one is that + 8): B bytes per sample, at(lds, o) the float of
// the sample at byte offset o of the 16-B aligned lds (o a multiple of the sample's alignment)
template<uint32_t Fmt> struct Wire;
template<> struct Wire<WF_HIP_WIRE_S24> {
    static constexpr uint32_t B = 3;
    static WF_DEV float at(const unsigned char *lds, uint32_t o) { return (float)((int32_t)(wire_u24(lds, o) << 8) >> 8) * 0x1p-23f; }
};
template<> struct Wire<WF_HIP_WIRE_S24_BE> {
    static constexpr uint32_t B = 3;
    // b0 b1 b2 ?? -> ?? b2 b1 b0 (one v_perm_b32): the sample in bits 8..31, most significant byte on top
    static WF_DEV float at(const unsigned char *lds, uint32_t o) { return (float)((int32_t)__builtin_bswap32(wire_u24(lds, o)) >> 8) * 0x1p-23f; }
};
template<> struct Wire<WF_HIP_WIRE_S16_BE> {
    static constexpr uint32_t B = 2;
    static WF_DEV float at(const unsigned char *lds, uint32_t o)
    {
        const uint32_t u = *reinterpret_cast<const uint16_t *>(lds + o); // (o is even: device data is 2-B aligned, blocks are whole samples)
        return (float)(int16_t)(u << 8 | u >> 8) * 0x1p-15f;
    }
};
template<> struct Wire<WF_HIP_WIRE_ULAW> {
    static constexpr uint32_t B = 1;
    static WF_DEV float at(const unsigned char *lds, uint32_t o)
    {
        const uint32_t u = ~(uint32_t)lds[o] & 0xFFu, e = (u >> 4) & 7u, m = u & 15u;
        const int32_t mag = (int32_t)((((m << 3) + 0x84u) << e) - 0x84u);
        return (float)(u & 0x80u ? -mag : mag) * 0x1p-15f; // (both zero codes: the integer 0, +0.0f)
    }
};
template<> struct Wire<WF_HIP_WIRE_ALAW> {
    static constexpr uint32_t B = 1;
    static WF_DEV float at(const unsigned char *lds, uint32_t o)
    {
        const uint32_t a = (uint32_t)lds[o] ^ 0x55u, e = (a >> 4) & 7u, m = a & 15u;
        const int32_t mag = (int32_t)(e ? ((m << 4) + 0x108u) << (e - 1u) : (m << 4) + 8u);
        return (float)(a & 0x80u ? mag : -mag) * 0x1p-15f;
    }
};

// ring_push_pcm_kernel's grid and arguments: (tiles, streams); Ragged: (1, streams), every stream appends its own frame count
// and advances its write position itself.  Tiles of one stream stride by gridDim.x.
template<uint32_t Fmt, bool Interleaved, bool Ragged>
__global__ __launch_bounds__(PCM_THREADS) void ring_push_wire_kernel(const PcmPushArgs a)
{
    using W = Wire<Fmt>;
    constexpr uint32_t B = W::B;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][PCM_TILE + 32]; // 15 B of misalignment in front, wire_u24's dword behind
    const uint32_t s = blockIdx.y, stream = a.first + s;
    const uint32_t n = Ragged ? (a.frames_per_stream[s] < a.frames ? a.frames_per_stream[s] : a.frames) : a.frames;
    const uint32_t w = a.wpos[stream];
    const uint32_t skip = n > a.ring_cap ? n - a.ring_cap : 0u; // a packet longer than the ring: only its tail survives
    const uint32_t mask = a.ring_cap - 1u;
    const unsigned char *blk = a.src + (size_t)s * a.block_bytes;
    float *dst = a.ring + (size_t)stream * a.cap_ch * a.ring_stride;
    float *rms = a.rms_ring ? a.rms_ring + (size_t)stream * a.rms_cap : nullptr;
    const uint32_t tile = wire_tile_frames(Interleaved, a.channels, B);
    for(uint32_t f0 = blockIdx.x * tile; f0 < n; f0 += gridDim.x * tile) {
        const uint32_t nf = n - f0 < tile ? n - f0 : tile;
        const unsigned char *run0 = Interleaved ? blk + (size_t)f0 * a.channels * B : blk + ((size_t)a.base * a.frames + f0) * B;
        const unsigned char *run1 = Interleaved ? run0 : run0 + (size_t)a.frames * B; // planar: the second captured plane
        if(Interleaved)
            pcm_stage<uint8_t>(lds[0], run0, nf * a.channels * B);
        else {
            pcm_stage<uint8_t>(lds[0], run0, nf * B);
            if(a.cap_ch > 1)
                pcm_stage<uint8_t>(lds[1], run1, nf * B);
        }
        __syncthreads();
        // byte offsets of frame 0's captured samples within lds[0] / lds[1], and from one frame to the next
        const uint32_t o0 = (uint32_t)((uintptr_t)run0 & 15u) + (Interleaved ? a.base * B : 0u);
        const uint32_t o1 = Interleaved ? o0 + B : (uint32_t)((uintptr_t)run1 & 15u);
        const uint32_t step = Interleaved ? a.channels * B : B;
        const unsigned char *l1 = Interleaved ? lds[0] : lds[1];
        for(uint32_t i = threadIdx.x; i < nf; i += blockDim.x) {
            const uint32_t f = f0 + i, pos = w + f;
            const float x0 = W::at(lds[0], o0 + i * step);
            float peak = __builtin_fabsf(x0);
            if(f >= skip)
                dst[pos & mask] = x0;
            if(a.cap_ch > 1) {
                const float x1 = W::at(l1, o1 + i * step);
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
