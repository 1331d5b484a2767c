"""Host-fed headline per sample format (wf_hip_push_pcm): 4096 stereo streams, FFT 4096, bars, one 800-frame hop per stream and
step through two page-locked slots (the copy of step i+1 under the tick of step i), one tick per step.  In one process, in
turn and for several rounds: float32 planar through wf_hip_push_audio_async, then s16 / u8 / s32 interleaved stereo through
wf_hip_push_pcm.  Prints one JSON line per (round, format) and a summary line with each format's median.
--wire adds the wire formats (wf_hip_wire_format) to the same rounds: s24, s24_be, s16_be and mu-law, interleaved stereo -- to be
read against s32 / f32, s16 and u8 of the same process --, and then times the append alone: the same packets pushed from device
memory (WF_HIP_PCM_DEVICE, no copy, no tick) between wf_hip_time_begin and wf_hip_time_end, every wire format beside s16 and s32.
usage: python tools/pcm_ingest_bench.py [--wire] [--rounds 3] [--warmup 400] [--steps 200] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf
from tools import synth
from tools.bench_common import device_block

FORMATS = [("f32_planar", np.float32, False), ("s16_interleaved", np.int16, True), ("u8_interleaved", np.uint8, True),
           ("s32_interleaved", np.int32, True)]
WIRE_FORMATS = [("s24_interleaved", "s24", True), ("s24_be_interleaved", "s24_be", True), ("s16_be_interleaved", "s16_be", True),
                ("ulaw_interleaved", "ulaw", True)]
# what a wire format's rate is read against (same width or wider)
NEIGHBOURS = {"s24_interleaved": ["s32_interleaved", "f32_planar"], "s24_be_interleaved": ["s32_interleaved", "f32_planar"],
              "s16_be_interleaved": ["s16_interleaved"], "ulaw_interleaved": ["u8_interleaved"]}


def packet(dtype, interleaved, streams, hop):
    """one synth hop per stream in the format's own samples (full scale)"""
    audio = synth.block(synth.DEFAULT_SEED, 0, 1, 2, 0, hop)[0]  # [2][hop] float in [-1, 1)
    x = np.clip(audio, -1.0, 1.0 - 2.0 ** -7)
    if dtype == np.float32:
        one = audio.astype(np.float32)
    elif dtype == np.int16:
        one = np.round(x * 32768.0).astype(np.int16)
    elif dtype == np.uint8:
        one = (np.round(x * 128.0) + 128).astype(np.uint8)
    else:
        one = np.round(x.astype(np.float64) * 2.0 ** 31).astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)
    one = one.T if interleaved else one  # [hop][2] or [2][hop]
    return np.broadcast_to(one[None], (streams,) + one.shape)


def g711_table(wire):
    """the 256 linear values of mu-law / A-law (include/wf_hip.h)"""
    b = np.arange(256)
    if wire == "ulaw":
        u = ~b & 0xFF
        mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
        return np.where(u & 0x80, -mag, mag)
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, mag, -mag)


def wire_packet(wire, interleaved, streams, hop):
    """the same hop in a wire format: uint8 [streams][hop][2][B] or [streams][2][hop][B]"""
    audio = synth.block(synth.DEFAULT_SEED, 0, 1, 2, 0, hop)[0].astype(np.float64)  # [2][hop]
    if wire in ("s24", "s24_be"):
        v = np.round(audio * 2.0 ** 23).astype(np.int64).clip(-2 ** 23, 2 ** 23 - 1)
        one = np.stack([(v >> sh) & 0xFF for sh in ((0, 8, 16) if wire == "s24" else (16, 8, 0))], axis=-1).astype(np.uint8)
    elif wire == "s16_be":
        v = np.round(audio * 32768.0).astype(np.int64).clip(-32768, 32767)
        one = np.stack([(v >> 8) & 0xFF, v & 0xFF], axis=-1).astype(np.uint8)
    else:  # G.711: the nearest code
        table = g711_table(wire)
        one = np.abs(audio[..., None] * 32768.0 - table).argmin(axis=-1).astype(np.uint8)[..., None]
    one = one.transpose(1, 0, 2) if interleaved else one
    return np.broadcast_to(one[None], (streams,) + one.shape)


def append_alone(b, a, packets):
    """device microseconds of one push from device memory (the append kernel, the write-position update and whatever follows a
    push; no copy, no tick), per format: the median over a.rounds brackets of a.append_pushes pushes each"""
    L = wf.lib()
    out = {}
    for name, (fmt, p) in packets.items():
        host = np.ascontiguousarray(p)
        with device_block(host.nbytes) as (d, memcpy):
            assert memcpy(d, C.c_void_p(host.ctypes.data), host.nbytes, 1) == 0
            pcm = wf.binding.Pcm(data=d.value, format=fmt, channels=2, channel_base=0, frames=a.hop, memory=wf.binding.PCM_DEVICE, slot=0)
            us = []
            for r in range(a.rounds + 1):  # (the first bracket warms up)
                b.time_begin()
                for _ in range(a.append_pushes):
                    assert L.wf_hip_push_pcm(b.h, 0, a.streams, C.byref(pcm)) == 0
                us.append(b.time_end() * 1e3 / a.append_pushes)
            out[name] = dict(us_per_push=round(float(np.median(us[1:])), 2), rounds_us=[round(u, 2) for u in us[1:]], bytes=host.nbytes,
                             read_GBps=round(host.nbytes / (float(np.median(us[1:])) * 1e-6) / 1e9, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wire", action="store_true", help="add the wire formats' rows and the append-alone times")
    ap.add_argument("--append-pushes", type=int, default=50)
    a = ap.parse_args()
    formats = [(name, dtype, inter, None) for name, dtype, inter in FORMATS]
    if a.wire:
        formats += [(name, np.uint8, inter, wire) for name, wire, inter in WIRE_FORMATS]
    cfg = wf.Config.defaults(fft_size=a.fft, stereo=1, slope=1.0, bars=1, interp_mode=1)
    rows = []
    with wf.SpectrumBatch(cfg, a.streams) as b:
        pins = {}
        for name, dtype, inter, wire in formats:
            p = wire_packet(wire, inter, a.streams, a.hop) if wire else packet(dtype, inter, a.streams, a.hop)
            pins[name] = [wf.PinnedBuffer(p.shape, dtype), wf.PinnedBuffer(p.shape, dtype)]
            for q in pins[name]:
                q.array[...] = p
        for r in range(a.rounds):
            for name, dtype, inter, wire in formats:
                pin = pins[name]
                nbytes = pin[0].array.nbytes
                for i in range(a.warmup + a.steps):
                    if i == a.warmup:
                        b.sync()
                        t0 = time.perf_counter()
                    slot = i & 1
                    b.ingest_done(slot)  # the buffer is free again (a real host would refill it here)
                    if name == "f32_planar":
                        b.push_audio_async(pin[slot], a.streams, a.hop, slot)
                    else:
                        b.push_pcm(pin[slot], interleaved=inter, slot=slot, wire=wire)
                    b.tick()
                b.sync()
                dt = (time.perf_counter() - t0) / a.steps
                row = dict(round=r, format=name, entry="wf_hip_push_audio_async" if name == "f32_planar" else "wf_hip_push_pcm",
                           streams=a.streams, fft=a.fft, hop=a.hop, ms_per_step=round(dt * 1e3, 4),
                           Mspectra_s=round(2 * a.streams / dt / 1e6, 2), host_GBps=round(nbytes / dt / 1e9, 2), bytes_per_step=nbytes)
                rows.append(row)
                print(json.dumps(row), flush=True)
        append = None
        if a.wire:
            b.sync()
            packets = {name: (wf.binding.PCM_FORMAT[np.dtype(dtype)], pins[name][0].array) for name, dtype, inter, wire in formats
                       if name in ("s16_interleaved", "s32_interleaved")}
            packets.update({name: (wf.binding.WIRE_FORMAT[wire], pins[name][0].array) for name, dtype, inter, wire in formats if wire})
            append = append_alone(b, a, packets)
            print(json.dumps(dict(append_alone=append)), flush=True)
        for ps in pins.values():
            for q in ps:
                q.close()
    per = {name: [x["Mspectra_s"] for x in rows if x["format"] == name] for name, _, _, _ in formats}
    med = {name: float(np.median(v)) for name, v in per.items()}
    summary = dict(median_Mspectra_s=med, ratio_to_f32={k: round(v / med["f32_planar"], 3) for k, v in med.items()},
                   warmup=a.warmup, steps=a.steps, rounds=a.rounds)
    if a.wire:
        summary["spread_over_rounds"] = {k: round((max(v) - min(v)) / med[k], 4) for k, v in per.items()}
        summary["wire_over_neighbour"] = {k: {n: round(med[k] / med[n], 3) for n in ns} for k, ns in NEIGHBOURS.items()}
    print(json.dumps(summary), flush=True)
    if a.out:
        doc = dict(rows=rows, summary=summary)
        if append is not None:
            doc["append_alone"] = dict(streams=a.streams, frames=a.hop, channels=2, pushes_per_bracket=a.append_pushes, formats=append)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
