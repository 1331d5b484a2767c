"""Host-fed headline per sample format (wf_hip_push_pcm): 4096 stereo streams, FFT 4096, bars, one 800-frame hop per stream and
step through two page-locked slots (the copy of step i+1 under the tick of step i), one tick per step.  In one process, in
turn and for several rounds: float32 planar through wf_hip_push_audio_async, then s16 / u8 / s32 interleaved stereo through
wf_hip_push_pcm.  Prints one JSON line per (round, format) and a summary line with each format's median.
usage: python tools/pcm_ingest_bench.py [--rounds 3] [--warmup 400] [--steps 200] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf
from tools import synth

FORMATS = [("f32_planar", np.float32, False), ("s16_interleaved", np.int16, True), ("u8_interleaved", np.uint8, True),
           ("s32_interleaved", np.int32, True)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = wf.Config.defaults(fft_size=a.fft, stereo=1, slope=1.0, bars=1, interp_mode=1)
    rows = []
    with wf.SpectrumBatch(cfg, a.streams) as b:
        pins = {}
        for name, dtype, inter in FORMATS:
            p = packet(dtype, inter, a.streams, a.hop)
            pins[name] = [wf.PinnedBuffer(p.shape, dtype), wf.PinnedBuffer(p.shape, dtype)]
            for q in pins[name]:
                q.array[...] = p
        for r in range(a.rounds):
            for name, dtype, inter in FORMATS:
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
                        b.push_pcm(pin[slot], interleaved=inter, slot=slot)
                    b.tick()
                b.sync()
                dt = (time.perf_counter() - t0) / a.steps
                row = dict(round=r, format=name, entry="wf_hip_push_audio_async" if name == "f32_planar" else "wf_hip_push_pcm",
                           streams=a.streams, fft=a.fft, hop=a.hop, ms_per_step=round(dt * 1e3, 4),
                           Mspectra_s=round(2 * a.streams / dt / 1e6, 2), host_GBps=round(nbytes / dt / 1e9, 2), bytes_per_step=nbytes)
                rows.append(row)
                print(json.dumps(row), flush=True)
        for ps in pins.values():
            for q in ps:
                q.close()
    med = {name: float(np.median([x["Mspectra_s"] for x in rows if x["format"] == name])) for name, _, _ in FORMATS}
    summary = dict(median_Mspectra_s=med, ratio_to_f32={k: round(v / med["f32_planar"], 3) for k, v in med.items()},
                   warmup=a.warmup, steps=a.steps, rounds=a.rounds)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(rows=rows, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
