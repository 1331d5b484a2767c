"""Cost of the loudness producer on the host-fed headline: 4096 stereo streams, 48 kHz, FFT 4096, bars, one 800-frame hop per
stream and step through two page-locked slots (wf_hip_push_audio_async), one tick per step.  Two handles in one process, one
with the producer off and one with it on (wf_hip_enable_loudness), run in turn for several rounds; one JSON line per (round,
producer) and a summary line with the medians and the difference per hop.  The producer's own kernel time comes from a
rocprofv3 --kernel-trace run of this tool (the wall clock of this host-fed shape is set by the H2D copies).
usage: python tools/loudness_bench.py [--rounds 3] [--warmup 400] [--steps 200] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf
from tools import synth


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
    cfg = wf.Config.defaults(fft_size=a.fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, interp_mode=1)
    audio = synth.block(synth.DEFAULT_SEED, 0, 1, 2, 0, a.hop)[0]  # [2][hop]
    rows = []
    with wf.SpectrumBatch(cfg, a.streams) as off, wf.SpectrumBatch(cfg, a.streams) as on:
        on.enable_loudness()
        pin = [wf.PinnedBuffer((a.streams, 2, a.hop)), wf.PinnedBuffer((a.streams, 2, a.hop))]
        for q in pin:
            q.array[...] = audio[None]
        for r in range(a.rounds):
            order = (("off", off), ("on", on)) if r % 2 == 0 else (("on", on), ("off", off))  # (alternating: no order effect)
            for name, b in order:
                for i in range(a.warmup + a.steps):
                    if i == a.warmup:
                        b.sync()
                        t0 = time.perf_counter()
                    slot = i & 1
                    b.ingest_done(slot)
                    b.push_audio_async(pin[slot], a.streams, a.hop, slot)
                    b.tick()
                b.sync()
                dt = (time.perf_counter() - t0) / a.steps
                row = dict(round=r, loudness=name, streams=a.streams, fft=a.fft, hop=a.hop, ms_per_step=round(dt * 1e3, 4),
                           Mspectra_s=round(2 * a.streams / dt / 1e6, 2))
                rows.append(row)
                print(json.dumps(row), flush=True)
        reading = on.loudness(0, 4)
        for q in pin:
            q.close()
    med = {name: float(np.median([x["ms_per_step"] for x in rows if x["loudness"] == name])) for name in ("off", "on")}
    summary = dict(median_ms_per_step=med, delta_us_per_hop=round((med["on"] - med["off"]) * 1e3, 1),
                   median_Mspectra_s={n: float(np.median([x["Mspectra_s"] for x in rows if x["loudness"] == n])) for n in ("off", "on")},
                   sample_reading={k: float(reading[k][0]) for k in ("momentary", "short_term", "integrated", "range", "true_peak")},
                   warmup=a.warmup, steps=a.steps, rounds=a.rounds)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(rows=rows, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
