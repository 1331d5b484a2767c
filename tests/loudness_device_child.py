"""child process of tests/test_gpu_loudness.py::test_device_memory_paths (needs a GPU): wf_hip_push_audio_device and
wf_hip_push_pcm (float32 planar, WF_HIP_PCM_DEVICE) reading torch tensors in place, with the loudness producer on, against a
twin fed the same frames by wf_hip_push_audio.  A process of its own because torch brings its own HIP runtime and has to be
imported before libwaveform_hip.so is loaded."""
import sys
from pathlib import Path

import numpy as np
import torch  # before libwaveform_hip.so: one HIP runtime per process

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import waveform_amd as wf  # noqa: E402

torch.cuda.set_device(0)
streams, cap, frames = 5, 2, 800
cfg = wf.Config.defaults(fft_size=1024, sample_rate=48000, capture_channels=cap, stereo=1, bars=1, slope=1.0)
for path in ("device", "pcm_f32_planar_device"):
    rng = np.random.default_rng(2)
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        b.enable_loudness()
        twin.enable_loudness()
        for t in range(60):
            pkt = rng.uniform(-0.7, 0.7, (streams, cap, frames)).astype(np.float32)
            d = torch.from_numpy(pkt).to("cuda:0")
            torch.cuda.synchronize()
            if path == "device":
                b.push_audio_device(d.data_ptr(), streams, frames)
            else:
                b.push_pcm(d, interleaved=False)
            twin.push_audio(pkt)
            b.sync()  # the tensor may go
        got, want = b.loudness(), twin.loudness()
        assert got.tobytes() == want.tobytes(), (path, got, want)
        assert np.all(got["frames"] == 60 * frames)
    print(f"{path}: ok", flush=True)
print("loudness device ok", flush=True)
