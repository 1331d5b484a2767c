"""child process of tests/test_gpu_signal.py::test_device_memory_paths (needs a GPU): wf_hip_push_audio_device and
wf_hip_push_pcm (s16 interleaved and float32 planar, WF_HIP_PCM_DEVICE) reading torch tensors in place, against a twin fed
the converted float32 frames by wf_hip_push_audio: WF_HIP_OUT_SIGNAL reads bit-identically.  A process of its own because
torch brings its own HIP runtime and has to be imported before libwaveform_hip.so is loaded."""
import sys
from pathlib import Path

import numpy as np
import torch  # before libwaveform_hip.so: one HIP runtime per process

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import waveform_amd as wf  # noqa: E402
from pcm_convert import captured, random_packet  # noqa: E402

torch.cuda.set_device(0)
streams, cap, frames = 5, 2, 801
cfg = wf.Config.defaults(fft_size=1024, sample_rate=48000, capture_channels=cap, stereo=1, bars=1, slope=1.0)
for path in ("device", "pcm_s16_interleaved_device", "pcm_f32_planar_device"):
    rng = np.random.default_rng(2)
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        for t in range(3):
            if path == "device":
                pkt = rng.uniform(-1.0, 1.0, (streams, cap, frames)).astype(np.float32)
                d = torch.from_numpy(pkt).to("cuda:0")
                torch.cuda.synchronize()
                b.push_audio_device(d.data_ptr(), streams, frames)
                conv = pkt
            else:
                inter = path.startswith("pcm_s16")
                pkt = random_packet(rng, np.int16 if inter else np.float32, streams, cap, frames, inter)
                d = torch.from_numpy(pkt).to("cuda:0")
                torch.cuda.synchronize()
                b.push_pcm(d, interleaved=inter)
                conv = captured(pkt, inter, 0, cap)
            twin.push_audio(conv)
            b.sync()  # the tensor may go
        got, want = b.signal(), twin.signal()
        assert got.tobytes() == want.tobytes(), (path, got, want)
    print(f"{path}: ok", flush=True)
print("signal device ok", flush=True)
