"""child process of tests/test_gpu_pitch.py::test_device_memory_path (needs a GPU): wf_hip_push_audio_device reading a torch
tensor in place, against a twin fed the same frames by wf_hip_push_audio: WF_HIP_OUT_PITCH reads bit-identically.  A process
of its own because torch brings its own HIP runtime and has to be imported before libwaveform_hip.so is loaded."""
import sys
from pathlib import Path

import torch  # before libwaveform_hip.so: one HIP runtime per process

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import waveform_amd as wf  # noqa: E402
import pitch_cases as cases  # noqa: E402

torch.cuda.set_device(0)
streams, cap, frames = 5, 2, 801
cfg = wf.Config.defaults(fft_size=1024, sample_rate=cases.SR, capture_channels=cap, stereo=1, bars=1, slope=1.0)
src = cases.bank(21, streams, cap, 3 * frames)
with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
    for t in range(3):
        pkt = src[:, :, t * frames:(t + 1) * frames].copy()
        d = torch.from_numpy(pkt).to("cuda:0")
        torch.cuda.synchronize()
        b.push_audio_device(d.data_ptr(), streams, frames)
        twin.push_audio(pkt)
        b.sync()  # the tensor may go
    got, want = b.pitch(), twin.pitch()
    assert got.tobytes() == want.tobytes() and got["lag"].all(), (got, want)
print("pitch device ok", flush=True)
