"""child process of tests/test_gpu_bands.py::test_device_memory_path (needs a GPU): audio pushed by wf_hip_push_audio_device from a
torch tensor in place, against a twin fed the same frames by wf_hip_push_audio: after the same ticks WF_HIP_OUT_BANDS reads
bit-identically and within the contract's bound of the restatement.  A process of its own because torch brings its own HIP
runtime and has to be imported before libwaveform_hip.so is loaded."""
import sys
from pathlib import Path

import torch  # before libwaveform_hip.so: one HIP runtime per process

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import waveform_amd as wf  # noqa: E402
import bands_ref as ref  # noqa: E402
from tools import synth  # noqa: E402

torch.cuda.set_device(0)
streams, cap, frames = 5, 2, 801
cfg = wf.Config.defaults(fft_size=1024, sample_rate=48000, capture_channels=cap, stereo=1, bars=1, slope=1.0)
with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
    for t in range(3):
        pkt = synth.block(21, 0, streams, cap, t * frames, frames)
        d = torch.from_numpy(pkt).to("cuda:0")
        torch.cuda.synchronize()
        b.push_audio_device(d.data_ptr(), streams, frames)
        twin.push_audio(pkt)
        b.tick()
        twin.tick()
        b.sync()  # the tensor may go
    got, want = b.bands(), twin.bands()
    assert got.tobytes() == want.tobytes() and np.all(np.isfinite(got["total_db"])), (got, want)
    bad = ref.mismatches(got, ref.bands(b.decibels(), b.table_window()[0], cfg.sample_rate, b.fft_size))
    assert not bad, bad
print("bands device ok", flush=True)
