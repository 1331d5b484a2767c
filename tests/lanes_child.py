"""TEST HARNESS (child of tests/test_gpu_lanes.py): runs against the DEVELOPMENT build of the library (libwaveform_hip_dev.so via
WF_HIP_LIB -- the release library reads no WF_HIP_LANES).

wf_hip_tick issues a spectrum batch as up to four slices of streams ("lanes"), each on a HIP stream of its own; on a lane every
kernel of the tick adds stream_base to whatever it indexes.  The lanes rule only fires from thousands of streams on, so the mixed
batches of tests/test_gpu_mixed_states.py (4-7 streams) all run on one lane.  Here the same batches are played with
WF_HIP_LANES = 1, 2, 3 and 4 (above 16384 samples: 1 and 4, see LANE_COUNTS_LARGE): the lane count is min(WF_HIP_LANES, 4,
streams), so the slices hold one or two streams and start at odd streams.  Per case:
  1. launches_per_tick() is the lane count asked for (a build that ignores the variable fails here) and kernel_name() names the
     family the case is there for;
  2. the records of every lane count equal the one-lane records bit for bit -- rows, display, m_last_silent and vertices, every
     tick, every stream;
  3. the four-lane records are held against every stream's own script played alone on the checker, through the comparison of
     test_gpu_mixed_states.run_case (no tolerance of this module's own);
  4. by arithmetic on the stream count: some slice starts at an odd stream, and with one captured channel (two STREAMS share a
     workgroup) some slice holds an odd number of streams, i.e. its last workgroup is half empty.

The kind "mirror" is the mirror hand-over (wf_hip_bars_mirror_ready, wf_hip_copy_bars_device_async) on three lanes.

usage: python tests/lanes_child.py <case id> | mirror | device_rms"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scenarios  # noqa: E402
import test_gpu_mixed_states as mixed  # noqa: E402

MAX_LANES = 4
LANE_COUNTS = (1, 2, 3, 4)
# Above 16384 samples (four streams per batch) only one and four lanes are played: a case costs 0.6 ... 1.2 s, most of it the
# child process itself, against 0.02 ... 0.5 s for its twin in test_gpu_mixed_states.py, and the replays of the large sizes are
# the part of that which can go.  Four lanes on four streams still give every slice but the first an odd or a non-zero base
# and one stream; slices of several streams at these sizes run in test_gpu_fullsize.test_lanes_on_the_one_workgroup_per_cu_kernels.
LANE_COUNTS_LARGE = (1, 4)


def lane_counts(n):
    return LANE_COUNTS if n <= 16384 else LANE_COUNTS_LARGE


def _table():
    """id -> arguments of test_gpu_mixed_states.Case, the seeds fixed here"""
    out = {}
    for n, layout, display, seed, aligned in mixed.CASES:
        out[f"{n}-{layout}-{display}-s{seed}{'-aligned' if aligned else ''}"] = dict(n=n, layout=layout, display=display, seed=seed, aligned=aligned)
    seed = len(mixed.CASES)
    more = [
        # the mixed-radix transform beyond a CU's LDS in one kernel, which SHAPES lacks
        ("32000-stereo-bars", dict(n=32000, layout="stereo", display="bars", kernel="big_mr_whole_kernel")),
        ("32000-mixdown-none", dict(n=32000, layout="mixdown", display="none", kernel="big_mr_whole_kernel")),
        # vertex_fill_kernel behind every lane's tick: vertex_args(h, lo, hi)
        ("verts-2048-stereo-curve", dict(n=2048, layout="stereo", display="curve", extra=dict(vertices=1), verts=True)),
        ("verts-1024-mono-stepped", dict(n=1024, layout="mono", display="bars", extra=dict(vertices=3, step_width=3, step_gap=1), verts=True)),
        ("verts-4096-stereo-caps", dict(n=4096, layout="stereo", display="bars", extra=dict(rounded_caps=1, vertices=1), verts=True)),
        # the display derived from the stored rows (big_outputs_kernel, (hi - lo) * display channels rows per lane): the
        # configuration of scenario curve_1024_3840_gauss32
        ("ext-1024-stereo-curve-3840-gauss32", dict(n=1024, layout="stereo", display="curve", extra=dict(interp_mode=2, width=3840, filter_mode=1, filter_radius=32.0),
                                                    ext=True)),
        # per-stream gain words (wf_hip_set_input_rms): test_mixed_batch_with_volume_normalisation's rms="set" form
        ("rms-set-2048-stereo", dict(n=2048, layout="stereo", display="bars", seed=100 + 2048 + len("stereo"), extra=mixed.NORMALIZE, rms="set", kernel="N=2048,")),
        ("rms-set-800-mono", dict(n=800, layout="mono", display="bars", seed=100 + 800 + len("mono"), extra=mixed.NORMALIZE, rms="set", kernel="mixed radix")),
    ]
    for k, (name, kw) in enumerate(more):
        kw.setdefault("seed", seed + k)
        out[name] = kw
    return out


CASES = _table()
KINDS = list(CASES) + ["mirror", "device_rms"]


class _Lanes:
    """WF_HIP_LANES in force for the handles created inside, the environment as it was afterwards"""

    def __init__(self, k):
        self.k = int(k)

    def __enter__(self):
        self.old = os.environ.get("WF_HIP_LANES")
        os.environ["WF_HIP_LANES"] = str(self.k)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("WF_HIP_LANES", None)
        else:
            os.environ["WF_HIP_LANES"] = self.old


def slices(S, lanes):
    """wf_hip_tick's slices of a batch of S streams on `lanes` lanes"""
    return [(S * l // lanes, S * (l + 1) // lanes) for l in range(lanes)]


def _bits(v):
    return np.ascontiguousarray(v).tobytes()


def _digest(records):
    import hashlib
    h = hashlib.sha256()
    for recs in records:
        for r in recs:
            h.update(bytes([r["silent"]]) + _bits(r["db"]) + (b"" if r["bars"] is None else _bits(r["bars"])))
            for v in r.get("verts", []):
                h.update(_bits(v))
    return h.hexdigest()[:16]


def assert_records_equal(got, one, what):
    """bit for bit, every stream, every tick: db, bars, silent and the vertices where present"""
    assert len(got) == len(one)
    for i, (gs, ws) in enumerate(zip(got, one)):
        assert len(gs) == len(ws)
        for t, (g, w) in enumerate(zip(gs, ws)):
            at = f"{what} stream {i} tick {t}"
            assert g["silent"] == w["silent"], f"{at}: m_last_silent {g['silent']} != {w['silent']} on one lane"
            assert g["db"].shape == w["db"].shape and _bits(g["db"]) == _bits(w["db"]), f"{at}: the rows differ from the one-lane rows"
            assert (g["bars"] is None) == (w["bars"] is None), f"{at}: one side has no display"
            if w["bars"] is not None:
                assert g["bars"].shape == w["bars"].shape and _bits(g["bars"]) == _bits(w["bars"]), f"{at}: the display differs from the one-lane display"
            assert ("verts" in g) == ("verts" in w), f"{at}: one side has no vertices"
            if "verts" in w:
                assert len(g["verts"]) == len(w["verts"])
                for c, (gv, wv) in enumerate(zip(g["verts"], w["verts"])):
                    assert gv.shape == wv.shape and _bits(gv) == _bits(wv), f"{at} channel {c}: the vertices differ from the one-lane vertices ({gv.shape} / {wv.shape})"


def run_mixed(name):
    kw = dict(CASES[name])
    want_verts, ext = kw.pop("verts", False), kw.pop("ext", False)
    case = mixed.Case(**kw)
    cfg, S = case.cfg, case.S
    counts = lane_counts(case.n)
    per_launch = None
    played = {}
    t0 = time.perf_counter()
    for k in counts:
        with _Lanes(k):
            got, kname, launches = mixed.play_hip(case)
        if per_launch is None:
            # one lane: 2 where a mono mixdown runs channel 1 a launch ahead of channel 0 (TransformPlan::split_mono: 32768 and the
            # sizes whose rows take that geometry), 1 everywhere else
            per_launch = launches
            mixdown = cfg.capture_channels == 2 and not cfg.stereo
            allowed = (1,) if not mixdown else (2,) if case.n == 32768 else (1, 2)
            assert per_launch in allowed, (case.what, kname, launches)
        assert launches == min(k, S) * per_launch, f"{case.what}: WF_HIP_LANES={k} gave {launches} launches per tick ({kname}); {min(k, S) * per_launch} expected"
        played[k] = got
    t_hip = time.perf_counter() - t0
    print(f"ONE-LANE case={name} sha256={_digest(played[1])}")  # (what a change to the lanes must leave as it is)
    if want_verts:
        assert all("verts" in rec for recs in played[1] for rec in recs), f"{case.what}: the records carry no vertices"
    if ext:
        _assert_ext_outputs(cfg, case.what)
    for k in counts[1:]:
        assert_records_equal(played[k], played[1], f"{case.what} on {min(k, S)} lanes")
    # the slices the batch ran as: some start at an odd stream; mono capture: some hold an odd number of streams, so that the
    # last of the slice's two-stream workgroups is half empty
    every = [sl for k in counts[1:] for sl in slices(S, min(k, S))]
    assert any(lo % 2 == 1 for lo, hi in every), (S, every)
    if int(cfg.capture_channels) == 1:
        assert any((hi - lo) % 2 == 1 for lo, hi in every), (S, every)
    t0 = time.perf_counter()
    with mixed._Counted():
        mixed.compare_with_solo(case, played[MAX_LANES])
    t = mixed.TOTALS
    print(f"TOTALS case={name} hip_s={t_hip:.2f} reference_s={time.perf_counter() - t0:.2f} values={t['values']} linear_arm={t['linear_arm']} "
          f"visible={t['linear_arm_visible']} deep={t['deep']} display_checks={t['display_checks']} display_arm={t['display_arm']}")


def _assert_ext_outputs(cfg, what):
    """the handle derives its display from the stored rows: such a handle -- and at a power-of-two size up to 32768 only such a
    one -- refuses further bars buffers (WF_HIP_ERR_UNSUPPORTED); the refusal comes before the pointers are looked at"""
    import waveform_amd as wf
    with wf.SpectrumBatch(cfg, 4) as b:
        try:
            b.set_bars_mirrors([0x1000], [0x2000])
        except wf.WfHipError as e:
            assert e.code == -2, f"{what}: {e}"
        else:
            raise AssertionError(f"{what}: the tick kernel finishes this display itself -- not the configuration the case is there for")


def run_device_rms():
    """the device RMS producer keeps a batch on one lane by design (update_input_rms runs on the handle's stream ahead of every tick)"""
    import waveform_amd as wf
    cfg = scenarios.make_config(mixed.case_config(2048, "mono", "bars", mixed.NORMALIZE))
    with _Lanes(MAX_LANES):
        with wf.SpectrumBatch(cfg, 7) as b:
            assert b.launches_per_tick() == MAX_LANES, b.launches_per_tick()  # (the variable is read ...)
            b.enable_input_rms()
            assert b.launches_per_tick() == 1, b.launches_per_tick()          # (... and the producer overrules it)


def run_mirror():
    """N = 1024 stereo bars, 5 streams on three lanes (slices [0, 1), [1, 3), [3, 5)), as test_gpu_late_settings.test_bars_mirrors_set_late"""
    import waveform_amd as wf
    from tools import synth
    from test_gpu_reset import _Hip, same, HIDDEN, PAUSED
    from test_gpu_late_settings import _cfg, _lead, HOP, SEED
    n, streams, ticks = 1024, 5, 3
    cfg = _cfg(n)
    with _Lanes(3):
        b = wf.SpectrumBatch(cfg, streams, ring_frames=_lead(n) + HOP * (ticks + 1))
    with b:
        assert b.launches_per_tick() == 3, b.launches_per_tick()
        assert slices(streams, 3) == [(0, 1), (1, 3), (3, 5)]
        hip = _Hip()
        shape = (streams, b.display_channels, b.num_bars)
        sets = [hip.alloc(int(np.prod(shape)) * 4) for _ in range(2)]
        first, count = 2, 2  # streams 2 and 3: the end of slice 1 and the start of slice 2
        part = hip.alloc(count * shape[1] * shape[2] * 4)
        consumer = hip.stream()
        try:
            b.set_bars_mirrors([sets[0]], [sets[1]])
            seen = []
            # before any tick: no tick has written the set, the handle's own bars stand in
            ptr = b.bars_mirror_ready(consumer)
            assert ptr in sets
            seen.append(ptr)
            assert hip.stream_sync(consumer) == 0
            assert same(hip.download(ptr, shape), b.bars()), "mirror set handed over before any tick"
            b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, 0, _lead(n)))
            for t in range(ticks):
                b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, _lead(n) + t * HOP, HOP))
                state = np.zeros(streams, np.uint8)
                if t == 1:
                    state[1], state[3] = PAUSED, HIDDEN
                b.set_hidden(state)
                b.tick()
                ptr = b.bars_mirror_ready(consumer)
                assert ptr in sets and ptr != seen[-1], "the sets take turns"
                seen.append(ptr)
                b.copy_bars_to_device_async(part, consumer, first, count)
                assert hip.stream_sync(consumer) == 0
                bars = b.bars()
                assert np.isfinite(bars).all()
                assert same(hip.download(ptr, shape), bars), f"mirror set handed over after tick {t}"
                assert same(hip.download(part, (count,) + shape[1:]), b.bars(first, count)), f"bars of streams {first}..{first + count - 1} copied after tick {t}"
                assert same(bars[first:first + count], b.bars(first, count))
            assert not same(bars[0], bars[1]), "the streams hear different audio"
        finally:
            b.sync()
            hip.stream_destroy(consumer)
            for p in sets + [part]:
                hip.free(p)


if __name__ == "__main__":
    import waveform_amd as wf
    assert hasattr(wf.lib(), "wf_hip_debug_age"), "needs the development build (WF_HIP_LIB=waveform_amd/libwaveform_hip_dev.so)"
    kind = sys.argv[1]
    if kind == "mirror":
        run_mirror()
    elif kind == "device_rms":
        run_device_rms()
    else:
        run_mixed(kind)
    print("lanes ok")
