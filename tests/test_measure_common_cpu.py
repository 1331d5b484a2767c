"""The shared harness of the measurement outputs' GPU tests feeds the device what the copies it replaced fed it: packets() cuts
as both `_packets` did, and wrap_child.Walk pushes, labels and counts as the loop of every <out>_wrap_child.py did.  The expected
values were recorded from that earlier code, on the CPU; the loop is restated here from it as well."""
import numpy as np
import pytest

from measure_common import packets
from wrap_child import HOPS, Schedule, Walk

RING = 8192
# name: R, win (the Schedule's), span (the frames a read looks back over); wrap = R - win
SCHEDULES = {"bits": (2 * RING, 2048, 2048), "sono": (3 * RING - 1024, RING, RING - 1)}

# recorded from `_packets(np.random.default_rng(seed), total)` of test_gpu_bits.py (rng.integers(1, 701)) and of test_gpu_cq.py (1, 700)
CUTS = {
    (700, 2048, 3001): [(0, 641), (641, 1186), (1186, 1397), (1397, 2016), (2016, 2170), (2170, 2704), (2704, 3001)],
    (700, 5, 5000): [(0, 470), (470, 1034), (1034, 1050), (1050, 1616), (1616, 1945), (1945, 2306), (2306, 2748), (2748, 2949), (2949, 3635),
                     (3635, 3673), (3673, 3868), (3868, 4137), (4137, 4537), (4537, 4823), (4823, 4915), (4915, 4947), (4947, 4948), (4948, 4983),
                     (4983, 5000)],
    (699, 1024, 3001): [(0, 392), (392, 618), (618, 1232), (1232, 1413), (1413, 1476), (1476, 1735), (1735, 2259), (2259, 2878), (2878, 3001)],
    (699, 11, 5000): [(0, 94), (94, 184), (184, 742), (742, 1091), (1091, 1504), (1504, 1925), (1925, 2423), (2423, 2444), (2444, 2784),
                      (2784, 2888), (2888, 3169), (3169, 3818), (3818, 4201), (4201, 4251), (4251, 4631), (4631, 4722), (4722, 5000)],
}

# recorded from the children's loop: (pushes, frames, reads, (before, straddling, exact, behind)), the first, a middle and the last label
RECORDED = {
    "bits": (18, 18903, 15, (4, 5, 1, 5), "read 3 at wpos = 2^32-1278", (10, 15651, "read 10 at wpos = 2^32+1315"), "read 17 at wpos = 2^32+4567"),
    "sono": (33, 26071, 30, (4, 20, 0, 6), "read 3 at wpos = 2^32-1278", (18, 20472, "read 18 at wpos = 2^32+5112"), "read 32 at wpos = 2^32+10711"),
}


@pytest.mark.parametrize("key", CUTS, ids=lambda k: f"most{k[0]}-seed{k[1]}-total{k[2]}")
def test_packets_cut_as_both_copies_did(key):
    most, seed, total = key
    assert packets(np.random.default_rng(seed), total, most) == CUTS[key]


class Recorder:
    """a stand-in twin: keeps what it is pushed"""

    def __init__(self):
        self.pushed = []

    def push_audio(self, a):
        self.pushed.append(a)


def _earlier_loop(sch, wrap, span):
    """the loop every child carried: which pushes are read, under which label, and the counters (the sono family's `behind` was
    this `exact + behind`)"""
    T, before, straddling, exact, behind, reads = 0, 0, 0, 0, 0, []
    for i, p in enumerate(sch.pushes):
        T += p
        if T < wrap - sum(HOPS):
            continue
        reads.append((i, T, f"read {i} at wpos = 2^32{T - wrap:+d}"))
        before += int(T <= wrap)
        straddling += int(0 < T - wrap < span)
        exact += int(T - wrap == span)
        behind += int(T - wrap > span)
    return reads, (before, straddling, exact, behind)


@pytest.mark.parametrize("name", SCHEDULES)
def test_the_walk_is_the_loop_the_children_carried(name):
    R, win, span = SCHEDULES[name]
    sch = Schedule(R, win, 0, big=RING // 2, fine=True)
    sch.check([0])
    wrap = R - win
    fresh, old = Recorder(), Recorder()
    drawn = []

    def audio(i, T, p):
        drawn.append((i, T, p))
        return np.full((1, 2, p), i, np.float32)

    w = Walk((fresh, old), sch.pushes, wrap, span, audio, hist=np.zeros((1, 2, win), np.float32))
    reads, hists = [], []
    for r in w:
        reads.append(r)
        hists.append(w.hist)
    want, counters = _earlier_loop(sch, wrap, span)
    assert reads == want and w.counts == counters and w.T == sum(sch.pushes)
    pushes, frames, n, recorded, first, (i, T, middle), last = RECORDED[name]
    assert (len(sch.pushes), w.T, len(reads), w.counts) == (pushes, frames, n, recorded)
    assert reads[0][2] == first and reads[n // 2] == (i, T, middle) and reads[-1][2] == last
    # every push went to both twins once, in order, drawn once with the frames before it
    starts = np.concatenate([[0], np.cumsum(sch.pushes)[:-1]])
    assert drawn == [(k, int(t), p) for k, (t, p) in enumerate(zip(starts, sch.pushes))]
    for twin in (fresh, old):
        assert [a.shape[2] for a in twin.pushed] == sch.pushes and all(np.all(a == k) for k, a in enumerate(twin.pushed))
    assert all(a is b for a, b in zip(fresh.pushed, old.pushed))
    # hist at a read: the newest `win` frames, the zeros of create before them
    everything = np.concatenate([np.zeros((1, 2, win), np.float32)] + fresh.pushed, axis=2)
    for (_, T, _), h in zip(reads, hists):
        assert np.array_equal(h, everything[:, :, T:T + win])
    # the coverage each family asserts
    before, straddling, exact, behind = w.counts
    if name == "bits":
        assert before >= 2 and straddling >= 3 and exact == 1 and behind >= 3
    else:
        assert before >= 2 and straddling >= 3 and exact + behind >= 3


def test_marked_pushes_are_read_and_no_others():
    """tempo's and hum's children give (frames, read) and count the read at the wrap itself"""
    pushes = [(4096, False), (4096, True), (100, False), (37, True), (8192, True), (1, True)]
    w = Walk((Recorder(),), pushes, 8192, 8192, lambda i, T, p: np.zeros((1, 2, p), np.float32))
    assert [(i, T) for i, T, _ in w] == [(1, 8192), (3, 8329), (4, 16521), (5, 16522)]
    assert (w.before, w.at, w.straddling, w.exact, w.behind) == (1, 1, 1, 0, 2) and w.T == 16522
