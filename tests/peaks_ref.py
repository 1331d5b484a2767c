"""Float64 restatement of WF_HIP_OUT_PEAKS (include/wf_hip.h, "spectral peaks"): the strongest local maxima of an
m_decibels row and the parabola through each of them and its two neighbours."""
import numpy as np

MAX_PEAKS = 8


def peaks(rows, floor_db, sample_rate, fft_size):
    """rows: [..., M] as WF_HIP_OUT_DECIBELS returns them.  Returns count [...], k [..., 8] (-1 unused), hz and db [..., 8]
    (unused: 0 / -inf), the interpolation in float64 from the rows' float32 values."""
    rows = np.asarray(rows)
    lead, M = rows.shape[:-1], rows.shape[-1]
    flat = rows.reshape(-1, M)
    count = np.zeros(flat.shape[0], np.int64)
    ks = np.full((flat.shape[0], MAX_PEAKS), -1, np.int64)
    hz = np.zeros((flat.shape[0], MAX_PEAKS), np.float64)
    db = np.full((flat.shape[0], MAX_PEAKS), -np.inf, np.float64)
    for i, r32 in enumerate(flat):
        d = r32.astype(np.float64)
        k = np.arange(1, M - 1)
        v = d[1:-1]
        cand = k[(v > d[:-2]) & (v >= d[2:]) & (v > floor_db)]
        order = np.lexsort((cand, -d[cand]))[:MAX_PEAKS]  # value descending, then lower bin first
        sel = cand[order]
        a, b, c = d[sel - 1], d[sel], d[sel + 1]
        p = 0.5 * (a - c) / (a - 2.0 * b + c)
        n = sel.size
        count[i] = n
        ks[i, :n] = sel
        hz[i, :n] = (sel + p) * sample_rate / fft_size
        db[i, :n] = b - 0.25 * (a - c) * p
    return (count.reshape(lead), ks.reshape(lead + (MAX_PEAKS,)), hz.reshape(lead + (MAX_PEAKS,)),
            db.reshape(lead + (MAX_PEAKS,)))
