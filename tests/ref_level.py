"""The six rules of multichannel clips and level-true output (DESIGN.md "Channels and level") in plain numpy: what the tests of
csrc/level.hip and of generate*(channels=, level=) compare against.  Nothing here comes from flowhigh_amd.

A clip of C channels is C rows.  Row c is divided by its own peak p_c (rule 1), shares the clip's prior (rule 2, nothing to
compute), comes out of the inverse STFT as w_c with q_c = max |w_c|, and then
  u_c = fl(w_c * p_c)                                    rule 3, one float32 multiply per sample
  level='input':  u_c                                    rule 4
  level='peak':   fl(fl(u_c / G) * 0.99),  G = max_c fl(q_c * p_c) over the rows with p_c != 0       rule 5
  a row with p_c == 0 is divided by 1 instead, gives u_c = 0 and does not count in G; G = 1 if no row counts        rule 6
Every operation is one correctly rounded float32 operation, so a kernel either has these bits or has not."""
import numpy as np

F32 = np.float32


def peak(cond):
    """p of one row: max |.| of its 48 kHz samples, as a float32"""
    return F32(np.max(np.abs(cond)))


def channel_peaks(peaks):
    """(gains, divisors) of rows with peaks p: the gain is p; the row is divided by p, or by 1 where p is zero"""
    p = np.asarray(peaks, dtype=F32)
    return p.copy(), np.where(p == 0, F32(1), p).astype(F32)


def normalise(cond, p):
    """rule 1 (and 6): the row the model sees"""
    return cond / (p if p > 0 else 1.0)


def row_gain(w, p):
    """rule 3: u = fl(w * p)"""
    return (np.asarray(w, dtype=F32) * F32(p)).astype(F32)


def group_peak(q, gains, group):
    """rule 5 / 6 for rows in groups (group ids non-decreasing): every row's G = the maximum over the rows of its group with a
    non-zero gain of fl(q * gain); 1 where that is zero or no row counts.  A q behind a zero gain is never looked at."""
    q, gains, group = np.asarray(q, dtype=F32), np.asarray(gains, dtype=F32), np.asarray(group)
    out = np.empty(len(q), dtype=F32)
    for g in np.unique(group):
        rows = np.nonzero(group == g)[0]
        m = F32(0)
        for r in rows:
            if gains[r] != 0:
                m = np.fmax(m, F32(q[r] * gains[r]))
        out[rows] = m if m > 0 else F32(1)
    return out


def peak_scale(u, G, target=0.99):
    """fl(fl(u / G) * target)"""
    return ((np.asarray(u, dtype=F32) / F32(G)).astype(F32) * F32(target)).astype(F32)


def finish(ws, ps, level):
    """rules 3-6 for ONE clip: ws = its rows' inverse-STFT outputs (float32 arrays), ps = their peaks -> the rows of the result"""
    us = [row_gain(w, p) for w, p in zip(ws, ps)]
    if level == "input":
        return us
    assert level == "peak"
    q = [F32(np.max(np.abs(np.asarray(w, dtype=F32)))) for w in ws]
    G = group_peak(q, ps, np.zeros(len(ws), dtype=np.int64))
    return [peak_scale(u, g) for u, g in zip(us, G)]
