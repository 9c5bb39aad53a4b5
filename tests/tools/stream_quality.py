"""Streaming sessions on the CPU oracle: how far stream.stitch(windows) is from the whole-clip run (profiles/streaming.md, section 3).

synth.TINY_CFG, a 1.5 s clip at 12 kHz, euler x 1, level='input'; the noise comes from prior_normal_host(first_frame=).  For three
(window, overlap, guard) settings, the defaults among them: the max-abs and RMS deviation of the stitched windows from the
whole-clip run with the session's shared prior, and the same with independent per-window keys.  Recorded, not asserted.  No GPU.

python tests/tools/stream_quality.py [--out file.jsonl]        (one JSON line)"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SR = 12000


def quality():
    """TINY_CFG, a 1.5 s clip at 12 kHz, euler x 1, through the CPU oracle (the reference's arithmetic in torch on the host)."""
    import scipy.signal
    import torch
    import ref_frontend
    from flowhigh_amd import stream as S
    from flowhigh_amd import synth
    from flowhigh_amd.prior import prior_normal_host
    from oracle import ref_cpu
    cfg = synth.TINY_CFG
    sd = synth.make_state_dict(cfg, 0)
    x = synth.lowres_clip(700, 1.5, SR)

    def run(seg, seed, stream, first):
        """level='input' of one clip: resample, divide by the peak p, sample, splice under the cutoff, inverse STFT, times p."""
        cond = scipy.signal.resample_poly(seg, 48000, SR)
        pk = np.float32(np.max(np.abs(cond)))
        cond48 = torch.tensor(cond / np.max(np.abs(cond))).unsqueeze(0).float()
        z = torch.from_numpy(prior_normal_host(seed, stream, cond48.shape[1] // 480, 256, np.float32, first_frame=first))[None]
        wav = ref_cpu.sample(sd, cfg, cond48, z, 1, "euler").squeeze(1)
        sp, ss = ref_cpu.stft_center(wav), ref_cpu.stft_center(cond48)
        cr = ref_cpu.cutoff_index(ss)
        n = min(sp.size(-1), ss.size(-1))
        res = torch.cat([ss[0, :cr, :n], sp[0, cr:, :n]], 0)
        w, _ = ref_frontend.istft_ola(ref_frontend.irfft(res.transpose(0, 1)), torch.hann_window(2048), cond48.shape[1], 2048, 480)
        return (w.numpy().astype(np.float32) * pk).astype(np.float32)

    whole = run(x, 7, 0, 0)
    rows = []
    for window_ms, overlap_ms, guard_ms in ((1000, 200, 50), (1000, 200, 0), (500, 100, 20)):
        p = S.StreamPlan(SR, window_ms, overlap_ms, guard_ms)
        for name in ("shared", "independent"):
            wins = [run(x[a:b], 7, 0 if name == "shared" else 1 + i, p.first_frame(i) if name == "shared" else 0)
                    for i, (a, b) in enumerate(p.spans(len(x)))]
            d = S.stitch(wins, p).astype(np.float64) - whole
            rows.append(dict(window_ms=window_ms, overlap_ms=overlap_ms, guard_ms=guard_ms, prior=name, windows=len(wins),
                             max_abs=float(np.abs(d).max()), rms=float(np.sqrt(np.mean(d * d)))))
            print(rows[-1], file=sys.stderr, flush=True)
    return dict(mode="quality", clip_s=1.5, signal_rms=float(np.sqrt(np.mean(whole.astype(np.float64) ** 2))),
                signal_peak=float(np.abs(whole).max()), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(quality())
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
