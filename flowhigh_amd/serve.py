"""Batched front for the serving caller of the reference (`/root/reference/app.py:8-15`: one
`generate((sr_in, audio), sr_out, timestep)` per HTTP request, one clip at a time).

Requests from any number of caller threads are collected for a few milliseconds, grouped by (input rate,
steps) -- by steps alone with mix_rates=True, the clips' rates going on as a list; without the steps with mix_steps=True, the
requests' step counts going on as a list -- and pushed through `FlowHighSR.generate_many`: clips of ANY lengths then run as one ragged launch
sequence on the GPU (equal lengths as one batch) while every caller still gets exactly what `generate()` would
have returned for its clip alone (same per-clip noise draw when a seed is given; on a prior='device' model the seed is the
clip's key (seed, 0) and the noise is drawn on the device).  Host logic only: no gradio,
no sockets (the reference's UI / network layers are out of scope); `generate()` below has the signature of
the function `app.py` hands to `gr.Interface`.
"""
import inspect
import os
import queue
import threading
from concurrent.futures import Future

import numpy as np
import torch


MIX_RATES_DEFAULT = False


def resolve_mix_rates(mix_rates=None):
    """mix_rates= of BatchingServer: the keyword, else FH_SERVE_MIX_RATES (1 / 0), else MIX_RATES_DEFAULT."""
    if mix_rates is None:
        env = os.environ.get("FH_SERVE_MIX_RATES")
        if env not in (None, "", "0", "1"):
            raise ValueError(f"FH_SERVE_MIX_RATES must be 0 or 1, got {env!r}")
        return MIX_RATES_DEFAULT if not env else env == "1"
    return bool(mix_rates)


MIX_STEPS_DEFAULT = False


def resolve_mix_steps(mix_steps=None):
    """mix_steps= of BatchingServer: the keyword, else FH_SERVE_MIX_STEPS (1 / 0), else MIX_STEPS_DEFAULT."""
    if mix_steps is None:
        env = os.environ.get("FH_SERVE_MIX_STEPS")
        if env not in (None, "", "0", "1"):
            raise ValueError(f"FH_SERVE_MIX_STEPS must be 0 or 1, got {env!r}")
        return MIX_STEPS_DEFAULT if not env else env == "1"
    return bool(mix_steps)


class BatchingServer:
    def __init__(self, model, max_batch=32, max_wait_ms=5.0, ends=None, mix_rates=None, mix_steps=None):
        """ends: 'per_clip' | 'ragged' | None (FH_RAGGED_ENDS, else 'per_clip'), handed to generate_many: how the front and back
        end of a ragged group run (flowhighsr.resolve_ends); a wrong value is a ValueError here, not in the worker.
        mix_rates: True | False | None (FH_SERVE_MIX_RATES = 1 / 0, else MIX_RATES_DEFAULT).  True: a collected batch is
        grouped by step count only and every group is ONE generate_many call with the clips' input rates as a list.  False:
        one call per (input rate, steps), the grouping before generate_many took a rate list.  The results are the same bits
        either way.  Measured (profiles/mixed_rates.md, 24 clips over four rates): the one mixed call is 2.2-2.6 ms of ~86-90 ms
        faster than the four per-rate calls; the default is False all the same, because a default server is pinned never to
        hand two input rates to one call (tests/test_parallel_cpu.py) and models whose generate_many takes one rate stay usable.
        mix_steps: True | False | None (FH_SERVE_MIX_STEPS = 1 / 0, else MIX_STEPS_DEFAULT).  True: the step count leaves the
        group key and a group is ONE generate_many call with the requests' step counts as a list (timestep=[s_0, ...]: one ragged
        sequence with a time per clip, integrate.py's grouped form); a window of one count hands over the int it always did.
        False: one call per step count.  The same bits either way; profiles/mixed_steps.md has the measurement.  The default is
        False: a default server's grouping is pinned (tests/test_parallel_cpu.py), and a model whose generate_many takes one
        count stays usable."""
        from .flowhighsr import resolve_ends
        self.ends = resolve_ends(ends)
        self.mix_rates = resolve_mix_rates(mix_rates)
        self.mix_steps = resolve_mix_steps(mix_steps)
        # (handed on only when something asked for a form: a model whose generate_many predates ends= keeps working)
        self._ends_kw = dict(ends=self.ends) if (ends is not None or os.environ.get("FH_RAGGED_ENDS")) else {}
        self.model = model
        self.max_batch = int(max_batch)
        self.max_wait = float(max_wait_ms) / 1e3
        self._q = queue.Queue()
        self._closed = False
        self._worker = threading.Thread(target=self._run, name="flowhigh-batcher", daemon=True)
        self._worker.start()

    # ---- caller side -------------------------------------------------------------------------------
    def submit(self, audio, sr_in, timestep=1, seed=None, *, channels=None, level='peak', output_rate=None, pcm=None,
               dither=None, dither_seed=0, loudness=None, true_peak=None, limiter=None):
        """Queue one clip (int16 or float, 1-D or [1, T]); returns a Future of a float32 numpy array [T48].
        channels = 'first' ([C, T]) | 'last' ([T, C]): a multichannel clip (FlowHighSR.generate), the Future's array is
        [C, T48].  level = 'peak' | 'input' as in generate.  A shape that fits no layout is a ValueError here.
        output_rate=, pcm=, dither=, dither_seed= as in generate (dither_seed: an int s = the key (s, 0), or a (seed, stream)
        pair), checked here; requests are grouped by them too.  With pcm= the Future's array is int16, and a channels='last'
        request gets it in its own layout, [T, C], written that way on the device.  pcm='s24in32': int32 in the same shapes;
        pcm='s24': uint8 with a last axis of 3 bytes, [T, C, 3] for a channels='last' request, [C, T, 3] or [1, T, 3] otherwise.
        loudness = None | a target in LUFS as in generate: requests are grouped by it, and it is handed to generate_many only
        where a request gave it.  true_peak = None | a ceiling in dBTP, limiter = None | 'lookahead' as in generate: the same."""
        if self._closed:
            raise RuntimeError("server is closed")
        from .delivery import resolve_delivery
        from .flowhighsr import resolve_channels, resolve_level
        level = resolve_level(level)
        if isinstance(dither_seed, (tuple, list)):
            dither_seed = tuple(dither_seed)
            if len(dither_seed) != 2:
                raise ValueError(f"dither_seed of a request is an int or a (seed, stream) pair, got {dither_seed!r}")
        opt = resolve_delivery(1, output_rate, pcm, dither, [dither_seed], loudness=loudness, level=level, true_peak=true_peak,
                               limiter=limiter)
        deliv = None
        if opt is not None:
            deliv = (opt["rate"], opt["pcm"], dither, bool(pcm is not None and channels == 'last'), opt.get("loudness"),
                     opt.get("true_peak"), opt.get("limiter"), dither_seed)
        a = np.asarray(audio.detach().cpu() if isinstance(audio, torch.Tensor) else audio)
        planar = resolve_channels(a, channels)
        if channels is not None:
            a = planar                            # [C, T]
        elif a.ndim == 2:
            a = a.squeeze(0)
        fut = Future()
        self._q.put((a, int(sr_in), int(timestep), seed, fut, level, deliv))
        return fut

    def generate(self, audio, sr_out=48000, timestep=1, *, level='peak', pcm=None, dither=None, true_peak=None, limiter=None):
        """Drop-in for app.py's `generate(audio, sr_out, timestep)`: audio = (sr_in, numpy array).  A 2-D array [T, C] with
        C <= 8 < T is gradio's multichannel clip (gr.Audio(type="numpy")): it runs with channels='last' and comes back [T48, C].
        sr_out other than 48000 goes on as output_rate= where the model's generate_many takes it; pcm='int16' (dither='tpdf')
        returns the int16 array a WAV writer or a socket takes, a [T, C] clip in that layout from the device.  true_peak=,
        limiter= go on to submit where they are given."""
        kw = {}
        if true_peak is not None or limiter is not None:
            kw.update(true_peak=true_peak, limiter=limiter)
        if int(sr_out) != 48000:
            if "output_rate" not in inspect.signature(self.model.generate_many).parameters:
                raise NotImplementedError("the mel codec is fixed at 48 kHz")
            kw["output_rate"] = int(sr_out)
        if pcm is not None or dither is not None:
            kw.update(pcm=pcm, dither=dither)
        sr_in, a = audio
        if np.ndim(a) == 2 and np.shape(a)[1] <= 8 < np.shape(a)[0]:
            y = self.submit(a, sr_in, timestep, channels='last', level=level, **kw).result()
            return int(sr_out), (y if pcm is not None else y.T)
        return int(sr_out), self.submit(a, sr_in, timestep, level=level, **kw).result()

    def close(self):
        self._closed = True
        self._q.put(None)
        self._worker.join()

    # ---- worker -----------------------------------------------------------------------------------
    def _collect(self):
        """Block for the first request, then keep taking requests for max_wait or until max_batch."""
        first = self._q.get()
        if first is None:
            return None
        batch = [first]
        deadline = threading.Event()
        timer = threading.Timer(self.max_wait, deadline.set)
        timer.start()
        try:
            while len(batch) < self.max_batch and not deadline.is_set():
                try:
                    item = self._q.get(timeout=self.max_wait / 4 or 1e-4)
                except queue.Empty:
                    continue
                if item is None:
                    self._q.put(None)           # let the outer loop see the shutdown marker
                    break
                batch.append(item)
        finally:
            timer.cancel()
        return batch

    def _run(self):
        while True:
            batch = self._collect()
            if batch is None:
                return
            groups = {}
            for item in batch:
                # same step count and level; mix_rates off: same input rate too
                # ... and the same delivery (output rate, sample format, dither, layout, loudness, true peak, limiter; the dither seed
                # is the request's own)
                # (mix_steps on: any step counts, going on as a list)
                groups.setdefault((None if self.mix_rates else item[1], None if self.mix_steps else item[2], item[5],
                                   item[6] and item[6][:7]), []).append(item)
            for (sr_in, steps, level, deliv), items in groups.items():
                try:
                    # (handed on only where a request asked: a model whose generate_many predates the keywords keeps working.
                    # One [C, T] clip makes the call a channels='first' one, the mono clips beside it going as [1, T])
                    planar = any(it[0].ndim == 2 for it in items)
                    level_kw = dict(channels='first') if planar else {}
                    if level != 'peak':
                        level_kw["level"] = level
                    if deliv is not None:
                        rate, pcm, dither, interleaved, target, ceiling, limiter = deliv
                        level_kw.update({k: v for k, v in (("output_rate", rate), ("pcm", pcm), ("dither", dither),
                                                           ("loudness", target), ("true_peak", ceiling), ("limiter", limiter))
                                         if v is not None})
                        if dither is not None:
                            level_kw["dither_seed"] = [it[6][7] for it in items]
                        if interleaved:
                            level_kw["interleaved"] = True
                    if sr_in is None:
                        sr_in = [it[1] for it in items]
                        if len(set(sr_in)) == 1:          # (one rate in the window: the call it has always been)
                            sr_in = sr_in[0]
                    if steps is None:
                        steps = [it[2] for it in items]
                        if len(set(steps)) == 1:          # (one count in the window: the call it has always been)
                            steps = steps[0]
                    noise, prior = None, {}
                    if getattr(self.model, "prior", "reference") == "device":
                        # the device prior: a request's seed is its key (seed, 0); nothing is drawn on the host
                        if any(it[3] is not None for it in items):
                            prior = dict(seed=[0 if it[3] is None else int(it[3]) for it in items])
                    elif any(it[3] is not None for it in items):
                        noise = []
                        for a, sr_i, _, seed, *_ in items:
                            g = torch.Generator().manual_seed(0 if seed is None else int(seed))
                            t48 = -(-a.shape[-1] * 48000 // sr_i)
                            noise.append(self.model._draw_noise(1, t48 // 480, g))
                    outs = self.model.generate_many([it[0][None] if planar and it[0].ndim == 1 else it[0] for it in items], sr_in,
                                                    48000, steps, noise=noise, max_batch=self.max_batch, **self._ends_kw, **prior,
                                                    **level_kw)
                    for it, y in zip(items, outs):
                        y = y.detach().cpu()
                        if deliv is not None and deliv[3]:          # [T, C] from the device; a 1-D request's is [T, 1]
                            it[4].set_result((y if it[0].ndim == 2 else y.squeeze(1)).numpy())
                            continue
                        # (pcm='s24' is a byte layout: a 1-D request's stays the planar uint8 [1, T, 3])
                        it[4].set_result((y if it[0].ndim == 2 or y.ndim == 3 else y.squeeze(0)).numpy())
                except Exception as e:            # noqa: BLE001  (every waiting caller must be released)
                    for it in items:
                        if not it[4].done():
                            it[4].set_exception(e)
