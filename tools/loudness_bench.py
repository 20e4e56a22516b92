"""Cost of loudness normalisation on the GPU (BS.1770-4 target under a peak ceiling; DESIGN
§4.3d), written to profiles/loudness_bench.json.  Every figure is a median over --runs runs
(>= 3) with its min and max beside it.

  stage     one 3.2 s item (102400 samples at 32 kHz) to 48 kHz int16, HIP events around the call:
              convert    gsv_audio_convert: the output stage alone, as the parent commit has it;
              normalize  gsv_audio_normalize at -16 LUFS: the four measurement launches, then the
                         stage with the gain (call times, not kernel times);
              measure    gsv_audio_loudness alone.
  batch64   the 64 utterances of configs[2] through Engine.vits_decode_batch as 48 kHz int16 with
            loudness=-16 on every item (one measurement pass + one stage launch), with the stage
            alone, and without either: three call times whose differences hold the two stages.
  stream    the configs[1] sentence stream of bench.py (--steps sentences, vocoder on 64 CUs), each
            sentence delivered to the host as 48 kHz int16 bytes:
              gpu    sample_rate=48000, pcm16=True, loudness=-16 on the vocoder item;
              plain  the same stream without loudness (the parent commit's path);
              host   that stream, and per sentence what a caller does without the stage: the
                     float64 BS.1770-4 oracle (tests/loudness_oracle.py: scipy's lfilter, numpy)
                     over the 48 kHz PCM, the gain, and the int16 conversion again.
            The three alternate within a run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGET = -16.0


def _stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=len(v))


def _event_ms(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stage(torch, eng, runs, iters):
    import ctypes
    from genie_tts_amd.engine import _stream, lib
    x = (torch.rand(1280 * 80, device=eng.dev) * 2 - 1) * 0.3
    stats = torch.empty(4, device=eng.dev)
    forms = dict(convert=lambda: eng.audio_convert(x, 48000, pcm16=True),
                 normalize=lambda: eng.audio_convert(x, 48000, pcm16=True, loudness=TARGET),
                 measure=lambda: lib().gsv_audio_loudness(eng.h, ctypes.c_void_p(x.data_ptr()), x.numel(),
                                                          ctypes.c_void_p(stats.data_ptr()), _stream()))
    out = {}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        meds = [float(np.median([_event_ms(torch, fn) for _ in range(iters)])) * 1e3 for _ in range(runs)]
        out[name] = dict(call_us=_stat(meds))
    out["n_in"] = x.numel()
    out["loudness_lufs"], out["peak"] = eng.audio_loudness(x)
    return out


def batch64(torch, run, runs):
    eng = run.eng
    utts = [(run.d_ref, t, run.d_ref_bert, b, run.d_ssl, it.force_steps)
            for t, b, it in zip(run.d_txt, run.berts(0, len(run.items)), run.items)]
    sems = eng.t2s_generate(utts, run.sp)
    cond = dict(ge=run.ge_v2)
    plain = [dict(text_seq=t, pred_semantic=s, noise_seed=7 + i, **cond) for i, (t, s) in enumerate(zip(run.d_txt, sems))]
    rated = [dict(it, sample_rate=48000, pcm16=True) for it in plain]
    loud = [dict(it, loudness=TARGET) for it in rated]
    forms = (("with_loudness", loud), ("with_stage", rated), ("without", plain))
    ms = {name: [] for name, _ in forms}
    for _, items in forms:
        eng.vits_decode_batch(items)
    torch.cuda.synchronize()
    for r in range(runs):
        for name, items in forms[r % 3:] + forms[:r % 3]:
            ms[name].append(_event_ms(torch, lambda: eng.vits_decode_batch(items)))
    res = {name: dict(call_ms=_stat(v)) for name, v in ms.items()}
    res["items"] = len(plain)
    res["samples_32k"] = int(sum(1280 * int(s.size) for s in sems))
    return res


def host_normalize(pcm, rate=48000):
    """What a caller does on the host: measure the PCM (float64 BS.1770-4), scale, convert again."""
    from tests import loudness_oracle as O
    x = pcm.astype(np.float64) / 32767.0
    m = O.measure(x, rate)
    g = O.gain(m["loudness"], m["peak"], TARGET, None, m["blocks_kept"])
    return np.clip(x * g * 32767.0, -32768.0, 32767.0).astype(np.int16)


def stream_once(run, n, mode):
    """bench.Runner.stream with each sentence delivered to the host as `mode` says; -> bytes out."""
    eng = run.eng
    utts = [(run.d_ref, t, run.d_ref_bert, run.d_bert[0], run.d_ssl, run.items[0].force_steps)
            for t in (run.d_txt[0], run.d_txt[0].clone())]
    utt = lambda i: utts[i % 2]
    cond = dict(ge=run.ge_v2)
    fmt = dict(sample_rate=48000, pcm16=True)
    if mode == "gpu":
        fmt["loudness"] = TARGET
    nbytes = 0

    def deliver(t):
        pcm = t.cpu().numpy()
        if mode == "host":
            pcm = host_normalize(pcm)
        return len(pcm.tobytes())
    eng.t2s_prefetch(utt(1), run.sp)
    eng.t2s_generate_start(utt(0), run.sp)
    pending = None
    for i in range(n):
        if i + 1 < n:
            if i + 2 < n:
                eng.t2s_prefetch(utt(i + 2), run.sp)
            eng.t2s_generate_start(utt(i + 1), run.sp)
        sem = eng.t2s_generate_finish()
        if pending is not None:
            eng.vits_wait()
            nbytes += deliver(pending)
        pending = eng.vits_decode_async(dict(text_seq=utt(i)[1], pred_semantic=sem, noise_seed=run.seed, **cond, **fmt))
    eng.vits_wait()
    nbytes += deliver(pending)
    return nbytes


def stream(torch, run, runs, steps):
    eng = run.eng
    eng.set_vocoder_cus(64)
    try:
        modes = ("plain", "gpu", "host")
        for m in modes:
            stream_once(run, 4, m)
        torch.cuda.synchronize()
        ms = {m: [] for m in modes}
        for r in range(runs):
            for m in modes[r % 3:] + modes[:r % 3]:   # alternate, rotating the order
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stream_once(run, steps, m)
                torch.cuda.synchronize()
                ms[m].append((time.perf_counter() - t0) * 1e3 / steps)
        return {m: dict(ms_per_utterance=_stat(v)) for m, v in ms.items()} | dict(steps=steps)
    finally:
        eng.set_vocoder_cus(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="stage: calls per run")
    ap.add_argument("--steps", type=int, default=100, help="stream: sentences per run")
    ap.add_argument("--only", choices=("stage", "batch64", "stream"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs: at least 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench needs a GPU: there is no CPU path to time")
    import bench
    from genie_tts_amd import workloads
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "target_lufs": TARGET}
    if a.only in (None, "stage", "stream"):
        wl = workloads.single()
        run = bench.Runner(wl, wl.items, dev, 0)
        try:
            if a.only in (None, "stage"):
                res["stage"] = stage(torch, run.eng, a.runs, a.iters)
            if a.only in (None, "stream"):
                res["stream"] = stream(torch, run, a.runs, a.steps)
        finally:
            run.eng.close()
    if a.only in (None, "batch64"):
        wl = workloads.batch64()
        run = bench.Runner(wl, wl.items, dev, 0)
        try:
            res["batch64"] = batch64(torch, run, a.runs)
        finally:
            run.eng.close()
    print(json.dumps(res), flush=True)
    if a.only is None:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
