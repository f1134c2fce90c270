#!/usr/bin/env python3
"""First-audio latency and total time of streamed synthesis on the headline model (MoL rnn/fc 512,
401 frames = 5 s), against the one-shot generate() of the same process.

    python tools/stream_latency.py [--chunks 4 8 32] [--reps 5] [--frames 401]

Per chunk size c (mel frames per push), total_frames announced (no 21-frame hold-back) and not:
  (a) first audio: the push that brings the session to the first frame count at which c frames of
      audio are final (c + lookahead frames when the total is known, c + 21 when it is not) — host
      time from entering push() to the float64 samples being in host memory (push synchronises and
      copies), and the device time between HIP events recorded around it;
  (b) total: all 401 frames pushed c at a time, every push's audio copied to the host — host time
      from the first push to the last sample on the host, device time likewise, and the number of
      pushes that launched the persistent kernel.
Every shape is warmed by one untimed session first (code objects, rocBLAS algorithm choice); each
figure is the median of --reps fresh sessions (a session allocates its workspaces in its first
pushes: that is part of what a caller waits for, and it is included).  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavernn_amd import synthetic as syn                     # noqa: E402
from wavernn_amd.fatchord_version import WaveRNN             # noqa: E402
from wavernn_amd.loop import stream_plan                     # noqa: E402


def _timed(fn, dev):
    """(result, host ms to completion, device ms between events around fn)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    return out, host, e0.elapsed_time(e1)


def first_audio(model, mel, c, known, dev):
    T = mel.shape[2]
    spec = model._upsample_spec()
    first = c + (model.pad + 1 if known else 21)
    with model.stream(1, T if known else None, seed=1000) as s:
        out, host, devms = _timed(lambda: s.push(mel[:, :, :first]), dev)
    assert out.shape[1] == stream_plan(spec, first, False, T if known else None)[1] == c * model.hop_length
    return host, devms


def total(model, mel, c, known, dev):
    T = mel.shape[2]
    spec = model._upsample_spec()

    def run():
        n, launches, steps = 0, 0, 0
        with model.stream(1, T if known else None, seed=1000) as s:
            for f in range(0, T, c):
                n += s.push(mel[:, :, f:f + c]).shape[1]
                now = stream_plan(spec, min(T, f + c), False, T if known else None)[0]
                launches += now > steps
                steps = now
            n += s.finish().shape[1]
        return n, launches + 1
    (n, launches), host, devms = _timed(run, dev)
    assert n == (T - 1) * model.hop_length
    return host, devms, launches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunks", type=int, nargs="+", default=[4, 8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=401)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_latency.py times the GPU path: no GPU visible")
    dev = torch.device("cuda", 0)
    d = syn.DEFAULT_MOL
    model = WaveRNN(**d.ctor_kwargs()).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, 0).items()})
    model.eval()
    mel = torch.from_numpy(syn.make_mel(d.feat_dims, args.frames, seed=1))[None].to(dev)
    med = statistics.median

    def one_shot():
        return model.generate(mel, None, False, 11000, 550, False, seed=1000, verbose=False)
    one_shot()
    runs = [_timed(one_shot, dev)[1:] for _ in range(args.reps)]
    base_host, base_dev = med(r[0] for r in runs), med(r[1] for r in runs)
    print(json.dumps({"what": "one-shot generate()", "frames": args.frames, "host_ms": round(base_host, 3),
                      "device_ms": round(base_dev, 3), "loop_kernel_ms": round(model.loop_handle().elapsed_ms(), 3),
                      "reps": args.reps}), flush=True)
    for known in (True, False):
        for c in args.chunks:
            first_audio(model, mel, c, known, dev)
            fa = [first_audio(model, mel, c, known, dev) for _ in range(args.reps)]
            total(model, mel, c, known, dev)
            tt = [total(model, mel, c, known, dev) for _ in range(args.reps)]
            host = med(t[0] for t in tt)
            launches = tt[0][2]
            print(json.dumps({
                "what": "streamed", "chunk_frames": c, "total_frames_known": known,
                "first_audio_frames_needed": c + (model.pad + 1 if known else 21),
                "first_audio_host_ms": round(med(f[0] for f in fa), 3),
                "first_audio_host_ms_min": round(min(f[0] for f in fa), 3),
                "first_audio_device_ms": round(med(f[1] for f in fa), 3),
                "total_host_ms": round(host, 3), "total_device_ms": round(med(t[1] for t in tt), 3),
                "launches": launches, "one_shot_host_ms": round(base_host, 3),
                "per_relaunch_overhead_ms": round((host - base_host) / launches, 4), "reps": args.reps}), flush=True)
    model.train()


if __name__ == "__main__":
    main()
