#!/usr/bin/env python3
"""Cost of the mel front end (csrc/melspec.hip) at the two shapes that matter, beside the float32
host path it replaces.

    python tools/melspec_bench.py [--reps 50] [--kernel-only] [--out profiles/melspec_frontend.jsonl]

Shapes: one 5 s utterance (110 000 samples, 401 frames, wrnn_melspec) and one wide tick (128 signals ×
8 frames in one wrnn_melspec_windows launch, each from a resident tail).  Per shape: the device
time between events around one launch (median of --reps, after a warm launch; it includes the job
list's host-to-device copy) and the host time of the call; then the float32 host path
(dsp.melspectrogram(device='cpu'), scipy.fft with 16 workers) plus the copy of its result to the
GPU, wall time to completion.  --kernel-only runs just the launches, for a rocprofv3 --kernel-trace
--stats run of its own (the kernel is `melspec_kernel`).  One JSON line per row, printed and
appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavernn_amd import dsp                                  # noqa: E402
from wavernn_amd.melspec import MelSpec                      # noqa: E402


def _events(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    dev_ms, host_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    return statistics.median(dev_ms), statistics.median(host_ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("melspec_bench.py times the GPU path: no GPU visible")
    dev = torch.device("cuda", 0)
    p = dsp.melspec_params(None)
    front = MelSpec.get(p, dev)
    hop = p["hop_length"]
    g = np.random.default_rng(0)
    utt = (0.1 * g.standard_normal(400 * hop)).astype(np.float32)
    utt_gpu = torch.from_numpy(utt).to(dev)
    # a wide tick: session i has frames [t0, t0 + 8) final, its tail resident from keep_from
    t0, nt = 40, 8
    s0 = t0 * hop - 551
    ns = (t0 + nt - 1) * hop + 550 - s0
    tails = [(0.1 * g.standard_normal(ns)).astype(np.float32) for _ in range(128)]
    tails_gpu = [torch.from_numpy(t).to(dev) for t in tails]
    jobs = [(t, s0, None, t0, nt) for t in tails_gpu]
    shapes = (("one 5 s utterance, 401 frames", lambda: front.run([utt_gpu]), [utt], 401),
              ("wide tick, 128 signals x 8 frames", lambda: front.windows(jobs), tails, 1024))

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for what, launch, host_signals, frames in shapes:
        dev_ms, host_ms = _events(launch, args.reps, dev)
        emit({"what": "front-end launch: " + what, "frames": frames, "device_ms_median": round(dev_ms, 4),
              "host_call_ms_median": round(host_ms, 4), "reps": args.reps})
        if args.kernel_only:
            continue
        import scipy.fft

        def host_path():
            with scipy.fft.set_workers(16):
                if frames == 401:
                    mels = [dsp.melspectrogram(host_signals[0], p, device="cpu")]
                else:
                    # the same 8 frames per session: the host computes the tail's own frames
                    mels = [dsp.melspectrogram(s, p, device="cpu")[:, 2:2 + nt] for s in host_signals]
            out = torch.from_numpy(np.ascontiguousarray(np.stack(mels))).to(dev)
            torch.cuda.synchronize(dev)
            return out
        host_path()
        walls = []
        for _ in range(max(3, args.reps // 10)):
            t = time.perf_counter()
            host_path()
            walls.append((time.perf_counter() - t) * 1e3)
        emit({"what": "float32 host path + copy to the GPU: " + what, "frames": frames,
              "wall_ms_median": round(statistics.median(walls), 3), "workers": 16, "reps": len(walls)})


if __name__ == "__main__":
    main()
