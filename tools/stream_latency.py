#!/usr/bin/env python3
"""First-audio latency and total time of streamed synthesis on the headline model (MoL rnn/fc 512,
401 frames = 5 s), against the one-shot generate() of the same process.

    python tools/stream_latency.py [--chunks 4 8 32] [--reps 5] [--frames 401] [--independent 8]

Per chunk size c (mel frames per push), total_frames announced (no 21-frame hold-back) and not:
  (a) first audio: the push that brings the session to the first frame count at which c frames of
      audio are final (c + lookahead frames when the total is known, c + 21 when it is not) — host
      time from entering push() to the float64 samples being in host memory (push synchronises and
      copies), and the device time between HIP events recorded around it;
  (b) total: all 401 frames pushed c at a time, every push's audio copied to the host — host time
      from the first push to the last sample on the host, device time likewise, and the number of
      pushes that launched the persistent kernel.
--independent N (default 8; 0 skips it) adds the server case, per chunk size c: N single-utterance
Philox sessions with lengths spread from 201 to 401 frames, session i opening 4·i ticks after
session 0, every open session pushing c frames per tick — run (a) with one wrnn_stream_push per
session per tick (one persistent launch each, one XCD busy) and (b) with one group push per tick
(wrnn_stream_push_group: one launch, a row per XCD).  Reported: wall time per tick (call to device
idle), aggregate samples/s and × real time, persistent launches, and the host time of a tick's
asynchronous call(s) — the per-member conditioning, the launch and the post being queued, an upper
bound of the host time before the persistent launch.  (a) and (b) must produce identical audio.
Beside it, on N mels of 401 frames from tick 0: a lock-step U = N session (the windowed kernel)
against a group of N U = 1 sessions (the grouped kernel), wall µs per step of a row.
Every shape is warmed by one untimed session first (code objects, rocBLAS algorithm choice); each
figure is the median of --reps fresh sessions (a session allocates its workspaces in its first
pushes: that is part of what a caller waits for, and it is included).  One JSON line per row.

    python tools/stream_latency.py --wide 8 16 32 64 128 [--legs a b] [--reps 3] [--raw]

--wide N (up to 128; nothing else runs): the server with more than eight open sessions.  N
single-utterance Philox sessions of 401 frames, all open from tick 0, every session pushing 8
frames per tick (99.8 ms of audio at hop 275) — leg (a) with ceil(N / 8) narrow group pushes per
tick, one after the other (entry points every revision with group pushes has, so the same leg
runs on an older library as the baseline), leg (b) with ONE wide group push per tick
(stream(wide=True): the many-row kernel, 16 rows per XCD).  Per leg: wall time per tick (call to
device idle; median, 90th percentile, maximum over the ticks of a run, each the median over the
runs), the device time between stream events recorded around the tick's call(s), for leg (b) its
split into loop (wrnn_elapsed_ms: interpolation, draws, resets and persistent launches of the
push) and conditioning (the rest: per-member mel window, MelResNet, frame-term GEMMs, post),
persistent launches per tick, × real time, and whether the N sessions are sustained: a tick
carries 8 · 275 / 22 050 s of audio, so they are when the tick's wall time stays below that.
--raw adds leg (r) in the same invocation: leg (b) on the RAW 9-bit rnn / fc 512 model (reference
geometry, Philox, mu-law on) — the many-row kernel's softmax head, which adds the f2 and logits hops
to every step — and the ratio of its loop share to leg (b)'s of the same run.
--audio adds leg (p) in the same invocation: leg (b) fed PCM instead of mel — every session pushes
8 · 275 samples per tick, the tick stages every session's PCM tail, computes the frames that became
final in ONE front-end launch (wrnn_melspec_windows) and hands them to the same wide group push —
and the difference of its tick to leg (b)'s: the front end's cost per tick.

    python tools/stream_latency.py --rows rnn256 dense896 raw512 [--chunks 4 8 32] [--reps 3] [--frames 101]
                                   [--out profiles/stream_rows_latency.jsonl]

--rows MODEL... (nothing else runs): sessions on the multi-row kernel (stream(rows=True)) for models no
XCD-resident session kernel covers — rnn256 (MoL rnn / fc 256), dense896 (MoL rnn 896, unpruned),
raw512 (RAW 9 bits), raw10 (RAW 10 bits), mol1024 (MoL rnn 1024 / fc 768), all at the reference
geometry.  Per model and chunk size c, total_frames announced: first audio (as above), the whole
utterance pushed c frames at a time, µs per step (host time over frames · hop) and whether that keeps
up with real time (1e6 / sample_rate µs per step), beside the one-shot generate() of the same utterance
in the same run — on the path it picks by default and on the multi-row kernel (WRNN_PATH=rows).  One
JSON line per leg, printed and appended to --out."""
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


def first_audio(model, mel, c, known, dev, **kw):
    T = mel.shape[2]
    spec = model._upsample_spec()
    first = c + (model.pad + 1 if known else 21)
    with model.stream(1, T if known else None, seed=1000, **kw) as s:
        out, host, devms = _timed(lambda: s.push(mel[:, :, :first]), dev)
    assert out.shape[1] == stream_plan(spec, first, False, T if known else None)[1] == c * model.hop_length
    return host, devms


def total(model, mel, c, known, dev, **kw):
    T = mel.shape[2]
    spec = model._upsample_spec()

    def run():
        n, launches, steps = 0, 0, 0
        with model.stream(1, T if known else None, seed=1000, **kw) as s:
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


def _ticks(model, mels, starts, c, grouped, dev, n_streams=1):
    """Sessions over `mels` ([U][feat][T_i] each), session i opening at tick starts[i], c frames per
    tick and an empty final push after the last: per tick one push per open session, or one group
    push.  → (audio per session, wall ms per tick, host ms per tick in the asynchronous calls,
    persistent launches, wall ms in all)."""
    spec, loop = model._upsample_spec(), model.loop_handle()
    N = len(mels)
    sess, f, out = [None] * N, [0] * N, [[] for _ in range(N)]
    walls, hosts, launches = [], [], 0
    torch.cuda.synchronize(dev)
    t_begin = time.perf_counter()
    try:
        tick = 0
        while any(s is None or not s._session.finished for s in sess):
            for i in range(N):   # opening a session synchronises: outside the tick's clock
                if sess[i] is None and tick >= starts[i]:
                    sess[i] = model.stream(n_streams, mels[i].shape[2], seed=1000, row_offset=i * n_streams)
            live = [i for i in range(N) if sess[i] is not None and not sess[i]._session.finished]
            pushes, ran = [], 0
            for i in live:
                T = mels[i].shape[2]
                n = min(c, T - f[i])
                before = stream_plan(spec, f[i], False, T)[0]
                ran += stream_plan(spec, f[i] + n, n == 0, T)[0] > before
                pushes.append((sess[i]._session, mels[i][:, :, f[i]:f[i] + n].contiguous() if n else None, n == 0))
                f[i] += n
            launches += (ran > 0) if grouped else ran
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if grouped:
                got = loop.push_streams(pushes, check=False) if pushes else []
            else:
                got = [s.push(mel, final=final, check=False) for s, mel, final in pushes]
            t1 = time.perf_counter()
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            if pushes:
                walls.append((t2 - t0) * 1e3)
                hosts.append((t1 - t0) * 1e3)
            for i, w in zip(live, got):
                out[i].append(w)
            tick += 1
        loop.check()
    finally:
        for s in sess:
            if s is not None:
                s.close()
    total_ms = (time.perf_counter() - t_begin) * 1e3
    return [torch.cat(o, 1).cpu().numpy() for o in out], walls, hosts, launches, total_ms


def independent(model, N, c, reps, dev, d):
    """The server case and the lock-step comparison (module docstring), one JSON line each."""
    med = statistics.median
    lengths = [401 if N == 1 else 201 + round(i * 200 / (N - 1)) for i in range(N)]
    mels = [torch.from_numpy(syn.make_mel(d.feat_dims, T, seed=10 + i))[None].to(dev) for i, T in enumerate(lengths)]
    starts = [4 * i for i in range(N)]
    samples = sum((T - 1) * d.hop_length for T in lengths)
    rows = {}
    for grouped in (False, True):
        _ticks(model, mels, starts, c, grouped, dev)
        runs = [_ticks(model, mels, starts, c, grouped, dev) for _ in range(reps)]
        rows[grouped] = runs
        if grouped:
            for a, b in zip(rows[False][0][0], runs[0][0]):
                assert np.array_equal(a, b), "group pushes and single pushes produced different audio"
        busy = med(sum(r[1]) for r in runs)   # the ticks alone: opening a session synchronises and is left out
        print(json.dumps({
            "what": "independent sessions, " + ("one group push per tick" if grouped else "one push per session per tick"),
            "sessions": N, "frames": lengths, "chunk_frames": c, "ticks": len(runs[0][1]),
            "tick_wall_ms_median": round(med(med(r[1]) for r in runs), 3),
            "tick_wall_ms_max": round(med(max(r[1]) for r in runs), 3),
            "tick_host_queue_ms_median": round(med(med(r[2]) for r in runs), 3),
            "persistent_launches": runs[0][3], "busy_ms": round(busy, 2),
            "samples_per_s": round(samples / busy * 1e3), "x_real_time": round(samples / d.sample_rate / busy * 1e3, 2),
            "reps": reps}), flush=True)
    # lock step against a group, the same N mels of 401 frames from tick 0
    T = 401
    same = [torch.from_numpy(syn.make_mel(d.feat_dims, T, seed=10 + i))[None].to(dev) for i in range(N)]
    steps = T * d.hop_length
    cases = (("lock-step U = %d session (windowed kernel)" % N, [torch.cat(same, 0)], False, N),
             ("group of %d U = 1 sessions (grouped kernel)" % N, same, True, 1))
    audio = {}
    for what, ms, grouped, U in cases:
        _ticks(model, ms, [0] * len(ms), c, grouped, dev, n_streams=U)
        runs = [_ticks(model, ms, [0] * len(ms), c, grouped, dev, n_streams=U) for _ in range(reps)]
        audio[grouped] = np.concatenate(runs[0][0], 0)
        busy = [sum(r[1]) for r in runs]
        print(json.dumps({
            "what": what, "rows": N, "frames": T, "chunk_frames": c, "persistent_launches": runs[0][3],
            "busy_ms": round(med(busy), 2), "busy_ms_min_max": [round(min(busy), 2), round(max(busy), 2)],
            "wall_us_per_step": round(med(busy) * 1e3 / steps, 4),
            "tick_host_queue_ms_median": round(med(med(r[2]) for r in runs), 3),
            "x_real_time": round(N * (T - 1) * d.hop_length / d.sample_rate / med(busy) * 1e3, 2), "reps": reps}), flush=True)
    assert np.array_equal(audio[False], audio[True]), "the lock-step session and the group produced different audio"


def _wide_ticks(model, mels, c, wide, dev):
    """N U = 1 sessions over `mels`, all from tick 0, c frames per tick and an empty final push:
    one wide group push per tick, or ceil(N / 8) narrow ones.  → (audio [N][samples], per tick:
    wall ms, device ms, loop ms (wide; else None), persistent launches)."""
    spec, loop = model._upsample_spec(), model.loop_handle()
    N, T = len(mels), mels[0].shape[2]
    kw = {"wide": True} if wide else {}
    sess = [model.stream(1, T, seed=1000, row_offset=i, **kw) for i in range(N)]
    out, ticks = [[] for _ in range(N)], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        f = 0
        while not sess[0]._session.finished:
            n = min(c, T - f)
            ran = stream_plan(spec, f + n, n == 0, T)[0] > stream_plan(spec, f, False, T)[0]
            pushes = [(s._session, m[:, :, f:f + n].contiguous() if n else None, n == 0) for s, m in zip(sess, mels)]
            groups = [pushes] if wide else [pushes[i:i + 8] for i in range(0, N, 8)]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            got = [w for g in groups for w in loop.push_streams(g, check=False)]
            e1.record()
            torch.cuda.synchronize(dev)
            wall = (time.perf_counter() - t0) * 1e3
            ticks.append((wall, e0.elapsed_time(e1), loop.elapsed_ms() if wide and ran else None, len(groups) * ran))
            for i, w in enumerate(got):
                out[i].append(w)
            f += n
        loop.check()
    finally:
        for s in sess:
            s.close()
    return np.concatenate([torch.cat(o, 1).cpu().numpy() for o in out], 0), ticks


def _wide_audio_ticks(model, pcms, c, dev):
    """Leg (p): N wide U = 1 sessions fed PCM (`pcms` [1][samples] each), c·hop samples per tick, then
    the flush (the remaining frames, and the empty final push).  → what _wide_ticks returns, the
    third entry of a tick being the host ms spent staging the PCM and queueing the front end."""
    loop = model.loop_handle()
    N, NS, hop = len(pcms), pcms[0].shape[1], model.hop_length
    sess = [model.stream(1, total_samples=NS, seed=1000, row_offset=i, wide=True) for i in range(N)]
    feeds = [s._audio_feed() for s in sess]
    front = feeds[0].front
    out, ticks = [[] for _ in range(N)], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        f = 0
        while not sess[0]._session.finished:
            n = min(c * hop, NS - f)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            staged = [fd.stage(p[:, f:f + n] if n else None, final=n == 0) for fd, p in zip(feeds, pcms)]
            jobs = [j for _, js, _ in staged for j in js]
            mels = front.windows(jobs) if jobs else []
            t1 = time.perf_counter()
            pushes = [(s._session, mels[i][None] if jobs else None, False) for i, s in enumerate(sess)]
            got = loop.push_streams(pushes, check=False)
            if n == 0:
                got = [torch.cat([a, b], 1) for a, b in
                       zip(got, loop.push_streams([(s._session, None, True) for s in sess], check=False))]
            e1.record()
            torch.cuda.synchronize(dev)
            wall = (time.perf_counter() - t0) * 1e3
            for fd, (state, _, _) in zip(feeds, staged):
                fd.commit(state)
            ticks.append((wall, e0.elapsed_time(e1), (t1 - t0) * 1e3, int(bool(jobs))))
            for i, w in enumerate(got):
                out[i].append(w)
            f += n
        loop.check()
    finally:
        for s in sess:
            s.close()
    return np.concatenate([torch.cat(o, 1).cpu().numpy() for o in out], 0), ticks


def wide_case(model, N, legs, reps, dev, d, raw_model=None, pcm_leg=False):
    """--wide N (module docstring): one JSON line per leg (raw_model: leg r after the others)."""
    med = statistics.median
    T, c = 401, 8
    mels = [torch.from_numpy(syn.make_mel(d.feat_dims, T, seed=10 + i))[None].to(dev) for i in range(N)]
    audio_ms = c * d.hop_length / d.sample_rate * 1e3
    audio, loop_ms = {}, {}
    pcms = [torch.from_numpy(0.1 * np.random.default_rng(10 + i).standard_normal((1, (T - 1) * d.hop_length))
                             .astype(np.float32)).to(dev) for i in range(N)] if pcm_leg else None
    wall = {}
    for leg in list(legs) + (["r"] if raw_model is not None else []) + (["p"] if pcm_leg else []):
        wide = leg in ("b", "r", "p")
        mdl = raw_model if leg == "r" else model
        if leg == "p":
            _wide_audio_ticks(mdl, pcms, c, dev)
            runs = [_wide_audio_ticks(mdl, pcms, c, dev) for _ in range(reps)]
        else:
            _wide_ticks(mdl, mels, c, wide, dev)
            runs = [_wide_ticks(mdl, mels, c, wide, dev) for _ in range(reps)]
        audio[leg] = runs[0][0]
        full = [[t for t in r[1] if t[3]][1:-1] for r in runs]   # ticks of 8 frames with a launch; not the first, not the flush

        def stat(k, fn):
            return round(med(fn([t[k] for t in ticks]) for ticks in full), 3)

        def p90(v):
            return sorted(v)[int(0.9 * (len(v) - 1))]

        row = {"what": "wide: " + ("fed PCM: one front-end launch, then one wide group push per tick" if leg == "p" else
                                   "RAW 9-bit, one wide group push per tick" if leg == "r" else
                                   "one wide group push per tick" if wide else "ceil(N / 8) narrow group pushes per tick"),
               "leg": leg, "sessions": N, "frames": T, "chunk_frames": c, "audio_ms_per_tick": round(audio_ms, 2),
               "ticks_measured": len(full[0]), "tick_wall_ms_median": stat(0, med), "tick_wall_ms_p90": stat(0, p90),
               "tick_wall_ms_max": stat(0, max), "tick_device_ms_median": stat(1, med),
               "launches_per_tick": full[0][0][3], "reps": reps}
        wall[leg] = row["tick_wall_ms_median"]
        if leg == "p":
            row["tick_front_end_host_ms_median"] = stat(2, med)
            if "b" in wall:
                row["tick_wall_ms_over_mel_fed"] = round(wall["p"] - wall["b"], 3)
        elif wide:
            row["tick_loop_ms_median"] = loop_ms[leg] = stat(2, med)
            row["tick_conditioning_ms_median"] = round(med(med(t[1] - t[2] for t in ticks) for ticks in full), 3)
        row["x_real_time"] = round(N * audio_ms / row["tick_wall_ms_median"], 1)
        row["sustained"] = bool(row["tick_wall_ms_p90"] < audio_ms)
        print(json.dumps(row), flush=True)
    if "b" in loop_ms and "r" in loop_ms:
        print(json.dumps({"what": "wide: RAW loop share against the MoL wide leg of the same run", "sessions": N,
                          "raw_over_mol_loop": round(loop_ms["r"] / loop_ms["b"], 3)}), flush=True)
    if "a" in audio and "b" in audio:
        print(json.dumps({"what": "wide: leg (b) against leg (a), the same sessions on the two kernels", "sessions": N,
                          "max_abs_diff": float(np.abs(audio["a"] - audio["b"]).max())}), flush=True)


ROWS_MODELS = {
    "rnn256": syn.FatchordDims(rnn_dims=256, fc_dims=256),
    "dense896": syn.FatchordDims(rnn_dims=896),
    "mol1024": syn.FatchordDims(rnn_dims=1024, fc_dims=768),
    "raw512": syn.DEFAULT_RAW,
    "raw10": syn.FatchordDims(bits=10, mode="RAW"),
}


def rows_case(name, chunks, reps, frames, dev, out_path):
    """--rows MODEL (module docstring): one JSON line per chunk size, after the one-shot lines."""
    med = statistics.median
    d = ROWS_MODELS[name]
    model = WaveRNN(**d.ctor_kwargs()).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, 0).items()})
    model.eval()
    mel = torch.from_numpy(syn.make_mel(d.feat_dims, frames, seed=1))[None].to(dev)
    steps = frames * d.hop_length
    real_time_us = 1e6 / d.sample_rate

    def emit(row):
        row = dict({"model": name, "mode": d.mode, "rnn_dims": d.rnn_dims, "fc_dims": d.fc_dims, "bits": d.bits,
                    "frames": frames, "steps": steps}, **row)
        line = json.dumps(row)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(line + "\n")

    def one_shot():
        return model.generate(mel, None, False, 11000, 550, True, seed=1000, verbose=False)
    base = {}
    for path_env in (None, "rows"):
        if path_env:
            os.environ["WRNN_PATH"] = path_env
        try:
            one_shot()
            runs = [_timed(one_shot, dev)[1:] for _ in range(reps)]
            path = model.loop_handle().info["last_path"]
        finally:
            os.environ.pop("WRNN_PATH", None)
        host = med(r[0] for r in runs)
        base[path_env] = host
        emit({"what": "one-shot generate()" + (" on the multi-row kernel (WRNN_PATH=rows)" if path_env else ""),
              "last_path": path, "host_ms": round(host, 3), "device_ms": round(med(r[1] for r in runs), 3),
              "us_per_step": round(host * 1e3 / steps, 3), "reps": reps})
    for c in chunks:
        first_audio(model, mel, c, True, dev, rows=True)
        fa = [first_audio(model, mel, c, True, dev, rows=True) for _ in range(reps)]
        total(model, mel, c, True, dev, rows=True)
        tt = [total(model, mel, c, True, dev, rows=True) for _ in range(reps)]
        host = med(t[0] for t in tt)
        us = host * 1e3 / steps
        emit({"what": "rows session", "last_path": model.loop_handle().info["last_path"], "chunk_frames": c,
              "total_frames_known": True, "first_audio_frames_needed": c + model.pad + 1,
              "first_audio_host_ms": round(med(f[0] for f in fa), 3), "first_audio_device_ms": round(med(f[1] for f in fa), 3),
              "total_host_ms": round(host, 3), "total_device_ms": round(med(t[1] for t in tt), 3), "launches": tt[0][2],
              "us_per_step": round(us, 3), "real_time_us_per_step": round(real_time_us, 2),
              "x_real_time": round(real_time_us / us, 3), "real_time": bool(us < real_time_us),
              "one_shot_host_ms": round(base[None], 3), "one_shot_rows_host_ms": round(base["rows"], 3), "reps": reps})
    model.train()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunks", type=int, nargs="+", default=[4, 8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=None, help="frames of the utterance (default 401; --rows: 101)")
    ap.add_argument("--independent", type=int, default=8, metavar="N",
                    help="sessions of the server case (1..8; 0: skip it)")
    ap.add_argument("--only-independent", action="store_true", help="skip the single-session latency rows")
    ap.add_argument("--wide", type=int, nargs="+", default=[], metavar="N",
                    help="only the wide-group case, for each N (1..128) sessions")
    ap.add_argument("--legs", nargs="+", choices=["a", "b"], default=["a", "b"],
                    help="--wide: a = narrow group pushes (runs on older libraries too), b = one wide group push")
    ap.add_argument("--raw", action="store_true",
                    help="--wide: add leg r, the wide leg on the RAW 9-bit rnn / fc 512 model")
    ap.add_argument("--audio", action="store_true",
                    help="--wide: add leg p, the wide leg fed PCM through the mel front end (push_audio's path)")
    ap.add_argument("--rows", nargs="+", choices=sorted(ROWS_MODELS), default=[], metavar="MODEL",
                    help="only the rows-session case, for each model: " + ", ".join(sorted(ROWS_MODELS)))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "stream_rows_latency.jsonl"),
                    help="--rows: the file the JSON lines are appended to")
    args = ap.parse_args()
    if any(not 1 <= n <= 128 for n in args.wide):
        ap.error("--wide takes 1..128 sessions (a wide group has at most 128 rows)")
    if not 0 <= args.independent <= 8:
        ap.error("--independent takes 0..8 sessions (a group has at most 8 rows)")
    if not torch.cuda.is_available():
        sys.exit("stream_latency.py times the GPU path: no GPU visible")
    dev = torch.device("cuda", 0)
    if args.rows:
        for name in args.rows:
            rows_case(name, args.chunks, args.reps, args.frames or 101, dev, args.out)
        return
    args.frames = args.frames or 401
    d = syn.DEFAULT_MOL
    model = WaveRNN(**d.ctor_kwargs()).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(d, 0).items()})
    model.eval()
    if args.wide:
        raw_model = None
        if args.raw:
            dr = syn.DEFAULT_RAW
            raw_model = WaveRNN(**dr.ctor_kwargs()).to(dev)
            raw_model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(dr, 0).items()})
            raw_model.eval()
        for n in args.wide:
            wide_case(model, n, args.legs, args.reps, dev, d, raw_model, args.audio)
        model.train()
        return
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
    for known in (() if args.only_independent else (True, False)):
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
    if args.independent:
        for c in args.chunks:
            independent(model, args.independent, c, args.reps, dev, d)
    model.train()


if __name__ == "__main__":
    main()
