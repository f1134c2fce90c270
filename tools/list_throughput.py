#!/usr/bin/env python3
"""Throughput of a list of utterances of unequal length (a TTS batch) on the headline model (MoL
rnn/fc 512), four ways in one process:

    python tools/list_throughput.py [--reps 3] [--utterances 24] [--ways abcd] [--sparse | --raw] [--out FILE]

  (a) one generate() per utterance, one after the other;
  (b) generate_many(list): every row runs for the longest member's steps, conditioning at sample rate;
  (c) generate_list(list): the eight XCDs as lanes, each a queue of utterances (wrnn_generate_list);
  (d) generate_list(list, wide=True): up to 128 many-row slots, each a queue (wrnn_generate_list_wide).
The list: `--utterances` (default 24) mels of 101 … 401 frames, lengths and contents from fixed seeds.
Beside it, eight equal utterances of 401 frames through (b) and (c): the same eight rows, one per
XCD, 401·hop steps each — what the piece walk costs inside the step loop, if anything.

Per row: wall ms of the call (host clock, from the call to the float64 waveforms on the host; the
median, min and max of --reps calls after one untimed warm-up of the same shapes, the three ways
alternating inside every repeat), samples/s and × real time from the median, the device ms between
the loop's timing events (frame terms + per-round interpolation + persistent launches; wall − loop
is MelResNet, host work and the float64 post), the persistent launches per call (restated from the
launch loops of csrc/capi_loops.cpp, capi_lists.cpp and capi_stream.cpp for the WRNN_TERMS_MB in effect), and for (c) the lane occupancy
Σ L_i / (lanes · longest lane timeline) and the MelResNet (frames()) time of the list measured on
its own.  (a) and (c) must produce identical audio; (d) runs another kernel: its largest difference
from the first other way that ran is reported.  For (d): the slots, the slot occupancy Σ steps /
(slots · longest slot timeline), and the share of its loop time that is not steps — (loop − Σ launch
steps × 11.9 µs, the wide step of DESIGN §4.4c) / loop.  A way the device cannot hold (generate_many
builds a sample-rate [L_max][rows][208] tensor) is recorded as refused with the error's text; with
--many-block N, (b) runs the list N utterances at a time, one generate_many after the other.
--batched: the fold-batched leg instead (target 11 000, overlap 550, the reference's default way to
vocode), on the list of --utterances, or with --skewed on one 4 800-frame utterance plus 23 of 160:
  (f) generate_list(list, wide=True, batched=True): all folds on the many-row slots (wrnn_generate_list_folds);
  (m) generate_many(list, batched=True): all folds as rows, conditioning at sample rate;
  (s) one generate(batched=True) per utterance;
  (w) generate_list(list, wide=True): the unbatched wide list.
For (f): folds, slots, rounds, persistent launches, the slot occupancy folds / (rounds · slots) and the
loop µs per slot-step (loop / (rounds · 12 100)); for (w) the loop µs per step of the longest slot, the
same kernel's step in the same process.  (f), (m) and (s) share their Philox keys: the largest
difference of (f) from the first of (s), (m) that ran is reported (another instantiation: not zero).
--sparse: the 95 %-pruned rnn-896 model.  --raw: the RAW 9-bit rnn / fc 512 model (mu-law off), which
has ways (a) and (d) only.  One JSON line per row; --out appends them to a file as well."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavernn_amd import synthetic as syn                     # noqa: E402
from wavernn_amd.fatchord_version import WaveRNN             # noqa: E402
from wavernn_amd.loop import list_folds_plan, list_plan, list_wide_plan   # noqa: E402
from wavernn_amd.pruning import prune_state                  # noqa: E402

N_XCD = 32 * 160       # terms per row and step of the one-row XCD kernel (csrc/fatchord_xcd.h)
N_XCDS = 32 * 228      # … of the block-sparse rnn-896 one-row kernel (csrc/fatchord_xcds.h)
N_XCDM = 32 * 144      # … of the many-row kernel (csrc/fatchord_xcdm.h: kMRing)
WIDE_STEP_US = 11.9    # the measured step of a full wide launch


def _budget():
    return float(os.environ.get("WRNN_TERMS_MB", 8192.0)) * (1 << 20) / 4.0   # floats


def launches_single(L, rows, kxc, N=N_XCD):
    """generate_xcd_rows (capi_loops.cpp): rows <= 8, time chunks of floor(budget / (rows·(N + KXc)) − 1) steps."""
    lc = int(max(1.0, min(float(L), _budget() / (rows * (N + kxc)) - 1.0)))
    return -(-L // lc)


def launches_many(L, rows, kxc, N=N_XCD):
    """generate_many's route: up to 8 rows the one-row kernel, from 9 the many-row kernel (capi_loops.cpp:
    generate_xcdm, Philox draws: 11 more floats per row-step)."""
    if rows <= 8 or N != N_XCD:     # the sparse model has no many-row kernel: eight rows at a time
        return sum(launches_single(L, min(8, rows - b0), kxc, N) for b0 in range(0, rows, 8))
    lc = int(max(1.0, min(float(L), _budget() / (rows * (N_XCDM + kxc + 11)))))
    return -(-L // lc)


def launches_list(frames, lanes, hop, N=N_XCD):
    """wrnn_generate_list: rounds of C = floor(budget / (lanes·N) − 1) lane-steps."""
    longest = max(list_plan(frames, lanes)[2]) * hop
    C = int(max(1.0, min(float(longest), math.floor(_budget() / (lanes * N) - 1.0))))
    return -(-longest // C), longest


def _wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3


def run_case(model, d, mels, ways, reps, dev, what, emit, many_block=0):
    frames = [int(m.shape[2]) for m in mels]
    hop, U = d.hop_length, len(mels)
    kxc = d.feat_dims + d.res_out_dims + 4
    N = N_XCD if d.rnn_dims == 512 else N_XCDS
    samples = sum((T - 1) * hop for T in frames)
    steps = sum(T * hop for T in frames)
    loop = model.loop_handle()
    seed = 1000

    def single():
        out, ms = [], 0.0
        for i, m in enumerate(mels):
            out.append(model.generate(m, None, False, 11000, 550, False, seed=seed, row_offset=i, verbose=False))
            ms += loop.elapsed_ms()
        return out, ms

    def many():
        if not many_block or many_block >= U:
            out = model.generate_many(mels, None, False, 11000, 550, False, seed=seed)
            return out, loop.elapsed_ms()
        out, ms = [], 0.0
        for b0 in range(0, U, many_block):      # the list in blocks: one generate_many after the other
            out += model.generate_many(mels[b0:b0 + many_block], None, False, 11000, 550, False, seed=seed, row_offset=b0)
            ms += loop.elapsed_ms()
        return out, ms

    def lst():
        out = model.generate_list(mels, seed=seed)
        return out, loop.elapsed_ms()

    def wide():
        out = model.generate_list(mels, seed=seed, wide=True, mu_law=False)
        return out, loop.elapsed_ms()

    fns = {"a": ("one generate() per utterance", single), "b": ("generate_many", many), "c": ("generate_list", lst),
           "d": ("generate_list(wide=True)", wide)}
    audio, wall, dev_ms, path, refused = {}, {w: [] for w in ways}, {w: [] for w in ways}, {}, {}
    for rep in range(reps + 1):          # rep 0: the untimed warm-up of every shape
        for w in ways:
            if w in refused:
                continue
            try:
                (out, lms), ms = _wall(fns[w][1], dev)
            except (NotImplementedError, torch.cuda.OutOfMemoryError) as e:
                refused[w] = f"{type(e).__name__}: {e}".splitlines()[0]
                torch.cuda.empty_cache()
                continue
            path[w] = loop.info["last_path"]
            audio[w] = out
            if rep:
                wall[w].append(ms)
                dev_ms[w].append(lms)
    if "a" in audio and "c" in audio:
        assert all(np.array_equal(x, y) for x, y in zip(audio["a"], audio["c"])), "generate_list differs from the single calls"
    wide_delta = None
    other = next((w for w in ("a", "c", "b") if w in audio), None)
    if "d" in audio and other:
        wide_delta = max(float(np.abs(x - y).max()) for x, y in zip(audio["d"], audio[other]))
    mr = []
    for rep in range(reps + 1):
        _, ms = _wall(lambda: [model.frames(m) for m in mels], dev)
        if rep:
            mr.append(ms)
    lanes = min(8, U)
    L_max = max(frames) * hop
    for w in ways:
        row = {"what": what, "way": fns[w][0], "utterances": U, "frames_min_max": [min(frames), max(frames)],
               "loop_steps": steps, "reps": reps}
        if w in refused:
            row["refused"] = refused[w]
            emit(row)
            continue
        med = statistics.median(wall[w])
        row.update({"wall_ms": round(med, 2), "wall_ms_min_max": [round(min(wall[w]), 2), round(max(wall[w]), 2)],
                    "samples_per_s": round(samples / med * 1e3), "x_real_time": round(samples / d.sample_rate / med * 1e3, 2),
                    "loop_device_ms": round(statistics.median(dev_ms[w]), 2),
                    "loop_device_ms_min_max": [round(min(dev_ms[w]), 2), round(max(dev_ms[w]), 2)],
                    "outside_loop_ms": round(med - statistics.median(dev_ms[w]), 2), "last_path": path[w]})
        if w == "a":
            row["persistent_launches"] = sum(launches_single(T * hop, 1, kxc, N) for T in frames)
        elif w == "b":
            equal = len(set(frames)) == 1
            row["persistent_launches"] = launches_many(L_max, U, kxc, N) if U > 8 or equal else \
                sum(launches_single(L_max, min(8, U - b0), kxc, N) for b0 in range(0, U, 8))
            row["row_steps_run"] = U * L_max
            if many_block and many_block < U:
                row["measured_in_blocks_of"] = many_block
            row["loop_us_per_step_of_the_longest_row"] = round(statistics.median(dev_ms[w]) * 1e3 / L_max, 4)
        elif w == "d":
            raw = d.mode == "RAW"
            _, _, slot_frames, ls = list_wide_plan(frames, None, hop=hop, raw=raw)
            longest, loop_ms = max(slot_frames) * hop, statistics.median(dev_ms[w])
            assert sum(s for _, s, _ in ls) == longest
            row.update({"persistent_launches": len(ls), "slots": len(slot_frames), "longest_slot_steps": longest,
                        "slot_occupancy": round(steps / (len(slot_frames) * longest), 4),
                        "launch_steps_min_median_max": [min(s for _, s, _ in ls), int(statistics.median(s for _, s, _ in ls)),
                                                        max(s for _, s, _ in ls)],
                        "loop_us_per_step_of_the_longest_slot": round(loop_ms * 1e3 / longest, 4),
                        "not_steps_share_of_loop": round((loop_ms - longest * WIDE_STEP_US * 1e-3) / loop_ms, 4),
                        "max_abs_diff_from": {"way": fns[other][0], "value": wide_delta} if other else None,
                        "melresnet_ms": round(statistics.median(mr), 2)})
        else:
            n, longest = launches_list(frames, lanes, hop, N)
            row.update({"persistent_launches": n, "lanes": lanes, "longest_lane_steps": longest,
                        "lane_occupancy": round(steps / (lanes * longest), 4),
                        "loop_us_per_step_of_the_longest_lane": round(statistics.median(dev_ms[w]) * 1e3 / longest, 4),
                        "melresnet_ms": round(statistics.median(mr), 2)})
        emit(row)


def run_batched(model, d, mels, ways, reps, dev, what, emit, target=11000, overlap=550):
    """The fold-batched leg: ways f, m, s, w of the module docstring on one list."""
    frames = [int(m.shape[2]) for m in mels]
    hop, U = d.hop_length, len(mels)
    samples = sum((T - 1) * hop for T in frames)
    loop = model.loop_handle()
    seed = 1000
    raw = d.mode == "RAW"
    Lf = target + 2 * overlap
    folds, first, launches = list_folds_plan(frames, hop, target, overlap, raw=raw)
    F = sum(folds)
    slots = min(128, F)
    rounds = -(-F // slots)

    def folded():
        out = model.generate_list(mels, seed=seed, wide=True, batched=True, target=target, overlap=overlap, mu_law=False)
        return out, loop.elapsed_ms()

    def many():
        out = model.generate_many(mels, None, True, target, overlap, False, seed=seed)
        return out, loop.elapsed_ms()

    def single():
        out, ms = [], 0.0
        for i, m in enumerate(mels):
            out.append(model.generate(m, None, True, target, overlap, False, seed=seed, row_offset=first[i], verbose=False))
            ms += loop.elapsed_ms()
        return out, ms

    def wide():
        out = model.generate_list(mels, seed=seed, wide=True, mu_law=False)
        return out, loop.elapsed_ms()

    fns = {"f": ("generate_list(wide=True, batched=True)", folded), "m": ("generate_many(batched=True)", many),
           "s": ("one generate(batched=True) per utterance", single), "w": ("generate_list(wide=True)", wide)}
    audio, wall, dev_ms, refused = {}, {w: [] for w in ways}, {w: [] for w in ways}, {}
    for rep_i in range(reps + 1):        # rep 0: the untimed warm-up of every shape
        for w in ways:
            if w in refused:
                continue
            try:
                (out, lms), ms = _wall(fns[w][1], dev)
            except (NotImplementedError, torch.cuda.OutOfMemoryError) as e:
                refused[w] = f"{type(e).__name__}: {e}".splitlines()[0]
                torch.cuda.empty_cache()
                continue
            audio[w] = out
            if rep_i:
                wall[w].append(ms)
                dev_ms[w].append(lms)
    other = next((w for w in ("s", "m") if w in audio), None)
    delta, parted = None, []
    if "f" in audio and other:
        delta = max(float(np.abs(x - y).max()) for x, y in zip(audio["f"], audio[other]))
        # utterances where the two kernels' samplers took different branches (a near-tie in the mixture
        # selection): where they part, and whether the folded result is still its own list of one
        for i, (x, y) in enumerate(zip(audio["f"], audio[other])):
            far = np.flatnonzero(np.abs(x - y) > 1e-5)
            if far.size:
                alone = model.generate_list([mels[i]], seed=seed, row_offset=first[i], wide=True, batched=True, target=target,
                                            overlap=overlap, mu_law=False)[0]
                parted.append({"utterance": i, "frames": frames[i], "max_abs_diff": float(np.abs(x - y).max()),
                               "first_sample_beyond_1e-5": int(far[0]),
                               "max_abs_diff_before_it": float(np.abs(x - y)[:far[0]].max()) if far[0] else 0.0,
                               "equal_to_its_folded_list_of_one": bool(np.array_equal(alone, x))})
    for w in ways:
        row = {"what": what, "way": fns[w][0], "utterances": U, "frames_min_max": [min(frames), max(frames)],
               "target_overlap": [target, overlap], "folds": F, "reps": reps}
        if w in refused:
            row["refused"] = refused[w]
            emit(row)
            continue
        med, loop_ms = statistics.median(wall[w]), statistics.median(dev_ms[w])
        row.update({"wall_ms": round(med, 2), "wall_ms_min_max": [round(min(wall[w]), 2), round(max(wall[w]), 2)],
                    "samples_per_s": round(samples / med * 1e3), "x_real_time": round(samples / d.sample_rate / med * 1e3, 2),
                    "loop_device_ms": round(loop_ms, 2),
                    "loop_device_ms_min_max": [round(min(dev_ms[w]), 2), round(max(dev_ms[w]), 2)],
                    "outside_loop_ms": round(med - loop_ms, 2)})
        if w == "f":
            assert sum(s for _, s, _ in launches) == rounds * Lf
            row.update({"slots": slots, "rounds": rounds, "persistent_launches": len(launches),
                        "slot_occupancy": round(F / (rounds * slots), 4), "slot_steps": rounds * Lf,
                        "loop_us_per_slot_step": round(loop_ms * 1e3 / (rounds * Lf), 4),
                        "max_abs_diff_from": {"way": fns[other][0], "value": delta} if other else None,
                        "utterances_beyond_1e-5": parted})
        elif w == "w":
            _, _, slot_frames, ls = list_wide_plan(frames, None, hop=hop, raw=raw)
            longest = max(slot_frames) * hop
            row.update({"slots": len(slot_frames), "persistent_launches": len(ls), "longest_slot_steps": longest,
                        "slot_occupancy": round(sum(T * hop for T in frames) / (len(slot_frames) * longest), 4),
                        "loop_us_per_step_of_the_longest_slot": round(loop_ms * 1e3 / longest, 4)})
        elif w == "m":
            row["row_steps_run"] = F * Lf
        emit(row)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--utterances", type=int, default=24)
    ap.add_argument("--sparse", action="store_true", help="the 95 %%-pruned rnn-896 model")
    ap.add_argument("--raw", action="store_true", help="the RAW 9-bit rnn / fc 512 model: ways (a) and (d)")
    ap.add_argument("--ways", default=None, help="the ways to run, e.g. bcd (default abcd; --raw: ad; --sparse: abc)")
    ap.add_argument("--many-block", type=int, default=0, help="(b) in blocks of this many utterances")
    ap.add_argument("--skip-equal", action="store_true", help="leave out the eight equal utterances")
    ap.add_argument("--skip-single", action="store_true", help="leave out (a), the slowest way")
    ap.add_argument("--batched", action="store_true", help="the fold-batched leg (ways fmsw; target 11000, overlap 550)")
    ap.add_argument("--skewed", action="store_true", help="--batched: one 4800-frame utterance plus 23 of 160 frames")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("list_throughput.py times the GPU path: no GPU visible")
    dev = torch.device("cuda", 0)
    d = syn.SPARSE896_MOL if args.sparse else syn.DEFAULT_RAW if args.raw else syn.DEFAULT_MOL
    state = syn.make_fatchord_state(d, 0)
    if args.sparse:
        state = prune_state(state, 0.95)
    model = WaveRNN(**d.ctor_kwargs()).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    model.eval()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    U = args.utterances
    lengths = [401 if U == 1 else 101 + round(i * 300 / (U - 1)) for i in range(U)]
    np.random.default_rng(24).shuffle(lengths)       # arrival order, not sorted
    mixed = [torch.from_numpy(syn.make_mel(d.feat_dims, T, seed=10 + i))[None].to(dev) for i, T in enumerate(lengths)]
    if args.batched:
        ways = tuple(args.ways) if args.ways else ("f", "m", "s", "w")
        if args.skewed:
            sk = [4800] + [160] * 23
            mels = [torch.from_numpy(syn.make_mel(d.feat_dims, T, seed=300 + i))[None].to(dev) for i, T in enumerate(sk)]
            run_batched(model, d, mels, ways, args.reps, dev, "skewed list, one of 4800 frames and 23 of 160", emit)
        else:
            run_batched(model, d, mixed, ways, args.reps, dev, f"mixed list, {min(lengths)}..{max(lengths)} frames", emit)
        model.train()
        return
    ways = tuple(args.ways) if args.ways else ("a", "d") if args.raw else ("a", "b", "c") if args.sparse else ("a", "b", "c", "d")
    if args.skip_single:
        ways = tuple(w for w in ways if w != "a")
    tag = ", sparse rnn 896" if args.sparse else ", RAW 9-bit" if args.raw else ""
    run_case(model, d, mixed, ways, args.reps, dev, "mixed list, 101..401 frames" + tag, emit, args.many_block)
    if args.raw or args.skip_equal:
        model.train()
        return
    equal = [torch.from_numpy(syn.make_mel(d.feat_dims, 401, seed=100 + i))[None].to(dev) for i in range(8)]
    run_case(model, d, equal, ("b", "c"), args.reps, dev, "eight equal utterances of 401 frames" + (", sparse rnn 896" if args.sparse else ""), emit)
    model.train()


if __name__ == "__main__":
    main()
