#!/usr/bin/env python3
"""Text → audio throughput: Tacotron (decoder loop as one HIP launch, or eager torch) and the vocoder.

    python tools/tts_throughput.py [--n 1 24 128 512] [--steps 200] [--reps 3] [--out FILE]

For each N: N synthetic sentences of 20 … 120 ids (fixed seeds), seeded hparams-size weights, r = 2, a
stop threshold no frame reaches, so every sentence runs ceil(steps / 2) decoder steps. One process,
one GPU, one untimed warm-up of the same shapes, then --reps timed repeats (median reported); GPU
work is timed between device events, end-to-end rows by the host clock around a synchronised call.

  encoder   embedding, prenet, CBHG and encoder_proj, one call per sentence (torch-ROCm modules);
  hip       the decoder loop of all N sentences: ⌈N / 128⌉ persistent launches (wrnn_taco_run);
  torch     the eager decoder loop, one sentence after the other — what a caller of the PyTorch
            Tacotron runs; timed on the first min(N, --torch-sample) sentences (the loop does not
            depend on N) and reported per sentence-step;
  postnet   postnet CBHG and post_proj, one call per sentence.
  list      synthesize_list: generate_list → rescale → vocoder generate_list(wide=True);
  single    one Tacotron.generate(backend='torch') plus one vocoder generate() per sentence, timed on
            the first min(N, --single-sample) sentences and scaled to N.

µs per decoder step: `hip_us_per_step` is loop time / decoder steps of the launch (all rows advance
together; the session's set-up — buffers, padding copies — is inside; `hip_launch_only_*` times
wrnn_taco_run alone on sessions set up beforehand), `hip_us_per_sentence_step` divides that by N; `torch_us_per_sentence_step` is the eager
loop's. `decoder_share` is the hip decoder's share of the `list` wall time. One JSON line per N.

    python tools/tts_throughput.py --cbhg [--n ...] [--out profiles/tts_cbhg_throughput.json]

`--cbhg` times the CBHG legs both ways in the same run, same protocol: the encoders of the N sentences
(`[encode(x)]` under repeatable_modules against one `encode_list(cbhg='hip')`), their postnets on the
HIP decoder's mels (`[postprocess(m)]` against `postprocess_list(cbhg='hip')`) and `synthesize_list`
with `cbhg=None` and `cbhg='hip'` (host clock). `hip_min_call_ms` is a one-id `encode_list`: the
per-call floor (id check, table upload, weight repack of the whole encoder, 18 launches)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wavernn_amd import gen_tacotron as gt                   # noqa: E402
from wavernn_amd import synthetic as syn                     # noqa: E402
from wavernn_amd.fatchord_version import WaveRNN             # noqa: E402
from wavernn_amd.tacotron import MAX_ROWS, DecoderSession, Tacotron, repeatable_modules   # noqa: E402


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(fn, reps, timer):
    timer(fn)
    ts = [timer(fn)[0] for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def cbhg_rows(args, tts, voc, vd):
    """The --cbhg table: torch and hip legs of the encoder, the postnet and synthesize_list."""
    d = syn.DEFAULT_TACOTRON
    rows = []
    one_id = [syn.make_text_ids(1, d.num_chars, seed=0)]
    for N in args.n:
        rng = np.random.default_rng(1000 + N)
        xs = [syn.make_text_ids(int(t), d.num_chars, seed=i) for i, t in enumerate(rng.integers(20, 121, size=N))]
        note = lambda what: print(f"# n={N}: {what}", file=sys.stderr, flush=True)   # noqa: E731
        with torch.no_grad():
            note("encoder")
            with repeatable_modules():
                enc_t = median(lambda: [tts.encode(x) for x in xs], args.reps, device_ms)
            enc_h = median(lambda: tts.encode_list(xs, cbhg="hip"), args.reps, device_ms)
            floor = median(lambda: tts.encode_list(one_id, cbhg="hip"), args.reps, device_ms)
            coded = tts.encode_list(xs, cbhg="hip")
            order = sorted(range(N), key=lambda i: -coded[i][0].shape[1])
            mels = []
            for k in range(0, N, MAX_ROWS):
                idx = order[k:k + MAX_ROWS]
                s = DecoderSession(tts, [coded[i][0][0] for i in idx], [coded[i][1][0] for i in idx], args.steps)
                s.run(s.step_cap)
                mels += [m.transpose(0, 1).unsqueeze(0).contiguous() for m, _, _ in s.outputs()]
            note("postnet")
            with repeatable_modules():
                post_t = median(lambda: [tts.postprocess(m) for m in mels], args.reps, device_ms)
            post_h = median(lambda: tts.postprocess_list(mels, cbhg="hip"), args.reps, device_ms)
        row = {"n": N, "steps": args.steps, "reps": args.reps, "positions_encoder": int(sum(len(x) for x in xs)),
               "positions_postnet": int(sum(m.shape[2] for m in mels)),
               "encoder_torch_ms": round(enc_t[0], 3), "encoder_hip_ms": round(enc_h[0], 3),
               "encoder_hip_ms_min_max": [round(enc_h[1], 3), round(enc_h[2], 3)],
               "encoder_speedup": round(enc_t[0] / enc_h[0], 2),
               "postnet_torch_ms": round(post_t[0], 3), "postnet_hip_ms": round(post_h[0], 3),
               "postnet_hip_ms_min_max": [round(post_h[1], 3), round(post_h[2], 3)],
               "postnet_speedup": round(post_t[0] / post_h[0], 2), "hip_min_call_ms": round(floor[0], 3)}
        if not args.no_vocoder:
            note("synthesize_list")
            lst_t = median(lambda: gt.synthesize_list(tts, voc, xs, seed=1, steps=args.steps), args.reps, wall_ms)
            lst_h = median(lambda: gt.synthesize_list(tts, voc, xs, seed=1, steps=args.steps, cbhg="hip"), args.reps, wall_ms)
            row.update({"list_torch_ms": round(lst_t[0], 1), "list_hip_ms": round(lst_h[0], 1),
                        "list_hip_ms_min_max": [round(lst_h[1], 1), round(lst_h[2], 1)],
                        "list_speedup": round(lst_t[0] / lst_h[0], 2),
                        "encoder_share_torch": round(enc_t[0] / lst_t[0], 3), "postnet_share_torch": round(post_t[0] / lst_t[0], 3),
                        "encoder_share_hip": round(enc_h[0] / lst_h[0], 3), "postnet_share_hip": round(post_h[0] / lst_h[0], 3)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[1, 24, 128, 512])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-sample", type=int, default=8)
    ap.add_argument("--single-sample", type=int, default=4)
    ap.add_argument("--no-vocoder", action="store_true", help="skip the list / single rows")
    ap.add_argument("--cbhg", action="store_true", help="time the encoder, postnet and list legs through torch and through hip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    d = syn.DEFAULT_TACOTRON
    tts = Tacotron(**d.ctor_kwargs())
    tts.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in syn.make_tacotron_state(d, seed=0, scale=2.0).items()})
    tts = tts.to(dev).eval()
    tts.r = 2
    tts.stop_threshold.fill_(-1e30)
    vd = syn.DEFAULT_MOL
    voc = WaveRNN(**vd.ctor_kwargs()).to(dev)
    voc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in syn.make_fatchord_state(vd, 0).items()})
    voc.eval()
    n_dec = -(-args.steps // tts.r)
    rows = cbhg_rows(args, tts, voc, vd) if args.cbhg else []
    for N in ([] if args.cbhg else args.n):
        rng = np.random.default_rng(1000 + N)
        xs = [syn.make_text_ids(int(t), d.num_chars, seed=i) for i, t in enumerate(rng.integers(20, 121, size=N))]
        note = lambda what: print(f"# n={N}: {what}", file=sys.stderr, flush=True)   # noqa: E731
        note("encoder")
        with torch.no_grad():
            with repeatable_modules():       # as generate() / generate_list() run them
                enc_ms = median(lambda: [tts.encode(x) for x in xs], args.reps, device_ms)
            coded = [tts.encode(x) for x in xs]
            order = sorted(range(N), key=lambda i: -coded[i][0].shape[1])
            chunks = [order[k:k + MAX_ROWS] for k in range(0, N, MAX_ROWS)]

            def hip_loop():
                outs = []
                for idx in chunks:
                    s = DecoderSession(tts, [coded[i][0][0] for i in idx], [coded[i][1][0] for i in idx], args.steps)
                    s.run(s.step_cap)
                    outs.append(s)
                return outs
            note("decoder loops")
            hip_ms = median(hip_loop, args.reps, device_ms)

            def launches_only():        # the sessions set up beforehand: wrnn_taco_run alone
                total = 0.0
                for idx in chunks:
                    s = DecoderSession(tts, [coded[i][0][0] for i in idx], [coded[i][1][0] for i in idx], args.steps)
                    total += device_ms(lambda: s.run(s.step_cap))[0]
                return total
            launches_only()
            launch_ms = statistics.median(launches_only() for _ in range(args.reps))
            ns = min(N, args.torch_sample)
            torch_ms = median(lambda: [tts.decode_torch(*coded[i], args.steps) for i in range(ns)], args.reps, device_ms)
            note("postnet")
            mels = [m.transpose(0, 1).unsqueeze(0).contiguous() for s in hip_loop() for m, _, _ in s.outputs()]
            with repeatable_modules():
                post_ms = median(lambda: [tts.postprocess(m) for m in mels], args.reps, device_ms)
        row = {"n": N, "steps": args.steps, "r": tts.r, "decoder_steps": n_dec, "launches": len(chunks),
               "ids_min": int(min(len(x) for x in xs)), "ids_max": int(max(len(x) for x in xs)), "reps": args.reps,
               "encoder_ms": round(enc_ms[0], 3), "hip_decoder_ms": round(hip_ms[0], 3),
               "hip_decoder_ms_min_max": [round(hip_ms[1], 3), round(hip_ms[2], 3)],
               "hip_us_per_step": round(hip_ms[0] * 1e3 / (n_dec * len(chunks)), 2),
               "hip_launch_only_ms": round(launch_ms, 3),
               "hip_launch_only_us_per_step": round(launch_ms * 1e3 / (n_dec * len(chunks)), 2),
               "hip_us_per_sentence_step": round(hip_ms[0] * 1e3 / (n_dec * N), 3),
               "torch_sentences_timed": ns, "torch_decoder_ms": round(torch_ms[0], 3),
               "torch_us_per_sentence_step": round(torch_ms[0] * 1e3 / (n_dec * ns), 2),
               "decoder_speedup": round((torch_ms[0] / ns) / (hip_ms[0] / N), 2), "postnet_ms": round(post_ms[0], 3)}
        if not args.no_vocoder:
            note("synthesize_list")
            lst = median(lambda: gt.synthesize_list(tts, voc, xs, seed=1, steps=args.steps), args.reps, wall_ms)
            n1 = min(N, args.single_sample)

            def singles():
                out = []
                for i in range(n1):
                    _, m, _ = tts.generate(xs[i], steps=args.steps, backend="torch")
                    out.append(voc.generate(gt.tacotron_mel_to_vocoder(m), None, False, 11000, 550, True, seed=1 + i,
                                            verbose=False))
                return out
            note("single calls")
            one = median(singles, args.reps, wall_ms)
            seconds = N * (args.steps - 1) * vd.hop_length / vd.sample_rate
            row.update({"list_ms": round(lst[0], 1), "list_ms_min_max": [round(lst[1], 1), round(lst[2], 1)],
                        "list_x_realtime": round(seconds / (lst[0] / 1e3), 1), "single_sentences_timed": n1,
                        "single_ms_scaled_to_n": round(one[0] / n1 * N, 1), "list_speedup": round(one[0] / n1 * N / lst[0], 2),
                        "decoder_share": round(hip_ms[0] / lst[0], 3), "encoder_share": round(enc_ms[0] / lst[0], 3),
                        "postnet_share": round(post_ms[0] / lst[0], 3)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
