"""Vocoder CLI on the MI355X path — the reference's gen_wavernn.py:68-150 flags.

    python -m wavernn_amd.gen_wavernn -f mel.npy|x.wav [-b|-u] [-t T] [-o O] [-w weights.pyt]
                                      [--hp_file hparams.py] [--out_dir DIR] [--stream-chunk N]

Mel input is a normalised (n_mels, n_hops) .npy in [0, 1] (checked like gen_wavernn.py:48-57).
A .wav is copy synthesis as in the reference (gen_wavernn.py:38-65): load_wav, the target written
next to the output as __{name}__{k}k_steps_target.wav, its mel computed on the GPU by the front-end
kernel (WaveRNN.melspectrogram — librosa's definition restated), then the same
path as a .npy.  Unlike the reference's librosa.load, load_wav does not resample: a file at another
rate than hp.sample_rate raises.  The test-set mode needs the training data pipeline, which is out
of scope; it raises.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

from .hparams import HParams


def build_model(hp, device):
    from .fatchord_version import WaveRNN
    return WaveRNN(rnn_dims=hp.voc_rnn_dims, fc_dims=hp.voc_fc_dims, bits=hp.bits, pad=hp.voc_pad,
                   upsample_factors=hp.voc_upsample_factors, feat_dims=hp.num_mels,
                   compute_dims=hp.voc_compute_dims, res_out_dims=hp.voc_res_out_dims,
                   res_blocks=hp.voc_res_blocks, hop_length=hp.hop_length, sample_rate=hp.sample_rate,
                   mode=hp.voc_mode).to(device)


def load_mel(path: Path, n_mels: int) -> np.ndarray:
    if path.suffix != ".npy":
        raise ValueError(f"Expected a .npy mel (a .wav goes through load_target_wav), got {path.suffix}")
    mel = np.load(path, allow_pickle=False)
    if mel.ndim != 2 or mel.shape[0] != n_mels:
        raise ValueError(f"Expected a numpy array shaped (n_mels, n_hops), but got {mel.shape}!")
    if mel.max() >= 1.01 or mel.min() <= -0.01:
        raise ValueError(f"Expected spectrogram range in [0,1] but was instead [{mel.min()}, {mel.max()}]")
    return mel


def load_target_wav(path: Path, hp) -> np.ndarray:
    """The wav branch of --file: the signal at hp.sample_rate, long enough for the front end's
    reflect padding (load_mel keeps refusing anything but a .npy)."""
    from . import dsp
    wav = dsp.load_wav(path, hp.sample_rate)
    if wav.ndim != 1 or len(wav) < hp.n_fft // 2 + 1:
        raise ValueError(f"{path}: need a mono signal of at least n_fft//2 + 1 = {hp.n_fft // 2 + 1} samples")
    return wav


def stream_wav(model, wav: np.ndarray, samples_per_push: int, seed: int, hp) -> list:
    """The wav through a streaming session, `samples_per_push` samples at a time (push_audio)."""
    def run(**kw):
        with model.stream(1, total_samples=len(wav), seed=seed, hp=hp, **kw) as s:
            out = [s.push_audio(wav[i:i + samples_per_push])[0] for i in range(0, len(wav), samples_per_push)]
            return out + [s.finish_audio()[0]]
    try:
        return run()
    except NotImplementedError:
        # no XCD-resident session kernel for this model: the multi-row kernel's sessions take any
        return run(rows=True, mu_law=hp.mu_law)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Generate WaveRNN samples on MI355X")
    ap.add_argument("--batched", "-b", dest="batched", action="store_true", help="Fast Batched Generation")
    ap.add_argument("--unbatched", "-u", dest="batched", action="store_false", help="Slow Unbatched Generation")
    ap.add_argument("--target", "-t", type=int)
    ap.add_argument("--overlap", "-o", type=int)
    ap.add_argument("--file", "-f", type=str, required=True, help="mel .npy to vocode, or a .wav to copy-synthesise")
    ap.add_argument("--voc_weights", "-w", type=str, help="reference-format state_dict (*.pyt)")
    ap.add_argument("--hp_file", metavar="FILE", default=None)
    ap.add_argument("--out_dir", default=".")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--stream-chunk", type=int, default=None, metavar="N",
                    help="unbatched only: vocode through a streaming session, N mel frames (for a .wav: N·hop samples) "
                         "per push (same wav)")
    ap.set_defaults(batched=None)
    args = ap.parse_args(argv)
    hp = HParams().configure(args.hp_file)
    target = args.target if args.target is not None else hp.voc_target
    overlap = args.overlap if args.overlap is not None else hp.voc_overlap
    batched = args.batched if args.batched is not None else hp.voc_gen_batched
    if args.stream_chunk is not None:
        if batched:
            ap.error("--stream-chunk streams the unbatched loop: pass -u")
        if args.stream_chunk < 1:
            ap.error("--stream-chunk needs a positive frame count")
    path = Path(args.file).expanduser()
    wav = load_target_wav(path, hp) if path.suffix == ".wav" else None
    if not torch.cuda.is_available():
        raise RuntimeError("the MI355X generation path needs a GPU")
    model = build_model(hp, torch.device("cuda"))
    if args.voc_weights:
        model.load(args.voc_weights)
    mel = None if wav is not None else torch.from_numpy(load_mel(path, hp.num_mels)).unsqueeze(0)
    k = model.get_step() // 1000
    if wav is not None:
        from . import dsp
        dsp.save_wav(wav, Path(args.out_dir) / f"__{path.stem}__{k}k_steps_target.wav", hp.sample_rate)
        if args.stream_chunk is None:
            mel = model.melspectrogram(wav, hp)[0]
    tag = f"gen_batched_target{target}_overlap{overlap}" if batched else "gen_NOT_BATCHED"
    out = Path(args.out_dir) / f"__{path.stem}__{k}k_steps_{tag}.wav"
    if args.stream_chunk is not None:
        from . import dsp
        model.eval()
        seed = args.seed if args.seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
        if wav is not None:
            chunks = stream_wav(model, wav, args.stream_chunk * hp.hop_length, seed, hp)
        else:
            try:
                chunks = list(model.generate_stream(mel, args.stream_chunk, seed=seed))
            except NotImplementedError:
                # no XCD-resident session kernel for this model: the multi-row kernel's sessions take any
                chunks = list(model.generate_stream(mel, args.stream_chunk, seed=seed, rows=True, mu_law=hp.mu_law))
        dsp.save_wav(np.concatenate(chunks), out, hp.sample_rate)
    else:
        model.generate(mel, out, batched, target, overlap, hp.mu_law, seed=args.seed)
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
