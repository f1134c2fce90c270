"""TTS caller on the MI355X vocoder — the WaveRNN half of the reference's gen_tacotron.py.

The reference synthesises each sentence with its PyTorch Tacotron and hands the mel to
`WaveRNN.generate()` (gen_tacotron.py:142-168):

    _, m, attention = tts_model.generate(x)          # :145
    m = (m + 4) / 8; np.clip(m, 0, 1, out=m)          # :147-148  (Tacotron scale → [0, 1])
    m = torch.tensor(m).unsqueeze(0)                  # :167
    voc_model.generate(m, save_path, batched, hp.voc_target, hp.voc_overlap, hp.mu_law)   # :168

The text front-end and Griffin-Lim stay outside this package: `synthesize()` takes any object
with the reference Tacotron's `generate(x)` triple and any sequence of already-encoded inputs
(`text_to_sequence` output), so `wavernn_amd.tacotron.Tacotron` (decoder loop on the GPU) and the
reference's own PyTorch Tacotron both drop in. `synthesize_list()` runs all sentences at once:
`tts_model.generate_list` → the same rescale → `voc_model.generate_list(wide=True)`. The CLI
vocodes mels that a Tacotron run saved as .npy (Tacotron scale, before the :147 rescale), or
synthesises encoded sentences from a Tacotron checkpoint:

    python -m wavernn_amd.gen_tacotron -m mel0.npy mel1.npy [-b|-u] [-t T] [-o O]
                                       [--voc_weights W.pyt] [--hp_file hparams.py]
                                       [--tts_k K] [--out_dir DIR] [--names a b ...]
    python -m wavernn_amd.gen_tacotron --tts_weights T.pyt --sequences ids.txt|ids.npy [--cbhg torch|hip] [...]

`--sequences` is a .npy of integer ids (1-D: one sentence; 2-D: one sentence per row) or a text file
with one line of integer ids per sentence. With `--sequences` the sentences go through
`synthesize_list` (the unbatched wide vocoder list): -b / -u, --target and --overlap do not apply and
are refused.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

from .hparams import HParams


def tacotron_mel_to_vocoder(m) -> torch.Tensor:
    """gen_tacotron.py:147-148 and :167 — Tacotron mel (n_mels, T) in its [-4, 4] scale →
    the (1, n_mels, T) [0, 1] tensor WaveRNN.generate() expects. Same float arithmetic as the
    reference: (m + 4) / 8 in the input's dtype, then clip."""
    m = np.asarray(m)
    m = (m + 4) / 8
    np.clip(m, 0, 1, out=m)
    return torch.tensor(m).unsqueeze(0)


def output_name(i: int, v_type: str, tts_k: int, input_text: Optional[str] = None,
                standard_name: Optional[str] = None) -> str:
    """Wav file name of sentence i (1-based), gen_tacotron.py:157-162."""
    if standard_name is not None:
        return f'{standard_name}.wav'
    if input_text:
        return f'__input_{input_text[:10]}_{v_type}_{tts_k}k.wav'
    return f'{i}_{v_type}_{tts_k}k.wav'


def vocoder_type(batched: bool) -> str:
    """gen_tacotron.py:150-155 (the WaveRNN branches)."""
    return 'wavernn_batched' if batched else 'wavernn_unbatched'


def synthesize(tts_model, voc_model, inputs: Sequence, out_dir: Path, batched: bool, target: int, overlap: int,
               mu_law: bool, tts_k: int = 0, input_text: Optional[str] = None,
               standard_names: Optional[Sequence[str]] = None, seed: Optional[int] = None,
               save_attention: Optional[Callable] = None) -> List[np.ndarray]:
    """gen_tacotron.py:142-168 with the vocoder on the MI355X path: for each encoded input,
    Tacotron (PyTorch, the caller's) → rescale → `voc_model.generate()`. Returns the waveforms."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    v_type = vocoder_type(batched)
    wavs = []
    for i, x in enumerate(inputs, 1):
        print(f'\n| Generating {i}/{len(inputs)}')
        _, m, attention = tts_model.generate(x)
        name = output_name(i, v_type, tts_k, input_text, standard_names[i - 1] if standard_names else None)
        save_path = out_dir / name
        if save_attention is not None:
            save_attention(attention, save_path)
        mel = tacotron_mel_to_vocoder(m)
        s = None if seed is None else seed + i - 1
        wavs.append(voc_model.generate(mel, save_path, batched, target, overlap, mu_law, seed=s))
    return wavs


def synthesize_list(tts_model, voc_model, inputs: Sequence, out_dir: Optional[Path] = None, tts_k: int = 0,
                    standard_names: Optional[Sequence[str]] = None, seed: Optional[int] = None, steps: int = 2000,
                    save_attention: Optional[Callable] = None, cbhg: Optional[str] = None) -> List[np.ndarray]:
    """All sentences at once: `tts_model.generate_list(inputs)` (one decoder launch per 128
    sentences), the :147-148 rescale of the second returned array as the reference takes it, then
    `voc_model.generate_list(mels, wide=True)`. With `out_dir` the waveforms are saved under the
    names `synthesize()` would give them. `cbhg` ('torch' / 'hip') is handed to `generate_list` when given:
    'hip' runs the list's encoders and postnets as ragged HIP passes. Returns the waveforms in the order
    of `inputs`."""
    from .dsp import save_wav
    kw = {} if cbhg is None else {'cbhg': cbhg}
    triples = tts_model.generate_list(list(inputs), steps=steps, **kw)
    mels = [tacotron_mel_to_vocoder(m) for _, m, _ in triples]
    wavs = voc_model.generate_list(mels, seed=seed, wide=True)
    if out_dir is not None:
        out_dir = Path(out_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        for i, (w, (_, _, attention)) in enumerate(zip(wavs, triples), 1):
            name = output_name(i, 'wavernn_list', tts_k, None, standard_names[i - 1] if standard_names else None)
            if save_attention is not None:
                save_attention(attention, out_dir / name)
            save_wav(np.asarray(w), out_dir / name)
    return wavs


def load_sequences(path: Union[str, Path]) -> List[np.ndarray]:
    """`--sequences FILE`: a .npy of ids (1-D: one sentence; 2-D: one per row) or a text file with one
    line of integer ids (blank- or comma-separated) per sentence."""
    p = Path(path)
    if p.suffix == '.npy':
        a = np.load(p, allow_pickle=False)
        if a.ndim not in (1, 2) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f'Expected a 1-D or 2-D integer array of symbol ids, but got {a.dtype} {a.shape}!')
        return [np.asarray(r, dtype=np.int64) for r in (a[None] if a.ndim == 1 else a)]
    seqs = []
    for n, line in enumerate(p.read_text().splitlines(), 1):
        line = line.replace(',', ' ').strip()
        if not line:
            continue
        try:
            seqs.append(np.array([int(t) for t in line.split()], dtype=np.int64))
        except ValueError:
            raise ValueError(f'{p}:{n}: expected integer symbol ids') from None
    if not seqs:
        raise ValueError(f'{p} holds no sentence')
    return seqs


class _SavedMels:
    """Stands in for Tacotron when its mels were saved to disk: generate(i) → (None, mel, None)."""

    def __init__(self, paths: Sequence[Path], n_mels: int):
        self.paths = [Path(p) for p in paths]
        self.n_mels = n_mels

    def generate(self, i):
        p = self.paths[i]
        if p.suffix != '.npy':
            raise ValueError(f'Expected a .npy Tacotron mel, got {p.suffix}')
        m = np.load(p, allow_pickle=False)
        if m.ndim != 2 or m.shape[0] != self.n_mels:
            raise ValueError(f'Expected a numpy array shaped (n_mels, n_frames), but got {m.shape}!')
        return None, m, None


def main(argv=None):
    ap = argparse.ArgumentParser(description='Vocode Tacotron mels on MI355X (gen_tacotron.py, wavernn branch)')
    ap.add_argument('--mels', '-m', nargs='+', help='Tacotron mel .npy files (Tacotron scale)')
    ap.add_argument('--tts_weights', type=str, help='reference-format Tacotron state_dict (*.pyt)')
    ap.add_argument('--sequences', metavar='FILE', help='encoded sentences: .npy, or one line of ids per sentence (vocoded as one unbatched wide list; '
                         'not with -b / -u / -t / -o)')
    ap.add_argument('--batched', '-b', dest='batched', action='store_true', help='Fast Batched Generation')
    ap.add_argument('--unbatched', '-u', dest='batched', action='store_false', help='Slow Unbatched Generation')
    ap.add_argument('--overlap', '-o', type=int)
    ap.add_argument('--target', '-t', type=int)
    ap.add_argument('--voc_weights', type=str, help='reference-format WaveRNN state_dict (*.pyt)')
    ap.add_argument('--hp_file', metavar='FILE', default=None)
    ap.add_argument('--tts_k', type=int, default=0, help='Tacotron step / 1000, for the file names')
    ap.add_argument('--names', nargs='*', default=None, help='output names (hp.test_sentences_names)')
    ap.add_argument('--out_dir', default='.')
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--cbhg', choices=('torch', 'hip'), default=None,
                    help='with --sequences: the Tacotron encoder / postnet CBHGs as torch modules (default) or ragged HIP passes')
    ap.set_defaults(batched=None)
    args = ap.parse_args(argv)
    hp = HParams().configure(args.hp_file)
    target = args.target if args.target is not None else hp.voc_target
    overlap = args.overlap if args.overlap is not None else hp.voc_overlap
    batched = args.batched if args.batched is not None else hp.voc_gen_batched
    if (args.mels is None) == (args.sequences is None):
        ap.error('give either --mels or --sequences')
    if args.sequences is not None and not args.tts_weights:
        ap.error('--sequences needs --tts_weights')
    if args.sequences is not None and (args.batched is not None or args.target is not None or args.overlap is not None):
        ap.error('--sequences vocodes through the unbatched wide list: -b / -u, --target and --overlap do not apply')
    seqs = load_sequences(args.sequences) if args.sequences is not None else None
    if args.names is not None and len(args.names) != len(args.mels if seqs is None else seqs):
        raise ValueError('--names needs one name per ' + ('mel' if seqs is None else 'sentence'))
    if not torch.cuda.is_available():
        raise RuntimeError('the MI355X generation path needs a GPU')
    from .gen_wavernn import build_model
    voc = build_model(hp, torch.device('cuda'))
    if args.voc_weights:
        voc.load(args.voc_weights)
    if seqs is not None:
        from .tacotron import build_tacotron
        tts = build_tacotron(hp, weights=args.tts_weights, device=torch.device('cuda'))
        synthesize_list(tts, voc, seqs, Path(args.out_dir), tts_k=args.tts_k or tts.get_step() // 1000,
                        standard_names=args.names, seed=args.seed, cbhg=args.cbhg)
        print('\n\nDone.\n')
        return
    tts = _SavedMels(args.mels, hp.num_mels)
    synthesize(tts, voc, list(range(len(args.mels))), Path(args.out_dir), batched, target, overlap, hp.mu_law,
               tts_k=args.tts_k, standard_names=args.names, seed=args.seed)
    print('\n\nDone.\n')


if __name__ == '__main__':
    main()
