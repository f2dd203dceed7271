"""examples/fastspeech2/generate.py on MI355X: one sentence -> mel spectrogram (msfs2_0.npy), optionally -> audio through WaveGrad.

    python -m mindaudio_amd.fastspeech2.generate --restore ckpt --ids ids.npy
    python -m mindaudio_amd.fastspeech2.generate --restore ckpt --phonemes "{HH AH0 L OW1}" --symbols symbols.txt
    python -m mindaudio_amd.fastspeech2.generate --restore ckpt --text "hello world" --lexicon lexicon.txt --symbols symbols.txt

The front end: the reference's g2p_en, pypinyin, cleaners and its LibriSpeech lexicon are not part of this package.  `--ids` takes the
token ids as they are; `--phonemes` maps the names between braces through `--symbols` (one symbol per line in id order, the space
written as <space>; tests/golden/fastspeech2_symbols.txt is the reference's table); `--text` looks every word up in `--lexicon` with the
reference's splitting and {sp} rule, and a word that is not in the lexicon is an error (the reference falls back to g2p_en, which is not
built).  `--vocoder ckpt --config wavegrad_base.yaml` hands mel_predictions to mindaudio_amd.wavegrad.reverse and writes msfs2_0.wav:
both examples store _normalize(mel) (20 log10, -20, +100, / 100, clipped to 0 .. 1) of the same 128-bin, hop-300, f_min-20 spectrogram, so
no conversion is needed; the prediction is not clipped by either example, and is handed over as it is."""
import argparse
import os
import re
from string import punctuation

import numpy as np


def read_symbols(path):
    with open(path) as fh:
        names = [line.rstrip("\n") for line in fh if line.rstrip("\n") != ""]
    return {(" " if s == "<space>" else s): i for i, s in enumerate(names)}


def phonemes_to_sequence(text, symbol_to_id):
    """text_to_sequence (text/__init__.py:15-41) for input that is ARPAbet between braces: what lies outside braces would go through
    the cleaners, which are not built."""
    seq, rest = [], text
    curly = re.compile(r"(.*?)\{(.+?)\}(.*)")
    while rest:
        m = curly.match(rest)
        if not m or m.group(1).strip():
            raise NotImplementedError("text outside {braces} needs the reference's cleaners, which are not built: %r" % rest)
        seq += [symbol_to_id[s] for s in ("@" + p for p in m.group(2).split()) if s in symbol_to_id and s not in ("_", "~")]
        rest = m.group(3)
    return seq


def read_lexicon(path):
    lexicon = {}
    with open(path) as fh:
        for line in fh:
            temp = re.split(r"\s+", line.strip("\n"))
            if temp[0].lower() not in lexicon:
                lexicon[temp[0].lower()] = temp[1:]
    return lexicon


def text_to_phonemes(text, lexicon):
    """preprocess_english (generate.py:33-47) without g2p_en."""
    text = text.rstrip(punctuation)
    phones = []
    for w in re.split(r"([,;.\-\?\!\s+])", text):
        if w.lower() in lexicon:
            phones += lexicon[w.lower()]
        elif re.fullmatch(r"[A-Za-z']+", w):
            raise NotImplementedError("%r is not in the lexicon, and the g2p_en fallback is not built" % w)
        else:
            phones += [p for p in w if p != " "]  # punctuation stands for itself, as in g2p_en's output
    phones = "{" + "}{".join(phones) + "}"
    phones = re.sub(r"\{[^\w\s]?\}", "{sp}", phones)
    return phones.replace("}{", " ")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="FastSpeech2 generate")
    parser.add_argument("--device_target", type=str, default="GPU", choices=("GPU", "CPU", "Ascend"))
    parser.add_argument("--device_id", "-i", type=int, default=0)
    parser.add_argument("--context_mode", type=str, default="py", choices=["py", "graph"])
    parser.add_argument("--text", "-t", type=str, default=None)
    parser.add_argument("--restore", "-r", type=str, default="")
    parser.add_argument("--data_url", default="")
    parser.add_argument("--train_url", default="")
    parser.add_argument("--fs2_config", type=str, default="fastspeech2.yaml")
    parser.add_argument("--ids", type=str, default=None)
    parser.add_argument("--phonemes", type=str, default=None)
    parser.add_argument("--symbols", type=str, default=None)
    parser.add_argument("--lexicon", type=str, default=None)
    parser.add_argument("--norm", type=str, default="group", choices=("group", "layer"))
    parser.add_argument("--vocoder", type=str, default=None)
    parser.add_argument("--config", "-c", type=str, default="wavegrad_base.yaml")
    parser.add_argument("--save", "-s", type=str, default=".")
    parser.add_argument("--seed", type=int, default=0)
    return parser.parse_args(argv)


def main(argv=None, hps=None):
    args = parse_args(argv)
    import torch

    from .. import _host
    from ..models import FastSpeech2
    from ..utils.ckpt import load_mindspore_checkpoint
    from ..wavegrad.config import load_config

    if hps is None:
        hps = load_config(args.fs2_config)
    vhps = load_config(args.config) if args.vocoder else None
    if vhps is not None and (vhps.n_mels, vhps.hop_samples, vhps.sample_rate) != (hps.n_mels, hps.hop_samples, hps.sample_rate):
        raise ValueError("the vocoder's mel geometry (n_mels, hop_samples, sample_rate) differs from FastSpeech2's")  # before any work
    if args.ids is not None:
        sequence = np.load(args.ids).astype(np.int64).reshape(-1)
    else:
        if args.symbols is None:
            raise ValueError("--phonemes / --text need --symbols (one symbol per line in id order)")
        phones = args.phonemes
        if phones is None:
            if args.text is None or args.lexicon is None:
                raise ValueError("give --ids, --phonemes, or --text with --lexicon")
            print("Raw Text Sequence: {}".format(args.text.rstrip(punctuation)))
            phones = text_to_phonemes(args.text, read_lexicon(args.lexicon))
        print("Phoneme Sequence:", phones)
        sequence = np.asarray(phonemes_to_sequence(phones, read_symbols(args.symbols)), np.int64)
    if sequence.size < 1:
        raise ValueError("the input maps to no token")
    _host.require_gpu()
    torch.manual_seed(args.seed)
    model = FastSpeech2(hps, norm=args.norm).to(torch.device("cuda", torch.cuda.current_device())).eval()
    if args.restore and os.path.exists(args.restore):
        print("[info] restore model from", args.restore)
        load_mindspore_checkpoint(model, args.restore, strict=False)
    texts = sequence[None, :]
    print("batchs:", 1)
    output = model.infer(speakers=np.zeros(1, np.int64), texts=texts, src_lens=np.asarray([texts.shape[1]]), max_src_len=texts.shape[1],
                         p_control=1.0, e_control=1.0, d_control=1.0)
    mel = output["mel_predictions"].cpu().numpy()
    os.makedirs(args.save, exist_ok=True)
    np.save(os.path.join(args.save, "msfs2_%s.npy" % 0), mel)
    if args.vocoder:
        from ..models import WaveGrad
        from ..wavegrad.reverse import reverse, write_wav

        vocoder = WaveGrad(vhps).to(torch.device("cuda", torch.cuda.current_device())).eval()
        load_mindspore_checkpoint(vocoder, args.vocoder)
        audio, _ = reverse(vocoder, np.ascontiguousarray(mel.transpose(0, 2, 1)), seed=args.seed, hps=vhps)
        write_wav(os.path.join(args.save, "msfs2_0.wav"), audio[0].cpu().numpy(), vhps.sample_rate)
    return output


if __name__ == "__main__":
    main()
