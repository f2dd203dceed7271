"""`python -m mindaudio_amd.wavegrad.reverse --config wavegrad_base.yaml --restore ckpt (--mel x.npy | --wav x.wav) --save dir` - the
counterpart of examples/wavegrad/reverse.py: the reverse diffusion loop of a WaveGrad vocoder, kept on the device.

It takes the reference's flags, prints its `old:` / `feature:` / `restore:` / `audio:` lines and writes its ten
`%d_predicted_%s_%d.wav` files, one for every 5th of the last 50 steps.  `--plot` and the gif are not built: `--plot True` raises
before anything else (the reference's default is True; here it is False).  `--restore_url`, `--data_url`, `--train_url`,
`--device_target` and `--device_id` are accepted and ignored.  Two flags are added: `--noise numpy|device` (where the Gaussian draws come
from, see `reverse`) and `--seed`."""
import argparse
import ast
import os
import wave

import numpy as np


def schedule(beta):
    """reverse.py:101-123 on the host.  alpha_cum is float32 as the script casts it (:103); c1, c2, sigma are float64 here and
    handed to the device as float32.  -> (noise_level (S,) float32 = sqrt(alpha_cum), c1, c2, sigma (S,) float64; sigma[0] = 0)."""
    beta = np.asarray(beta, np.float64).reshape(-1)
    alpha = 1 - beta
    alpha_cum = np.cumprod(alpha).astype(np.float32)
    c1 = 1 / alpha ** 0.5
    c2 = (1 - alpha) / (1 - alpha_cum.astype(np.float64)) ** 0.5
    sigma = np.zeros_like(c1)
    a64 = alpha_cum.astype(np.float64)
    sigma[1:] = ((1.0 - a64[:-1]) / (1.0 - a64[1:]) * beta[1:]) ** 0.5
    return alpha_cum ** 0.5, c1, c2, sigma


def snapshot_steps(S):
    """The loop counts m + 1 at which the script writes a file (reverse.py:125)."""
    return [m + 1 for m in range(S) if (m + 1) > (S - 50) and (m + 1) % 5 == 0]


def reverse(model, feature, beta=None, noise="numpy", seed=None, chunk=50, hps=None, _network=None):
    """The S-step loop of reverse.py:98-131 -> (audio (B, T) float32 on the device, {m + 1: audio} for the script's steps).

    feature (B, n_mels, frames) float32 (ndarray or tensor).  beta: any 1-D schedule; None = the yaml's linspace(noise_schedule_start,
    noise_schedule_end, noise_schedule_S) of `hps`.  noise="numpy" draws with the reference's np.random call order (seed != None:
    np.random.seed(seed) first): the initial audio as one normal(0, 1, [B, T]) cast to float32, then one float64 normal(0, 1, [B, T])
    per step with n > 0, cast to float32 and uploaded in chunks of `chunk` steps.  noise="device" draws with torch.randn from a
    generator on the device: nothing comes from the host inside the loop.  Under NumPy < 2, which the reference pins, `audio` stays
    float32 through the loop; that is what the device does.  Every chunk is one ma_wavegrad_reverse call; a chunk also ends at every
    step the script writes a file for.  `_network(audio, n) -> pred (B, T)`: a stand-in for the network (tests)."""
    import torch

    from .. import _host, _lib
    from ..models.wavegrad import positional_table

    if noise not in ("numpy", "device"):
        raise ValueError("noise must be 'numpy' or 'device'")
    if beta is None:
        beta = np.linspace(hps.noise_schedule_start, hps.noise_schedule_end, hps.noise_schedule_S)
    level, c1, c2, sigma = schedule(beta)
    S = len(level)
    if S < 1 or chunk < 1:
        raise ValueError("the schedule and the chunk must hold at least one step")
    _host.require_gpu()
    dev = model.last_conv.weight.device
    feature = torch.as_tensor(np.asarray(feature) if not torch.is_tensor(feature) else feature).to(device=dev, dtype=torch.float32)
    if feature.dim() != 3:
        raise ValueError("feature must be (B, n_mels, frames)")
    B, T = feature.shape[0], model.hop * feature.shape[2]
    gen = None
    if noise == "numpy":
        if seed is not None:
            np.random.seed(seed)
        audio = torch.from_numpy(np.random.normal(0, 1, [B, T]).astype(np.float32)).to(dev)
    else:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0 if seed is None else int(seed))
        audio = torch.randn((B, T), generator=gen, device=dev, dtype=torch.float32)
    mel = model.mel_rows(feature)
    enc = torch.from_numpy(positional_table(level, model.enc_dims)).to(dev)
    c1f, c2f, sgf = (v.astype(np.float32) for v in (c1, c2, sigma))
    stops = set(snapshot_steps(S))
    saved = {}
    m = 0
    while m < S:
        n_steps = min(chunk, S - m)
        for k in range(1, n_steps + 1):  # a chunk ends where the script writes a file
            if m + k in stops:
                n_steps = k
                break
        n_noise = n_steps - 1 if m + n_steps == S else n_steps
        draws = None
        if n_noise:
            if noise == "numpy":
                draws = torch.from_numpy(np.stack([np.random.normal(0, 1, [B, T]).astype(np.float32) for _ in range(n_noise)])).to(dev)
            else:
                draws = torch.randn((n_noise, B, T), generator=gen, device=dev, dtype=torch.float32)
        if _network is None:
            model.reverse_steps(audio, mel, enc, c1f, c2f, sgf, draws, m, n_steps)
        else:  # pred comes from the stand-in; the update is the same kernel: a (1 tap, 4 channel) last_conv that copies channel 0
            lib = _lib.load()
            w = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
            zero = torch.zeros((4,), device=dev)
            for k in range(n_steps):
                n = S - 1 - (m + k)
                x = torch.zeros((B, T, 4), device=dev)
                x[:, :, 0] = _network(audio, n)
                _lib.check(lib.ma_wavegrad_last_conv_update_f32(
                    x.data_ptr(), B, T, 4, w.data_ptr(), zero.data_ptr(), 1, audio.data_ptr(), draws[k].data_ptr() if n > 0 else None,
                    float(c1f[n]), float(c2f[n]), float(sgf[n]), audio.data_ptr(), None, _host.current_stream_ptr()), "wavegrad_update")
        m += n_steps
        if m in stops:
            saved[m] = audio.clone()
    return audio, saved


def write_wav(path, samples, rate):
    """A mono 16-bit PCM file: samples * 32768, rounded, clipped to the int16 range (data.io.read divides by 32768)."""
    pcm = np.clip(np.rint(np.asarray(samples, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(int(rate))
        fh.writeframes(pcm.tobytes())


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="WaveGrad reverse diffusion")
    parser.add_argument("--device_target", type=str, default="GPU", choices=("GPU", "CPU", "Ascend"))
    parser.add_argument("--device_id", "-i", type=int, default=0)
    parser.add_argument("--save", "-s", type=str, default="results")
    parser.add_argument("--plot", "-p", type=ast.literal_eval, default=False)
    parser.add_argument("--config", "-c", type=str, default="wavegrad_base.yaml")
    parser.add_argument("--restore", "-r", type=str, default="")
    parser.add_argument("--restore_url", "-u", type=str, default="")
    parser.add_argument("--wav", "-w", type=str, default="data/LJspeech-1.1/wavs")
    parser.add_argument("--mel", "-m", type=str, default=None)
    parser.add_argument("--data_url", default="")
    parser.add_argument("--train_url", default="")
    parser.add_argument("--noise", default="numpy", choices=("numpy", "device"))
    parser.add_argument("--seed", type=int, default=None)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.plot:
        raise NotImplementedError("--plot: the mel plots and the gif are not built")
    import torch

    from .. import _host
    from ..models import WaveGrad
    from ..utils.ckpt import load_mindspore_checkpoint, read_mindspore_ckpt
    from .config import load_config
    from .preprocess import mel_features, read_wav

    hps = load_config(args.config)
    os.makedirs(args.save, exist_ok=True)
    _host.require_gpu()
    if args.mel is not None:
        feature = np.load(args.mel)
        if len(feature.shape) == 2:
            feature = feature[None, ...]
        if feature.shape[-1] == hps.n_mels:
            feature = feature.transpose([0, 2, 1])
        old = args.mel.split("/")[-1].replace(".npy", "")
    else:
        feature = mel_features(read_wav(args.wav)[0], hps)[None, ...]
        old = args.wav.split("/")[-1].replace(".wav", "")
    print("old:", old)
    print("feature:", tuple(feature.shape))
    model = WaveGrad(hps).to(torch.device("cuda", torch.cuda.current_device())).eval()
    global_step = 0
    if args.restore:
        load_mindspore_checkpoint(model, args.restore)
        raw = read_mindspore_ckpt(args.restore)
        global_step = int(np.asarray(raw["cur_step"]).reshape(-1)[0]) if "cur_step" in raw else 0
    print("restore:", global_step)
    frames = feature.shape[-1]
    # the reference holds hop_samples * frames samples (reverse.py:105-108): a mel that was cut to whole frames
    print("audio:", (feature.shape[0], hps.hop_samples * frames))
    audio, saved = reverse(model, feature, noise=args.noise, seed=args.seed, hps=hps)
    for step in sorted(saved):
        write_wav(args.save + "/%d_predicted_%s_%d.wav" % (global_step, old, step), saved[step][0].cpu().numpy(), hps.sample_rate)
    return audio, saved


if __name__ == "__main__":
    main()
