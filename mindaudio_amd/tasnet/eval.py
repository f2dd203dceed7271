"""`python -m mindaudio_amd.tasnet.eval --config_path tasnet.yaml` - the counterpart of examples/tasnet/eval.py.

Reads the example's yaml keys (data_dir, eval_batch_size, sample_rate, model_path, L, N, hidden_size, num_layers, bidirectional, nspk,
cal_sdr), builds TasNet, loads the MindSpore checkpoint, and for batches of eval_batch_size utterances (each 3320 segments of L samples)
runs the model on the device, Separation_Loss (permutation by pairwise SI-SNR, no padding mask) and, per utterance on the host,
cal_SISNRi over all 3320 * L samples, as the reference's remove_pad_and_flat keeps them.  It logs the reference's lines: `Utt n`,
`\\tSI-SNRi=x.xx`, and at the end `Average SISNR improvement: x.xx`.

`cal_sdr: 1` raises: cal_SDRi needs mir_eval's bss_eval_sources, which this package does not depend on."""
import argparse

import numpy as np

from .data import SEGMENTS, DatasetGenerator


def build_model(config):
    from ..models import TasNet
    from ..utils.ckpt import load_mindspore_checkpoint

    model = TasNet(int(config["L"]), int(config["N"]), int(config["hidden_size"]), int(config["num_layers"]),
                   bidirectional=bool(int(config.get("bidirectional", 0) or 0)), nspk=int(config.get("nspk", 2)),
                   **({"schedule": config["schedule"]} if config.get("schedule") else {}))
    load_mindspore_checkpoint(model, str(config["model_path"]))
    return model


def evaluate(config, model=None, log=print):
    """eval.py:61-129 on a config mapping; returns (average SI-SNRi, [SI-SNRi per utterance]).  `model`: a callable
    (mixture (b, K, L) float32 device tensor) -> (b, 2, K, L) used as it is, instead of the one built from the config and loaded from
    config["model_path"].  `segments` (not a key of the reference's yaml; default 3320) is handed to DatasetGenerator."""
    import torch

    from .. import _host
    from ..loss import Separation_Loss
    from ..metric import cal_SISNRi

    if int(config.get("cal_sdr", 0) or 0):
        raise NotImplementedError("cal_sdr: cal_SDRi needs mir_eval.separation.bss_eval_sources and is not built")
    _host.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    if model is None:
        log("=====> load params into generator")
        model = build_model(config).to(dev).eval()
        log("=====> finish load generator")
    batch = int(config["eval_batch_size"])
    dataset = DatasetGenerator(config["data_dir"], batch, sample_rate=int(config["sample_rate"]), L=int(config["L"]),
                               segments=int(config.get("segments", SEGMENTS) or SEGMENTS))
    loss_fn = Separation_Loss()
    values = []
    for first in range(0, len(dataset), batch):
        items = [dataset[i] for i in range(first, min(first + batch, len(dataset)))]
        padded_mixture = torch.from_numpy(np.stack([it[0] for it in items])).to(dev)
        lengths = torch.tensor([int(it[1]) for it in items])
        padded_source = torch.from_numpy(np.stack([it[2] for it in items])).to(dev)
        estimate = model(padded_mixture)  # (b, C, K, L)
        _, _, _, reordered = loss_fn(padded_source, estimate, lengths)
        b = len(items)
        mix_np = padded_mixture.reshape(b, -1).cpu().numpy()  # remove_pad_and_flat, eval.py:132-149: nothing is removed
        src_np = padded_source.reshape(b, padded_source.shape[1], -1).cpu().numpy()
        est_np = reordered.reshape(b, reordered.shape[1], -1).cpu().numpy()
        for i in range(b):
            log("Utt %d" % (len(values) + 1))
            v = float(cal_SISNRi(src_np[i], est_np[i], mix_np[i]))
            log("\tSI-SNRi={0:.2f}".format(v))
            values.append(v)
    if not values:
        raise ValueError("no utterance to evaluate")
    average = sum(values) / len(values)
    log("Average SISNR improvement: {0:.2f}".format(average))
    return average, values


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    for key in ("data_dir", "model_path", "schedule"):
        ap.add_argument("--" + key)
    for key in ("eval_batch_size", "sample_rate", "cal_sdr", "L", "N", "hidden_size", "num_layers", "bidirectional", "nspk", "segments"):
        ap.add_argument("--" + key, type=int)
    a = ap.parse_args(argv)
    over = {k: v for k, v in vars(a).items() if k != "config_path" and v is not None}
    return evaluate(load_config(a.config_path, over))


if __name__ == "__main__":
    main()
