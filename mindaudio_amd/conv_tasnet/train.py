"""`python -m mindaudio_amd.conv_tasnet.train --config_path conv_tasnet.yaml` - the counterpart of examples/conv_tasnet/train.py.

Reads the example's yaml keys: train_dir, batch_size, sample_rate, segment, N, L, B, H, P, X, R, C, norm_type, causal, mask_nonlinear,
epochs, l2, momentum, continue_train, ckpt_path, save_folder, device_num, max_norm.  DatasetGenerator(train_dir, batch_size,
sample_rate, segment) is walked in file order, `batch_size` segments per step (a short last batch is a step of its own); the
optimizer is nn.SGD(weight_decay=l2, momentum=momentum) under piecewise_constant_lr([35, 55, 75, 100] x steps_per_epoch,
[1e-3, 1e-4, 5e-5, 1e-5]) as train.py:87-96 builds it.  The yaml's `optimizer: 'adam'` and `lr` are IGNORED, as the reference ignores
them.  One checkpoint per epoch is written to save_folder in the reference's wire format and names (Conv-TasNet-<epoch>_<steps>.ckpt,
keep_checkpoint_max = 1: the previous one is removed); `continue_train: 1` loads `ckpt_path` first.  A line per step carries epoch,
step and loss.

Not built (NotImplementedError before any device call): device_num > 1, causal: 1, max_norm > 0."""
import argparse
import os
import time

import numpy as np

from .data import DatasetGenerator

MILESTONE_EPOCHS = (35, 55, 75, 100)
LEARNING_RATES = (1e-3, 1e-4, 5e-5, 1e-5)
PREFIX = "Conv-TasNet"


def piecewise_constant_lr(milestone, learning_rates):
    """mindspore.nn.piecewise_constant_lr: a list of milestone[-1] rates, learning_rates[i] for the steps below milestone[i]."""
    if len(milestone) != len(learning_rates) or any(b <= a for a, b in zip(milestone, milestone[1:])) or milestone[0] <= 0:
        raise ValueError("milestone must be positive and increasing, one learning rate each")
    out, last = [], 0
    for m, lr in zip(milestone, learning_rates):
        out += [lr] * (m - last)
        last = m
    return out


def learning_rate(step, steps_per_epoch):
    """The rate of global step `step` (from 0); the last rate holds beyond the last milestone."""
    for e, lr in zip(MILESTONE_EPOCHS, LEARNING_RATES):
        if step < e * steps_per_epoch:
            return lr
    return LEARNING_RATES[-1]


def check_config(config):
    """The refusals, before anything touches the device."""
    if int(config.get("device_num", 1) or 1) > 1:
        raise NotImplementedError("device_num > 1: multi-GPU Conv-TasNet training is not built")
    if int(config.get("causal", 0) or 0):
        raise NotImplementedError("causal: 1 is not built (the reference's causal branch cannot run either)")
    if float(config.get("max_norm", 0) or 0) > 0:
        raise NotImplementedError("max_norm > 0: gradient clipping is not built (the reference's script never clips)")


def build_model(config):
    from ..models import ConvTasNet

    return ConvTasNet(*(int(config[k]) for k in "NLBHPXRC"), norm_type=config.get("norm_type", "gLN"),
                      causal=bool(int(config.get("causal", 0) or 0)), mask_nonlinear=config.get("mask_nonlinear", "relu"))


def train(config, log=print, operands="bf16"):
    """train.py:21-118 on a config mapping; returns the list of per-step losses."""
    check_config(config)
    import torch

    from .. import _host
    from ..models import ConvTasNetTrainer
    from ..utils import ckpt

    model = build_model(config)
    if int(config.get("continue_train", 0) or 0):
        ckpt.load_mindspore_checkpoint(model, str(config["ckpt_path"]))
    _host.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    model.to(dev)
    batch = int(config["batch_size"])
    dataset = DatasetGenerator(config["train_dir"], batch, sample_rate=int(config["sample_rate"]), segment=float(config["segment"]), log=log)
    if len(dataset) == 0:
        raise ValueError("no segment to train on: every utterance is shorter than one segment")
    steps_per_epoch = (len(dataset) + batch - 1) // batch
    trainer = ConvTasNetTrainer(model, momentum=float(config.get("momentum", 0.0)), weight_decay=float(config.get("l2", 0.0)),
                                operands=operands)
    folder = str(config["save_folder"])
    os.makedirs(folder, exist_ok=True)
    epochs, losses, step, previous = int(config["epochs"]), [], 0, None
    hop = int(config["L"]) // 2
    for epoch in range(1, epochs + 1):
        for i in range(steps_per_epoch):
            items = [dataset[j] for j in range(i * batch, min((i + 1) * batch, len(dataset)))]
            mixture = torch.from_numpy(np.stack([it[0] for it in items]).astype(np.float32)).to(dev)
            sources = torch.from_numpy(np.stack([it[2] for it in items]).astype(np.float32)).to(dev)
            T = mixture.shape[1]
            T_out = (model.num_frames(T) + 1) * hop  # the estimate's length: the targets are cut to it
            lengths = [min(int(it[1]), T_out) for it in items]
            t0 = time.time()
            lr = learning_rate(step, steps_per_epoch)
            value = trainer.step(mixture, sources[:, :, :T_out].contiguous(), lengths, lr)
            step += 1
            losses.append(value)
            log("epoch: %d step: %d, loss is %.6f (lr %.6f, %.3f s)" % (epoch, i + 1, value, lr, time.time() - t0))
        path = os.path.join(folder, "%s-%d_%d.ckpt" % (PREFIX, epoch, steps_per_epoch))
        state = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
        ckpt.write_mindspore_ckpt(path, ckpt.conv_tasnet_to_reference_names(state))
        if previous and previous != path and os.path.exists(previous):
            os.remove(previous)  # keep_checkpoint_max = 1
        previous = path
    return losses


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    for key in ("train_dir", "save_folder", "ckpt_path"):
        ap.add_argument("--" + key)
    for key in ("batch_size", "sample_rate", "epochs", "continue_train", "device_num"):
        ap.add_argument("--" + key, type=int)
    for key in ("segment", "l2", "momentum"):
        ap.add_argument("--" + key, type=float)
    args = ap.parse_args(argv)
    overrides = {k: v for k, v in vars(args).items() if k != "config_path"}
    return train(load_config(args.config_path, overrides))


if __name__ == "__main__":
    main()
