"""`python -m mindaudio_amd.deepspeech2.train --config_path deepspeech2.yaml` - the counterpart of examples/deepspeech2/train.py.

Reads the example's yaml keys: TrainingConfig (epochs, batch_size, train_manifest), SpectConfig, ModelConfig (rnn_type, hidden_size,
hidden_layers), OptimConfig (learning_rate, epsilon, loss_scale), CheckpointConfig (ckpt_file_name_prefix, ckpt_path,
keep_checkpoint_max), Pretrained_model and labels.  The bins of ASRTrainDataset are walked in order (the reference shuffles them
through a DistributedSampler, which is not built); every step prints LossMonitor's line `epoch: E step: S, loss is L`; a checkpoint in
the reference's wire format is written every SAVE_CHECKPOINT_STEPS = 5 steps as <prefix>-<epoch>_<step in epoch>.ckpt, and only the
newest keep_checkpoint_max of them stay.  A checkpoint holds the model's parameters under the reference's names plus the trainer's
`moment1.*` / `moment2.*` and Adam's `global_step`; `Pretrained_model` may be a checkpoint of either kind.

What the reference's script does and this keeps (models.DeepSpeech2Trainer has the details): the loss scale is the constant 1024,
Adam divides the unscaled gradient by OptimConfig.loss_scale a second time, step_lr is computed and never used - the rate is constant -
and OptimConfig's weight_decay, momentum, eps, betas and learning_anneal are never read (epsilon is Adam's eps).
The convolution front end is frozen unless `--frontend trained` is given (train(config, frontend="trained")): conv1, conv2 and both
BatchNorm2d are then trained as the reference trains them, and a checkpoint also holds `moment1.conv.*` / `moment2.conv.*`, which a
later `--frontend trained` run restores.  `--is_distributed` raises NotImplementedError."""
import argparse
import os
import time

import numpy as np

SAVE_CHECKPOINT_STEPS = 5  # train.py:80
LOSS_SCALE = 1024          # train.py:64: Tensor(1024)


def settings(config):
    """The yaml's values that training reads, as plain Python values."""
    t, m, o, c = config["TrainingConfig"], config["ModelConfig"], config["OptimConfig"], config["CheckpointConfig"]
    return dict(epochs=int(t["epochs"]), batch_size=int(t["batch_size"]), train_manifest=str(t["train_manifest"]),
                rnn_type=str(m["rnn_type"]), hidden_size=int(m["hidden_size"]), hidden_layers=int(m["hidden_layers"]),
                learning_rate=float(o["learning_rate"]), epsilon=float(o["epsilon"]), optimizer_loss_scale=float(o["loss_scale"]),
                prefix=str(c["ckpt_file_name_prefix"]), ckpt_path=str(c["ckpt_path"]), keep_checkpoint_max=int(c["keep_checkpoint_max"]),
                pretrained=str(config.get("Pretrained_model") or ""), labels=list(config["labels"]), spect=config["SpectConfig"])


class Checkpoints:
    """ModelCheckpoint(prefix, directory, CheckpointConfig(save_checkpoint_steps, keep_checkpoint_max)): after_step() writes
    <directory>/<prefix>-<epoch>_<step in epoch>.ckpt when the global step count is a multiple of `every`, then removes the oldest files
    it wrote until at most keep_max are left."""

    def __init__(self, trainer, directory, prefix, keep_max, every=SAVE_CHECKPOINT_STEPS):
        self.trainer, self.directory, self.prefix, self.keep_max, self.every = trainer, directory, prefix, max(1, int(keep_max)), every
        self.written = []

    def after_step(self, global_step, epoch, step_in_epoch):
        """global_step counts from 1 -> the path written, or None"""
        if global_step % self.every:
            return None
        from ..utils import ckpt

        os.makedirs(self.directory, exist_ok=True)
        path = os.path.join(self.directory, "%s-%d_%d.ckpt" % (self.prefix, epoch, step_in_epoch))
        state = self.trainer.state_dict()
        out = ckpt.deepspeech2_to_reference_names({k: v for k, v in state.items() if k != "steps"})
        out["global_step"] = np.array([int(state["steps"])], np.int32)  # Adam's step count (nn.Adam keeps it under this name)
        ckpt.write_mindspore_ckpt(path, out)
        self.written.append(path)
        while len(self.written) > self.keep_max:
            old = self.written.pop(0)
            if os.path.exists(old):
                os.remove(old)
        return path


def restore(trainer, path):
    """A MindSpore checkpoint of the model, or one of this script's (with the moments), into the trainer."""
    from ..utils import ckpt

    raw = ckpt.read_mindspore_ckpt(path)
    moments = {k: v for k, v in raw.items() if k.startswith(("moment1.", "moment2."))}
    params = ckpt.convert_deepspeech2_names({k: v for k, v in raw.items() if k not in moments})
    trainer.model.load_weights(params)
    if moments:
        steps = int(np.asarray(raw.get("global_step", 0)).reshape(-1)[0])
        trainer.load_state_dict(dict(trainer.model.state_dict(), steps=steps, **moments))


def train(config, is_distributed=False, log=print, max_steps=None, frontend="frozen", save_checkpoint_steps=SAVE_CHECKPOINT_STEPS):
    """train.py:26-96 on a config mapping; returns the list of per-step losses.  frontend: models.DeepSpeech2Trainer's;
    save_checkpoint_steps: the reference's constant 5 unless a caller (a short run, a test) asks for another interval."""
    if is_distributed:
        raise NotImplementedError("--is_distributed: multi-GPU DeepSpeech2 training is not built")
    s = settings(config)
    from .. import _host
    from ..models import DeepSpeech2Trainer, DeepSpeechModel
    from .dataset import ASRTrainDataset

    _host.require_gpu()
    dataset = ASRTrainDataset(audio_conf=s["spect"], manifest_filepath=s["train_manifest"], labels=s["labels"], normalize=True,
                              batch_size=s["batch_size"], log=log)
    model = DeepSpeechModel(batch_size=s["batch_size"], rnn_hidden_size=s["hidden_size"], nb_layers=s["hidden_layers"], labels=s["labels"],
                            rnn_type=s["rnn_type"], audio_conf=s["spect"], bidirectional=True).cuda()
    trainer = DeepSpeech2Trainer(model, s["learning_rate"], s["epsilon"], loss_scale=LOSS_SCALE, optimizer_loss_scale=s["optimizer_loss_scale"],
                                 frontend=frontend)
    if s["pretrained"]:
        restore(trainer, s["pretrained"])
        log("Successfully loading the pre-trained model")
    saver = Checkpoints(trainer, s["ckpt_path"], s["prefix"], s["keep_checkpoint_max"], every=save_checkpoint_steps)
    losses, global_step = [], 0
    for epoch in range(1, s["epochs"] + 1):
        for i in range(len(dataset)):
            inputs, input_length, targets, target_lengths = dataset[i]
            t0 = time.time()
            loss, overflow = trainer.step(inputs, input_length, targets, target_lengths)
            global_step += 1
            losses.append(loss)
            log("epoch: %d step: %d, loss is %s%s (%.3f s)" % (epoch, i + 1, loss, ", overflow: update skipped" if overflow else "",
                                                            time.time() - t0))
            saver.after_step(global_step, epoch, i + 1)
            if max_steps is not None and global_step >= max_steps:
                return losses
    return losses


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    ap.add_argument("--Pretrained_model")
    ap.add_argument("--is_distributed", action="store_true")
    ap.add_argument("--frontend", choices=("frozen", "trained"), default="frozen", help="train the convolution front end as well")
    a = ap.parse_args(argv)
    return train(load_config(a.config_path, {"Pretrained_model": a.Pretrained_model}), is_distributed=a.is_distributed, frontend=a.frontend)


if __name__ == "__main__":
    main()
