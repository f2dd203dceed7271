"""ECAPA training-data generation on the device: generate_train_data() / generate_npy() of
examples/ECAPA-TDNN/train_speaker_embeddings.py (530-729).

    python -m mindaudio_amd.ecapa.generate_train_data --config_path ecapatdnn.yaml

Every batch of `batch_size` chunks of `sentence_len` seconds goes through the five time-domain augmenters (two
TimeDomainSpecAugment, three EnvCorrupt); the clean batch and the five versions - each computed from the ORIGINAL batch and cut or
zero-padded to its length - form one ((1 + 5) B, N) matrix, which becomes 80-mel fbanks (n_fft 400, hop 160), transposed to
(rows, frames, 80) and sentence-mean-normalised.  The waveforms never leave the device between the upload of the clean batch and
the download of the features for the .npy write: every augmenter writes straight into its slice of the matrix the fbank reads.

Reads the yaml keys of the example (train_annotation, feat_folder, data_folder, sample_rate, sentence_len, random_chunk,
number_of_epochs, concat_augment, dataloader_options.batch_size); writes <stamp>_<index>_fea.npy ((1 + 5) B, frames, 80) float32,
<stamp>_<index>_id.npy ((1 + 5) B, 1) - the batch's speaker ids, numbered in order of first appearance in the annotation and
repeated once per version - and the sorted fea.lst / label.lst into feat_folder.

Out of scope: prepare_voxceleb and the download of the verification list (network, data set: `train_annotation` must exist, with
the columns ID,duration,wav,start,stop,spk_id); the Manager / Process fan-out over `data_process_num` CPU processes (one process,
one GPU: the annotation is read in file order, without the example's shuffling MindSpore CSVDataset).  data_trans_dp (the
concatenation of these files into feat_folder_merge - its inputs are exactly the files and lists written here) is in
ecapa/train_speaker_embeddings.py."""
import argparse
import csv
import datetime
import os
import random

import numpy as np

from .spec_augment import EnvCorrupt, TimeDomainSpecAugment

__all__ = ["augment_batch", "read_annotation", "load_chunk", "iter_batches", "default_augmenters", "generate_npy",
           "generate_train_data", "main"]


def augment_batch(wavs, spec_aug, concat_augment=True):
    """The body of generate_npy for one batch: wavs (B, N) float32 (device tensor or NumPy) -> (rows, frames, 80) float32 device
    tensor, rows = (1 + len(spec_aug)) B with concat_augment (the clean batch first, then one block per augmenter, each computed
    from the clean batch), else B (the augmenters applied one after the other)."""
    import torch

    from .. import ops
    from ..data.features import fbank

    x = torch.as_tensor(np.ascontiguousarray(wavs) if isinstance(wavs, np.ndarray) else wavs).to(device="cuda", dtype=torch.float32)
    if x.dim() != 2:
        raise ValueError("wavs must be [batch, time]")
    b, n = x.shape
    lens = np.ones(b)
    if concat_augment:
        mat = torch.empty(((1 + len(spec_aug)) * b, n), dtype=torch.float32, device=x.device)
        mat[:b].copy_(x)
        for k, aug in enumerate(spec_aug):
            aug.construct(x, lens, out=mat[(k + 1) * b:(k + 2) * b])
    else:
        mat = x
        for aug in spec_aug:
            mat = aug.construct(mat, lens, out=torch.empty((b, n), dtype=torch.float32, device=x.device))
    feats = fbank(mat, deltas=False, n_mels=80, left_frames=0, right_frames=0, n_fft=400, hop_length=160)
    return ops.sentence_mean_norm(feats.transpose(1, 2).contiguous())


def read_annotation(path):
    """(rows, spk_id_encoded_dict): the rows of the annotation csv as dicts, and the speaker ids numbered in order of appearance."""
    with open(path, newline="") as fh:
        rows = [row for row in csv.DictReader(fh, skipinitialspace=True) if row.get("wav")]
    spk = {}
    for row in rows:
        spk.setdefault(str(row["spk_id"]), len(spk))
    return rows, spk


def load_chunk(row, sample_rate, sentence_len, random_chunk):
    """audio_pipeline of dataio_prep (52-65): a random chunk of sentence_len seconds (`random.randint` on the global generator), or
    samples start..stop; stereo averaged to mono."""
    from ..data.io import read

    snt_len_sample = int(sample_rate * sentence_len)
    if random_chunk:
        duration_sample = int(float(row["duration"]) * sample_rate)
        start = random.randint(0, duration_sample - snt_len_sample)
        stop = start + snt_len_sample
    else:
        start, stop = int(float(row["start"])), int(float(row["stop"]))
    sig, _ = read(str(row["wav"]))
    sig = np.asarray(sig)
    if sig.ndim > 1:
        sig = sig.mean(axis=-1)
    return sig[start:stop]


def iter_batches(rows, spk, batch_size, sample_rate=16000, sentence_len=3.0, random_chunk=True):
    """(wavs (b, N) float32, ids (b,) int) per batch of the annotation, the last one short (the example's batch() keeps it)."""
    for b0 in range(0, len(rows), batch_size):
        part = rows[b0:b0 + batch_size]
        sigs = [load_chunk(r, sample_rate, sentence_len, random_chunk) for r in part]
        yield np.stack(sigs).astype(np.float32), np.array([spk[str(r["spk_id"])] for r in part])


def default_augmenters(data_folder):
    """The five augmenters generate_train_data builds (654-681)."""
    env = dict(openrir_folder=data_folder, openrir_max_noise_len=3.0, noise_snr_low=0, noise_snr_high=15)
    return [TimeDomainSpecAugment(sample_rate=16000, speeds=[100]), TimeDomainSpecAugment(sample_rate=16000, speeds=[95, 100, 105]),
            EnvCorrupt(reverb_prob=1.0, noise_prob=0.0, **env), EnvCorrupt(reverb_prob=0.0, noise_prob=1.0, **env),
            EnvCorrupt(reverb_prob=1.0, noise_prob=1.0, **env)]


def generate_npy(batches, spec_aug, save_dir, index=0, concat_augment=True, batch_counts=None, log=print, featurize=None):
    """One .npy pair per batch of `batches` ((wavs, ids) pairs); returns (label file names, feature file names).  `featurize`
    stands in for augment_batch (tests without a device)."""
    featurize = featurize or augment_batch
    label_fp_list, fea_fp_list = [], []
    last = None
    for count, (wavs, ids) in enumerate(batches, 1):
        feats = featurize(wavs, spec_aug, concat_augment)
        feats = feats.cpu().numpy() if hasattr(feats, "cpu") else np.asarray(feats)
        n_augment = feats.shape[0] // len(ids)
        stamp = datetime.datetime.now().timestamp()
        if last is not None and stamp <= last:  # two batches within the clock's resolution must not share a file
            stamp = float(np.nextafter(last, np.inf))
        last = stamp
        id_save_name = str(stamp) + "_" + str(index) + "_id.npy"
        fea_save_name = str(stamp) + "_" + str(index) + "_fea.npy"
        spkid = np.concatenate([[np.asarray(ids)]] * n_augment).reshape(-1, 1)
        np.save(os.path.join(save_dir, id_save_name), spkid)
        np.save(os.path.join(save_dir, fea_save_name), feats)
        label_fp_list.append(id_save_name)
        fea_fp_list.append(fea_save_name)
        if batch_counts:
            log("Process {} percentage {}%".format(index, round(float(count) / batch_counts * 100, 2)))
    return label_fp_list, fea_fp_list


def generate_train_data(cfg, spec_aug=None, log=print, featurize=None):
    """generate_train_data of the example on a config mapping; returns (label file names, feature file names) as written to
    label.lst / fea.lst.  `spec_aug`: the augmenters instead of default_augmenters(cfg["data_folder"])."""
    log("Generate train data.")
    save_dir = str(cfg["feat_folder"])
    os.makedirs(save_dir, exist_ok=True)
    rows, spk = read_annotation(str(cfg["train_annotation"]))
    log("spk_id_encoded_dict len = %d" % len(spk))
    if spec_aug is None:
        spec_aug = default_augmenters(cfg.get("data_folder"))
    opts = cfg.get("dataloader_options") or {}
    batch_size = int(opts.get("batch_size", 32))
    epochs = int(cfg.get("number_of_epochs", 1))
    log("len of train: %d" % len(rows))
    batch_counts = len(rows) / batch_size * epochs
    labels, feas = [], []
    for _ in range(epochs):
        batches = iter_batches(rows, spk, batch_size, int(cfg.get("sample_rate", 16000)), float(cfg.get("sentence_len", 3.0)),
                               bool(cfg.get("random_chunk", True)))
        lab, fea = generate_npy(batches, spec_aug, save_dir, 0, bool(cfg.get("concat_augment", True)), batch_counts, log, featurize)
        labels += lab
        feas += fea
    labels.sort()
    feas.sort()
    with open(os.path.join(save_dir, "label.lst"), "w") as fh:
        fh.writelines(name + "\n" for name in labels)
    with open(os.path.join(save_dir, "fea.lst"), "w") as fh:
        fh.writelines(name + "\n" for name in feas)
    return labels, feas


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    for key in ("train_annotation", "feat_folder", "data_folder"):
        ap.add_argument("--" + key)
    a = ap.parse_args(argv)
    over = {k: v for k, v in vars(a).items() if k != "config_path" and v is not None}
    return generate_train_data(load_config(a.config_path, over))


if __name__ == "__main__":
    main()
