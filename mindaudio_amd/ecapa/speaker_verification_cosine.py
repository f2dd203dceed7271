"""Speaker verification by cosine distance - mirror of examples/ECAPA-TDNN/speaker_verification_cosine.py on MI355X.

    python -m mindaudio_amd.ecapa.speaker_verification_cosine --config_path ecapatdnn.yaml

reads the example's yaml keys (in_channels, channels, emb_size, model_path, eval_data_path, train_norm_path, veri_file_path,
score_norm, cohort_size, cut_wav, n_train_snts, npy_file_path; plus `excluded_set` and `embed_batch_size`, see below) and prints the three equal error rates the example prints:
baseline, with mean subtraction, with score normalisation.

What runs where: fbank + sentence mean normalisation, the embedding model, the running-mean subtraction, the cohort statistics
(one exact-float32 matrix product of the distinct trial utterances against the cohort + an exact top-K selection per row, instead
of the example's two cosine_similarity + np.partition calls per trial) and the trial scores are HIP kernels; embeddings stay on
the device between the stages.  File parsing and the equal error rates (metric/eer.py) are host code.

Differences from the example, all deliberate:
  * its hard-coded `excluded_set` (indices of bad utterances of ONE feature dump) is data: the `excluded_set` yaml key /
    parameter, empty by default;
  * downloading the trial list and voxceleb_prepare are not here (they need the network and the dataset);
  * an unknown `score_norm` raises ValueError (the example silently scores without normalisation);
  * the cohort embeddings are cached under npy_file_path as one .npz per 50 000 utterances (names + matrix), not as pickled dicts,
    and any number of chunks is read back (the example reads exactly six);
  * utterances with the same frame count are embedded as one batch of up to `embed_batch_size` (default 16; the model ignores
    `lengths`, so nothing is ever padded).
"""
import argparse
import csv
import datetime
import os

import numpy as np

from ..metric.eer import EER, get_eer_from_scores

__all__ = ["compute_feat_loop", "DatasetGenerator", "EmbeddingTable", "compute_embeddings", "emb_mean", "parse_trials",
           "validate_scoring", "evaluate", "evaluate2", "eval_impl", "main"]

SCORE_NORMS = ("z-norm", "t-norm", "s-norm")


def compute_feat_loop(csv_file, save_dir, sample_rate=16000, num_samples=None, log=print):
    """fbank (80 mels, n_fft 400, hop 160) + sentence mean normalisation of every `ID, wav, start, stop` row of `csv_file`
    (samples start..stop of the file, stereo averaged to mono), one utterance per batch as the example's eval_batch_size: 1.
    Writes the example's folder: <stamp>_fea_mvn.npy (1, frames, 80) float32, <stamp>_label.npy [ID], fea.lst, label.lst."""
    import torch

    from .. import ops
    from ..data.features import fbank
    from ..data.io import read

    log("compute_feat_loop")
    os.makedirs(save_dir, exist_ok=True)
    last = None
    with open(csv_file, newline="") as fh, open(os.path.join(save_dir, "fea.lst"), "w") as fea_fp, \
            open(os.path.join(save_dir, "label.lst"), "w") as label_fp:
        for n, row in enumerate(csv.DictReader(fh, skipinitialspace=True)):
            if num_samples is not None and n >= num_samples:
                break
            start, stop = int(float(row["start"])), int(float(row["stop"]))
            sig, _ = read(str(row["wav"]), duration=float(stop - start) / sample_rate, offset=float(start) / sample_rate)
            sig = np.asarray(sig)
            if sig.ndim > 1:
                sig = sig.mean(axis=-1)
            wav = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32)[None]).cuda()
            feats = fbank(wav, deltas=False, n_mels=80, left_frames=0, right_frames=0, n_fft=400, hop_length=160)
            feats = ops.sentence_mean_norm(feats.transpose(1, 2).contiguous())
            stamp = datetime.datetime.now().timestamp()
            if last is not None and stamp <= last:  # two utterances within the clock's resolution must not share a file
                stamp = np.nextafter(last, np.inf)
            last = stamp
            fea_name, label_name = "%r_fea_mvn.npy" % float(stamp), "%r_label.npy" % float(stamp)
            np.save(os.path.join(save_dir, fea_name), feats.cpu().numpy())
            np.save(os.path.join(save_dir, label_name), np.array([str(row["ID"])]))
            fea_fp.write(fea_name + "\n")
            label_fp.write(label_name + "\n")


class DatasetGenerator:
    """reader.py::DatasetGenerator: the (features, label) files fea.lst / label.lst name; `drop` leaves the last one out."""

    def __init__(self, data_dir, drop=True, log=None):
        self.data, self.label = [], []
        with open(os.path.join(data_dir, "fea.lst"), "r") as fp:
            for line in fp:
                self.data.append(os.path.join(data_dir, line.strip()))
        with open(os.path.join(data_dir, "label.lst"), "r") as fp:
            for line in fp:
                self.label.append(os.path.join(data_dir, line.strip()))
        if drop:
            self.data.pop()
            self.label.pop()
        if log is not None:
            log("dataset init ok, total len: %d" % len(self.data))

    def __getitem__(self, index):
        return np.load(self.data[index]), np.load(self.label[index]).tolist()[0]

    def __len__(self):
        return len(self.data)


class EmbeddingTable:
    """The example's {utterance: embedding} dict with the embeddings as ONE device matrix: names[i] <-> emb[i]."""

    def __init__(self, names, emb):
        self.names = list(names)
        self.emb = emb
        self.index = {n: i for i, n in enumerate(self.names)}
        if len(self.index) != len(self.names) or len(self.names) != emb.shape[0]:
            raise ValueError("an embedding table needs one distinct name per row")

    def __len__(self):
        return len(self.names)

    def __getitem__(self, name):
        return self.emb[self.index[name]]


def compute_embeddings(embedder, dataset, startidx=0, dur=50000, exc_set=None, cut_wav=False, batch_size=16, log=print):
    """Embeddings of dataset[startidx : startidx + dur] minus the indices in exc_set, as an EmbeddingTable on the device.
    cut_wav keeps the first 301 frames.  Utterances of equal frame count are embedded together, `batch_size` at a time."""
    import torch

    embedder.eval()
    log("Compute embeddings, num to process: %d" % len(dataset))
    names, feats = [], []
    for index in range(startidx, startidx + dur):
        if index >= len(dataset):
            log("exceed data size")
            break
        if exc_set is not None and index in exc_set:
            continue
        data, label = dataset[index]
        if data.ndim != 3 or data.shape[0] != 1:
            raise ValueError("feature file %d holds %s: one (1, frames, mels) utterance per file is expected" % (index, data.shape))
        if cut_wav:
            data = data[:, :301, :]
        if index % 1000 == 0:
            log("%s, iter-%d" % (datetime.datetime.now(), index))
        names.append(label)
        feats.append(data)
    # the example's dict: a repeated name keeps its first position and its last value
    slot, order = {}, []
    for i, n in enumerate(names):
        if n not in slot:
            order.append(n)
        slot[n] = i
    keep = [slot[n] for n in order]
    by_len = {}
    for row, i in enumerate(keep):
        by_len.setdefault(feats[i].shape[1], []).append((row, i))
    dev = next(embedder.parameters()).device
    emb = None
    for frames in sorted(by_len):
        group = by_len[frames]
        for g0 in range(0, len(group), batch_size):
            part = group[g0:g0 + batch_size]
            x = torch.from_numpy(np.concatenate([feats[i] for _, i in part]).astype(np.float32)).to(dev)
            e = embedder(x).reshape(len(part), -1).float()
            if emb is None:
                emb = torch.empty((len(keep), e.shape[1]), dtype=torch.float32, device=dev)
            emb[torch.tensor([r for r, _ in part], device=dev)] = e
    if emb is None:
        raise ValueError("no utterance to embed")
    return EmbeddingTable(order, emb)


def emb_mean(g_mean, increment, table):
    """The example's emb_mean: every embedding minus the running mean up to and including it; returns (table of the differences,
    running mean (float64 device vector), count).  At increment 0 the incoming g_mean is ignored, as in the example."""
    from .. import ops

    y, g, cnt = ops.running_mean_sub(table.emb, g_mean if increment else None, increment)
    return EmbeddingTable(table.names, y), g, cnt


def parse_trials(trials, spk_index, utt_index):
    """`label enrol.wav test.wav` lines -> (labels, enrol rows, test rows); the last four characters of both names are dropped."""
    labels, enrol, test = [], [], []
    with open(trials, "r") as f:
        for trial in f:
            trial = trial.strip()
            label, spk, tst = trial.split(" ")
            labels.append(1 if label == "1" else 0)
            enrol.append(spk_index[spk[:-4]])
            test.append(utt_index[tst[:-4]])
    return np.asarray(labels, np.int64), np.asarray(enrol, np.int64), np.asarray(test, np.int64)


def validate_scoring(score_norm, cohort_size, n_cohort):
    """ValueError for a score_norm the example does not know or a cohort_size above the cohort (np.partition's error there)."""
    if score_norm is not None and score_norm not in SCORE_NORMS:
        raise ValueError("unknown score_norm %r: one of %s" % (score_norm, ", ".join(SCORE_NORMS)))
    if cohort_size is not None and n_cohort is not None:
        if int(cohort_size) < 1 or int(cohort_size) > int(n_cohort):
            raise ValueError("cohort_size %d is not within the cohort of %d embeddings" % (int(cohort_size), int(n_cohort)))


def _joint(spk2emb, utt2emb):
    import torch

    if spk2emb is utt2emb:
        return spk2emb.emb, 0
    return torch.cat((spk2emb.emb, utt2emb.emb)), len(spk2emb)


def _trial_scores(spk2emb, utt2emb, trials, norm_cohort=None, score_norm=None, cohort_size=None):
    import torch

    from .. import ops

    labels, enrol, test = parse_trials(trials, spk2emb.index, utt2emb.index)
    emb, off = _joint(spk2emb, utt2emb)
    test = test + off
    mean = std = None
    if score_norm is not None:
        used = np.unique(np.concatenate((enrol, test)))  # only the utterances the trials name are scored against the cohort
        um, us = ops.cohort_stats(emb[torch.from_numpy(used).to(emb.device)], norm_cohort, cohort_size)
        mean = torch.zeros((emb.shape[0],), dtype=torch.float64, device=emb.device)
        std = torch.ones((emb.shape[0],), dtype=torch.float64, device=emb.device)
        mean[torch.from_numpy(used).to(emb.device)] = um
        std[torch.from_numpy(used).to(emb.device)] = us
    scores = ops.trial_scores(emb, enrol, test, mean, std, score_norm)
    return scores.cpu().numpy(), labels


def evaluate(spk2emb, utt2emb, trials):
    """Equal error rate (get_eer_from_scores) of the plain cosine scores of the trial file."""
    scores, labels = _trial_scores(spk2emb, utt2emb, trials)
    return get_eer_from_scores(scores, labels)[0]


def evaluate2(spk2emb, utt2emb, norm_dict, params, trials, log=print):
    """(positive scores, negative scores) of the trial file, float64 arrays in file order.  norm_dict: the cohort (N, D) device
    matrix or None; params: a mapping with optional `score_norm` (z-norm / t-norm / s-norm) and `cohort_size`."""
    score_norm, cohort_size = params.get("score_norm"), params.get("cohort_size")
    if norm_dict is None:
        validate_scoring(score_norm, None, None)
        if score_norm is not None:
            raise ValueError("score_norm %r needs a cohort" % (score_norm,))
    else:
        validate_scoring(score_norm, cohort_size, norm_dict.shape[0])
        log("train_cohort shape: %s" % (tuple(norm_dict.shape),))
    scores, labels = _trial_scores(spk2emb, utt2emb, trials, norm_dict, score_norm, cohort_size)
    return scores[labels == 1], scores[labels == 0]


def _cohort_embeddings(model, cfg, log):
    """Embeddings of the normalisation set, 50 000 utterances per cached file under npy_file_path."""
    import torch

    dataset_train = DatasetGenerator(cfg["train_norm_path"], False, log)
    n = len(dataset_train)
    if cfg.get("n_train_snts") is not None:
        n = min(n, int(cfg["n_train_snts"]))
    log("steps_per_epoch_train: %d" % n)
    names, parts = [], []
    dev = next(model.parameters()).device
    for start in range(0, n, 50000):
        end = min(start + 50000, n)
        log("start end: %d %d" % (start, end))
        fpath = os.path.join(cfg["npy_file_path"], "train_dict_%d_%d.npz" % (start, end))
        if os.path.isfile(fpath):
            log("find cache file:%s, continue" % fpath)
            with np.load(fpath) as z:
                names += [str(s) for s in z["names"]]
                parts.append(torch.from_numpy(z["emb"]).to(dev))
            continue
        table = compute_embeddings(model, dataset_train, startidx=start, dur=end - start, cut_wav=bool(cfg.get("cut_wav")),
                                   batch_size=int(cfg.get("embed_batch_size", 16)), log=log)
        np.savez(fpath, names=np.array(table.names), emb=table.emb.cpu().numpy())
        names += table.names
        parts.append(table.emb)
    slot = {}
    for i, nm in enumerate(names):  # dict.update across the chunks: first position, last value
        slot[nm] = i
    order = list(dict.fromkeys(names))
    emb = torch.cat(parts)
    if len(order) != len(names):
        emb = emb[torch.tensor([slot[nm] for nm in order], device=dev)]
    log("norm data len: %d" % len(order))
    return EmbeddingTable(order, emb)


def eval_impl(cfg, log=print, model=None, details=None):
    """The example's eval_impl on a config mapping; returns (eer baseline, eer with sub mean, EER with norm or None when
    score_norm is absent or cut_wav is set).  `model`: an EcapaTDNN on the device instead of cfg["model_path"].  `details`: a dict
    that receives the embedding tables and the normalised positive / negative scores."""
    import torch

    from ..models import EcapaTDNN
    from ..utils.ckpt import load_mindspore_checkpoint

    validate_scoring(cfg.get("score_norm"), None, None)
    if model is None:
        channels = int(cfg["channels"])
        model = EcapaTDNN(int(cfg["in_channels"]), channels=(channels, channels, channels, channels, channels * 3),
                          lin_neurons=int(cfg["emb_size"]))
        log(str(cfg["model_path"]))
        load_mindspore_checkpoint(model, str(cfg["model_path"]))
        model = model.to(torch.device("cuda", torch.cuda.current_device()))
    model.eval()
    dataset_enroll = DatasetGenerator(cfg["eval_data_path"], False, log)
    log("size of enroll, test: %d" % len(dataset_enroll))
    veri_file_path = cfg["veri_file_path"]
    os.makedirs(cfg["npy_file_path"], exist_ok=True)
    cut_wav = bool(cfg.get("cut_wav"))
    enroll = compute_embeddings(model, dataset_enroll, dur=len(dataset_enroll), exc_set=set(cfg.get("excluded_set") or ()),
                                cut_wav=cut_wav, batch_size=int(cfg.get("embed_batch_size", 16)), log=log)
    eer_base = evaluate(enroll, enroll, veri_file_path)
    log("eer baseline: %s" % eer_base)

    log("Sub mean...")
    glob_mean, cnt = None, 0
    for _ in range(3):
        enroll_mean, glob_mean, cnt = emb_mean(glob_mean, cnt, enroll)
    eer_mean = evaluate(enroll_mean, enroll_mean, veri_file_path)
    log("eer with sub mean: %s" % eer_mean)
    if details is not None:
        details.update(enroll=enroll, enroll_mean=enroll_mean)

    eer_norm = None
    if cfg.get("score_norm") is not None and cfg.get("cut_wav") is not True:
        train = _cohort_embeddings(model, cfg, log)
        validate_scoring(cfg.get("score_norm"), cfg.get("cohort_size"), len(train))
        train_mean, glob_mean, cnt = emb_mean(glob_mean, cnt, train)
        pos, neg = evaluate2(enroll_mean, enroll_mean, train_mean.emb, cfg, veri_file_path, log)
        eer_norm = EER(pos, neg)
        log("EER with norm: %s" % eer_norm)
        if details is not None:
            details.update(train=train, train_mean=train_mean, pos=pos, neg=neg)
    return eer_base, eer_mean, eer_norm


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    for key in ("model_path", "eval_data_path", "train_norm_path", "veri_file_path", "score_norm", "npy_file_path"):
        ap.add_argument("--" + key)
    for key in ("in_channels", "channels", "emb_size", "cohort_size", "n_train_snts"):
        ap.add_argument("--" + key, type=int)
    a = ap.parse_args(argv)
    over = {k: v for k, v in vars(a).items() if k != "config_path" and v is not None}
    return eval_impl(load_config(a.config_path, over))


if __name__ == "__main__":
    main()
