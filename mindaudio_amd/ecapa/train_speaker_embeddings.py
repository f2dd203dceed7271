"""Training side of examples/ECAPA-TDNN (train_speaker_embeddings.py, reader.py, sampler.py), restricted to the speaker-classification
head: the merged-feature writer and reader, the sampler, the cyclic learning rate and a one-step trainer for the cosine classifier
under AAM-softmax, all device work in the kernels of csrc/aam_softmax.hip and the engine's overflow check / Adam.

    python -m mindaudio_amd.ecapa.train_speaker_embeddings --config_path ecapatdnn.yaml

The embedding network's backward and train-mode BatchNorm are not built, so `train` needs `freeze_embedding_model: true` in the yaml:
the (pre-trained) EcapaTDNN stays in eval mode and only `classifier.weight` is trained on its embeddings.

Kept from the reference: the accuracy is counted on the margin-penalised output; the learning rate of step i is lr_list[i]; Adam with
weight decay folded into the gradient, a fixed loss scale of 2**14 and the overflow check of TrainOneStepWithLossScaleCell; the file
layout of data_trans_dp (`<k>.npy`, `<k>_label.npy`, ind_sample.p, ind_label.p) and the batch order of DatasetGeneratorBatch.
Different on purpose: data_trans_dp runs in one process and raises on a label / feature row-count mismatch (the reference prints and
stops that shard); Adam's bias correction counts the calls of step(), skipped steps included, so that no step reads the overflow flag
back (MindSpore's counter stands still on a skipped step).  Not verified: the name MindSpore would give the classifier weight inside
its TrainOneStepWithLossScaleCell checkpoint - the file written here stores it as `classifier.weight`."""
import argparse
import datetime
import math
import os
import pickle
import time

import numpy as np

__all__ = ["learning_rate_clr_triangle_function", "update_average", "data_trans_dp", "DatasetGeneratorBatch", "DistributedSampler",
           "SpeakerHeadTrainer", "train", "main"]


def learning_rate_clr_triangle_function(step_size, max_lr, base_lr, clr_iterations):
    """Triangular cyclic learning rate (arXiv:1506.01186) at iteration `clr_iterations`: base_lr at multiples of 2 * step_size,
    max_lr half-way between them."""
    cycle = math.floor(1 + clr_iterations / (2 * step_size))
    x = abs(clr_iterations / step_size - 2 * cycle + 1)
    return base_lr + (max_lr - base_lr) * max(0, 1 - x)


def update_average(loss_, avg_loss, step):
    """Running mean of the losses: avg <- avg - avg / step + loss / step."""
    return avg_loss - avg_loss / step + loss_ / step


def _read_list(folder, name):
    with open(os.path.join(folder, name)) as fh:
        return [os.path.join(folder, line.strip()) for line in fh if line.strip()]


def data_trans_dp(datasetPath, dataSavePath, samples_per_file=4000, epoch_len=73357, log=print):
    """Merge the per-batch files generate_train_data wrote (fea.lst / label.lst in `datasetPath`) into files of `samples_per_file`
    batches each: `<k>.npy` the flattened features one after the other, `<k>_label.npy` the labels, and two pickled dictionaries
    ind_sample.p / ind_label.p {feature file base name: (k, offset, length)} into those flat arrays.  Every entry whose 1-based
    position is a multiple of `epoch_len` is left out, as in the reference (the short last batch of each generated epoch)."""
    os.makedirs(dataSavePath, exist_ok=True)
    feas, labels = _read_list(datasetPath, "fea.lst"), _read_list(datasetPath, "label.lst")
    log("total length of fea, label: %d %d" % (len(feas), len(labels)))
    if len(feas) != len(labels):
        raise ValueError("fea.lst and label.lst differ in length: %d, %d" % (len(feas), len(labels)))
    kept = [(f, l) for idx, (f, l) in enumerate(zip(feas, labels)) if (idx + 1) % epoch_len != 0]
    samples_dict, labels_dict = {}, {}
    for file_ind, start in enumerate(range(0, len(kept), samples_per_file)):
        fea_parts, label_parts = [], []
        offset = offset_label = 0
        for fea_path, label_path in kept[start:start + samples_per_file]:
            fea, label = np.load(fea_path), np.load(label_path)
            if label.shape[0] != fea.shape[0]:
                raise ValueError("%s holds %d rows, %s %d" % (label_path, label.shape[0], fea_path, fea.shape[0]))
            flat, ids = fea.reshape(-1), label.reshape(-1)
            utt = os.path.basename(fea_path)
            samples_dict[utt] = (file_ind, offset, flat.shape[0])
            labels_dict[utt] = (file_ind, offset_label, ids.shape[0])
            fea_parts.append(flat)
            label_parts.append(ids)
            offset += flat.shape[0]
            offset_label += ids.shape[0]
        np.save(os.path.join(dataSavePath, "%d_label.npy" % file_ind), np.hstack(label_parts))
        np.save(os.path.join(dataSavePath, "%d.npy" % file_ind), np.hstack(fea_parts))
        log("process %d done" % file_ind)
    with open(os.path.join(dataSavePath, "ind_sample.p"), "wb") as fh:
        pickle.dump(samples_dict, fh)
    with open(os.path.join(dataSavePath, "ind_label.p"), "wb") as fh:
        pickle.dump(labels_dict, fh)
    return samples_dict, labels_dict


class DatasetGeneratorBatch:
    """reader.py's DatasetGeneratorBatch over one or several folders written by data_trans_dp: item i is (features (-1, 301, 80),
    labels) of the i-th batch, the batches of each folder in sorted-name order; the merged files are memory-mapped on first use and
    re-opened every `read_limit` reads."""

    def __init__(self, data_paths, read_limit=5000000):
        self.batchlist = []
        self.index_sample, self.index_label = {}, {}
        self.memmaps_sample, self.memmaps_label = {}, {}
        self.reads = 0
        self.read_limit = read_limit
        for data_path in [data_paths] if isinstance(data_paths, str) else data_paths:
            with open(os.path.join(data_path, "ind_sample.p"), "rb") as fh:
                sample_index = pickle.load(fh)
            with open(os.path.join(data_path, "ind_label.p"), "rb") as fh:
                label_index = pickle.load(fh)
            for utt, (file_ind, offset, length) in sample_index.items():
                self.index_sample[utt] = (os.path.join(data_path, "%s.npy" % file_ind), offset, length)
            for utt, (file_ind, offset, length) in label_index.items():
                self.index_label[utt] = (os.path.join(data_path, "%s_label.npy" % file_ind), offset, length)
            self.batchlist += sorted(sample_index)

    @staticmethod
    def _mapped(cache, path):
        if path not in cache:
            cache[path] = np.load(path, mmap_mode="r")
        return cache[path]

    def __getitem__(self, index):
        utt = self.batchlist[index]
        fea_path, off, n = self.index_sample[utt]
        label_path, off_l, n_l = self.index_label[utt]
        fea = self._mapped(self.memmaps_sample, fea_path)[off:off + n]
        label = self._mapped(self.memmaps_label, label_path)[off_l:off_l + n_l]
        self.reads += 1
        if self.reads >= self.read_limit:
            self.flush_memmaps()
        return fea.reshape((-1, 301, 80)), label

    def flush_memmaps(self):
        for cache in (self.memmaps_sample, self.memmaps_label):
            for path in cache:
                cache[path] = np.load(path, mmap_mode="r")
        self.reads = 0

    def __len__(self):
        return len(self.batchlist)


class DistributedSampler:
    """sampler.py: every iter() draws RandomState(seed=epoch).permutation(dataset_size) (epoch counts the iter() calls), repeats its
    head up to a multiple of num_replicas and yields the indices rank, rank + num_replicas, ..."""

    def __init__(self, dataset_size, num_replicas=None, rank=None, shuffle=True):
        self.dataset_size = dataset_size
        self.num_replicas = 1 if num_replicas is None else num_replicas
        self.rank = 0 if rank is None else rank
        self.epoch = 0
        self.num_samples = int(math.ceil(dataset_size / self.num_replicas))
        self.total_size = self.num_samples * self.num_replicas
        self.shuffle = shuffle

    def __iter__(self):
        if self.shuffle:
            indices = np.random.RandomState(seed=self.epoch).permutation(self.dataset_size).tolist()
            self.epoch += 1
        else:
            indices = list(range(self.dataset_size))
        indices += indices[:self.total_size - len(indices)]
        return iter(indices[self.rank:self.total_size:self.num_replicas])

    def __len__(self):
        return self.num_samples


class SpeakerHeadTrainer:
    """BuildTrainNetwork + TrainOneStepWithLossScaleCell of the example, restricted to the head: step(emb, labels) runs the fused
    AAM-softmax forward and backward on `classifier.weight`, the overflow check and Adam (betas 0.9 / 0.999, eps 1e-8, learning rate
    lr_list[step], weight decay added to the gradient as MindSpore's nn.Adam does).  The gradient is taken of loss_scale * loss and
    un-scaled inside Adam; on overflow the update is skipped on the device.  step() only enqueues work: the four returned values are
    device tensors (and the scale), and reading them is the caller's synchronisation."""

    def __init__(self, classifier, margin=0.2, scale=30.0, lr_list=(), weight_decay=0.0, loss_scale=2 ** 14):
        import torch

        self.classifier = classifier
        self.weight = classifier.weight.data
        if not self.weight.is_cuda or self.weight.dtype != torch.float32 or not self.weight.is_contiguous():
            raise ValueError("classifier.weight must be a contiguous float32 tensor on the HIP device")
        self.margin, self.scale, self.eps = float(margin), float(scale), 1e-4  # (eps: the default of MindSpore's L2Normalize)
        self.lr_list = lr_list
        self.weight_decay = float(weight_decay)
        self.loss_scale = float(loss_scale)
        self.b1, self.b2, self.adam_eps = 0.9, 0.999, 1e-8
        self.exp_avg = torch.zeros_like(self.weight)
        self.exp_avg_sq = torch.zeros_like(self.weight)
        self.grad = torch.empty_like(self.weight)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.weight.device)
        self.grad_scale = torch.full((1,), self.loss_scale, dtype=torch.float32, device=self.weight.device)
        self.global_step = 0

    def step(self, emb, labels):
        """-> (loss, overflow, scale, correct): loss () float32, overflow (1,) int32 (non-zero: the update was skipped), the loss
        scale, correct () int32, the number of rows whose arg-maximum of the margin-penalised output is their label.
        Labels given as a host array are range-checked (ValueError); labels already on the device are not read back - a label
        outside [0, N) then makes its row one without a target."""
        import torch

        from .. import ops
        from ..train import kernels as K
        from ..train.flat import adam_lr_t

        emb = emb.detach()
        on_device = isinstance(labels, torch.Tensor) and labels.is_cuda
        y = ops._aam_check(emb, self.weight, labels, check_labels=not on_device)
        output, _, loss, correct, saved = ops.aam_softmax_fwd(emb, self.weight, y, self.margin, self.scale, False, self.eps)
        dx = torch.empty_like(emb)
        ops.aam_softmax_bwd(emb, self.weight, y, output, saved, self.grad_scale, self.weight_decay * self.loss_scale, self.scale,
                            self.eps, dx=dx, dw=self.grad)
        self.flag.zero_()
        K.grad_overflow(self.grad, self.flag)
        lr = float(self.lr_list[min(self.global_step, len(self.lr_list) - 1)])
        lr_t = adam_lr_t(lr, self.global_step + 1, self.b1, self.b2)
        K.adam(self.weight, self.grad, self.exp_avg, self.exp_avg_sq, lr_t, self.b1, self.b2, self.adam_eps, 1.0 / self.loss_scale,
               self.flag)
        self.global_step += 1
        return loss.reshape(()), self.flag.clone(), self.loss_scale, correct.reshape(())


def _save_classifier(classifier, ckpt_dir, step, kept, keep_max):
    from ..utils.ckpt import write_mindspore_ckpt

    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, "ecapatdnn_vox12_head-%d.ckpt" % step)
    write_mindspore_ckpt(path, {"classifier.weight": classifier.weight.detach().cpu().numpy()})
    kept.append(path)
    while len(kept) > max(int(keep_max), 1):
        old = kept.pop(0)
        if os.path.exists(old):
            os.remove(old)
    return path


def train(cfg, model=None, log=print):
    """train() of the example on a config mapping, for the head alone (`freeze_embedding_model: true`).  `model`: an EcapaTDNN on the
    device instead of the one built from the yaml (and loaded from ckpt_save_dir / checkpoint_path when `pre_trained` is set).
    Returns the trained Classifier."""
    if not cfg.get("freeze_embedding_model"):
        raise NotImplementedError("training the embedding network needs the backward of the EcapaTDNN trunk (and train-mode BatchNorm), "
                                  "which is not built; set `freeze_embedding_model: true` to train the classifier head on a frozen model")
    import torch

    from ..models import Classifier, EcapaTDNN
    from ..utils.ckpt import load_mindspore_checkpoint

    dev = torch.device("cuda", torch.cuda.current_device())
    rank, group_size = int(cfg.get("rank", 0)), int(cfg.get("group_size", 1))
    emb_size, class_num = int(cfg["emb_size"]), int(cfg["class_num"])
    minibatch_size, num_epochs = int(cfg["minibatch_size"]), int(cfg["num_epochs"])
    ckpt_save_dir = str(cfg.get("ckpt_save_dir", "."))
    if model is None:
        channels = int(cfg["channels"])
        model = EcapaTDNN(int(cfg["in_channels"]), channels=(channels, channels, channels, channels, channels * 3), lin_neurons=emb_size)
        if cfg.get("pre_trained"):
            load_mindspore_checkpoint(model, os.path.join(ckpt_save_dir, str(cfg["checkpoint_path"])))
        model = model.to(dev)
    model.eval()
    dataset = DatasetGeneratorBatch(cfg["train_data_path"])
    sampler = DistributedSampler(len(dataset), group_size, rank, shuffle=True) if cfg.get("run_distribute") else \
        DistributedSampler(len(dataset), 1, 0, shuffle=False)
    steps_per_epoch = int(len(dataset) / group_size)
    log("group_size:%d, data total len:%d" % (group_size, steps_per_epoch))
    lr_list = [learning_rate_clr_triangle_function(float(cfg["step_size"]), float(cfg["max_lrate"]), float(cfg["base_lrate"]), i)
               for i in range(steps_per_epoch * num_epochs)]
    classifier = Classifier(1, 0, emb_size, class_num).to(dev)
    trainer = SpeakerHeadTrainer(classifier, 0.2, 30.0, lr_list or [float(cfg["base_lrate"])], float(cfg.get("weight_decay", 0.0)))
    save_steps = max(steps_per_epoch // 10, 1)
    print_dur = int(cfg.get("print_dur", 3000))
    kept = []
    if rank == 0:
        log("============== Starting Training ==============")
    for epoch in range(num_epochs):
        t_start = time.time()
        train_loss = train_loss_cur = torch.zeros((), device=dev)
        train_correct = train_correct_cur = torch.zeros((), device=dev)
        avg_loss = 0
        for idx, index in enumerate(sampler):
            data, gt_classes = dataset[index]
            if data.shape[0] != minibatch_size:
                continue
            feats = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(dev)
            emb = model(feats)
            batch_loss, _, _, correct = trainer.step(emb, np.asarray(gt_classes).reshape(-1).astype(np.int64))
            train_loss = train_loss + batch_loss
            train_correct = train_correct + correct
            train_loss_cur = train_loss_cur + batch_loss
            train_correct_cur = train_correct_cur + correct
            avg_loss = update_average(batch_loss, avg_loss, idx + 1)
            if rank == 0 and idx % print_dur == 0:
                cur_loss, acc = float(train_loss_cur), float(correct) / minibatch_size
                if idx > 0:
                    cur_loss, acc = cur_loss / print_dur, float(train_correct_cur) / (minibatch_size * print_dur)
                log("%s, epoch:%d/%d, iter-%d/%d,cur loss:%.4f, aver loss:%.4f,total_avg loss:%.4f, acc_aver:%.4f" % (
                    datetime.datetime.now(), epoch + 1, num_epochs, idx, steps_per_epoch, cur_loss, float(avg_loss),
                    float(train_loss) / (idx + 1), acc))
                train_loss_cur = torch.zeros((), device=dev)
                train_correct_cur = torch.zeros((), device=dev)
            if rank == 0 and trainer.global_step % save_steps == 0:
                _save_classifier(classifier, ckpt_save_dir, trainer.global_step, kept, cfg.get("keep_checkpoint_max", 5))
        if rank == 0 and steps_per_epoch:
            used = max(time.time() - t_start, 1e-9)
            log("epoch[%d], %.2f imgs/sec" % (epoch, minibatch_size * steps_per_epoch / used))
            log("Train Loss: %s" % (float(train_loss) / steps_per_epoch))
            log("Train Accuracy: %s %%" % (100.0 * float(train_correct) / (minibatch_size * steps_per_epoch)))
    return classifier


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    for key in ("train_data_path", "ckpt_save_dir", "checkpoint_path"):
        ap.add_argument("--" + key)
    a = ap.parse_args(argv)
    over = {k: v for k, v in vars(a).items() if k != "config_path" and v is not None}
    return train(load_config(a.config_path, over))


if __name__ == "__main__":
    main()
