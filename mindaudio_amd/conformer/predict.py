"""`python -m mindaudio_amd.conformer.predict --config_path conformer.yaml` — the counterpart of examples/conformer/predict.py for
decode_mode `ctc_greedy_search` (greedy CTC search + CER is the one external pin on the whole model, readme.md:126),
`ctc_prefix_beam_search` (the best prefix of the CTC prefix beam search), `attention_rescoring` (the prefix search's hypotheses
rescored by the attention decoder, the mode of the reference's best CER) and `attention` with `full_graph: true` (the autoregressive
beam search on the attention decoder, the shipped yaml's form: a KV-cached decoder step and a device-resident beam step).

Same yaml keys (test_data, dict, exp_name, decode_ckpt, decode_mode, dataset_conf, collate_conf), same per-utterance flow
(create_asr_predict_dataset, dataset.py:750-908: utterances outside the frame / token limits are dropped, one utterance per step,
Kaldi fbank of the waveform x 2^15, zero-padded to its frame bucket, mask of the real frames), the same id -> character rule
(predict.py:146-154: `w += 2`, stop at eos, ids past the dictionary skipped) and the same outputs: `<exp_name>/test_<mode>/result.txt`
with "<uttid> <text>" lines, one "cer" log line per utterance, "cer_average" at the end.  The two beam modes take the yaml's top-level
`beam_size` (default 10) and, for the rescoring, the decode section's top-level `ctc_weight` (default 0.0; not model_conf.ctc_weight);
both searches run on the GPU (ma_ctc_topk_f32, ma_ctc_prefix_beam_search_f32, ma_hyp_score_f32).  `attention` takes `beam_size` too and
writes `<exp_name>/test_attention/result.txt`.  `attention_rescoring` and `attention` need the attention decoder: a pure-CTC model
(model_conf.ctc_weight 1.0) raises NotImplementedError.  `attention` with `full_graph` absent or false - the reference's host-stepped
PredictNet form - raises NotImplementedError as well: it is not built, `full_graph: true` (or --full_graph) selects the built one."""
import argparse
import os


def load_language_dict(dict_file):
    """dataset.py:825-837: {id: symbol} with char_dict[0] = 0; sos = eos = the last id; vocab_size = number of entries."""
    char_dict = {}
    with open(dict_file, "r") as fin:
        for line in fin:
            arr = line.strip().split()
            if len(arr) != 2:
                raise ValueError("dictionary lines are '<symbol> <id>': %r" % line)
            char_dict[int(arr[1])] = arr[0]
    char_dict[0] = 0
    sos = eos = len(char_dict) - 1
    return sos, eos, len(char_dict), char_dict


def predict_samples(data_file, dict_file, dataset_conf, frame_factor=100):
    """AsrPredictDataset (dataset.py:750-822): [(uttid, wav_path, frames, [token ids])] inside the frame and token limits."""
    from .dataset import load_samples

    lo, hi = int(dataset_conf["min_length"]), int(dataset_conf["max_length"])
    tlo, thi = int(dataset_conf["token_min_length"]), int(dataset_conf["token_max_length"])
    out = []
    for uttid, path, frames, ids, _ in load_samples(data_file, dict_file, frame_factor):
        toks = [int(t) for t in ids.split()]
        if lo <= frames <= hi and tlo <= len(toks) <= thi:
            out.append((uttid, path, frames, toks))
    return out


def bucket_length(frames, frame_bucket_limit):
    """get_padding_length (dataset.py:212 of the reference's collate helpers): the first bucket that holds the utterance."""
    for limit in frame_bucket_limit:
        if limit > frames:
            return limit
    return frame_bucket_limit[-1]


def ids_to_text(hyp, eos, char_dict):
    """predict.py:146-154."""
    out = []
    for w in hyp:
        w += 2
        if w == eos:
            break
        if w > len(char_dict):
            continue
        out.append(char_dict[w])
    return out


def predict(config, device=None, log=print, model=None):
    """Runs the decode of config["decode_mode"] over config["test_data"]; returns (mean CER, [(uttid, text, cer)])."""
    import numpy as np
    import torch

    from ..data.io import read
    from ..metric import wer
    from .asr_model import (Attention, AttentionRescoring, CTCGreedySearch, CTCPrefixBeamSearch, attention_rescoring,
                            ctc_greedy_search, ctc_prefix_beam_search, recognize)
    from .dataset import compute_fbank_feats_batch

    mode = config.get("decode_mode", "ctc_greedy_search")
    if mode == "attention" and not config.get("full_graph", False):
        raise NotImplementedError("decode_mode 'attention' without full_graph: the host-stepped form of the attention search is not "
                                  "built; full_graph: true selects the built, device-resident one")
    if mode not in ("ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring", "attention"):
        raise NotImplementedError("decode_mode %r: ctc_greedy_search, ctc_prefix_beam_search, attention_rescoring and attention "
                                  "(full_graph: true) are built" % mode)
    if mode in ("attention_rescoring", "attention"):
        has_decoder = getattr(model, "decoder", None) is not None if model is not None else \
            float((config.get("model_conf") or {}).get("ctc_weight", 0.3)) != 1.0
        if not has_decoder:
            raise NotImplementedError("%s needs the attention decoder; this model is pure CTC (ctc_weight 1.0)" % mode)
    beam_size = int(config.get("beam_size", 10))
    ctc_weight = float(config.get("ctc_weight", 0.0))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    sos, eos, vocab_size, char_dict = load_language_dict(config["dict"])
    fe = config["collate_conf"]["feature_extraction_conf"]
    buckets = [int(v) for v in str(config["dataset_conf"]["frame_bucket_limit"]).split(",")]
    samples = predict_samples(config["test_data"], config["dict"], config["dataset_conf"])
    if model is None:
        from ..utils.ckpt import load_mindspore_checkpoint
        from .train import build_model

        model = build_model(config, int(fe["mel_bins"]), vocab_size, device)
        ckpt = os.path.join(str(config.get("exp_name", "default")), "model", str(config["decode_ckpt"]))
        load_mindspore_checkpoint(model, ckpt, strict=False)
        log("Successfully loading the asr model: %s" % ckpt)
    model.eval()
    if mode == "ctc_greedy_search":
        net = CTCGreedySearch(model)
    elif mode == "attention":
        net = Attention(model, beam_size, eos)
    else:
        net = CTCPrefixBeamSearch(model, beam_size)
        rescore = AttentionRescoring(model, beam_size) if mode == "attention_rescoring" else None
    decode_dir = os.path.join(str(config.get("exp_name", "default")), "test_" + mode)
    os.makedirs(decode_dir, exist_ok=True)
    log("Total predict samples size: %d" % len(samples))
    results, total = [], 0.0
    with open(os.path.join(decode_dir, "result.txt"), "w") as result_file:
        for count, (uttid, path, frames, tokens) in enumerate(samples, 1):
            wav, sr = read(path)
            wav = np.asarray(wav, dtype=np.float32) * (1 << 15)
            feats, nfr = compute_fbank_feats_batch(wav[None], [wav.shape[0]], sample_rate=sr, frame_len=int(fe["frame_length"]),
                                                   frame_shift=int(fe["frame_shift"]), mel_bin=int(fe["mel_bins"]))
            n = int(nfr[0])
            pad = max(bucket_length(frames, buckets), n)
            xs = torch.zeros((1, pad, feats.shape[-1]), dtype=torch.float32, device=device)
            xs[0, :n] = feats[0, :n]
            masks = torch.zeros((1, 1, pad), dtype=torch.float32, device=device)
            masks[0, 0, :n] = 1
            if mode == "ctc_greedy_search":
                hyps, _ = ctc_greedy_search(net, xs, masks, None)
            elif mode == "ctc_prefix_beam_search":
                beams, _, _ = ctc_prefix_beam_search(net, xs, masks, beam_size, None)
                hyps = [list(beams[0][0][0])]
            elif mode == "attention":  # predict.py:90-111: the search's initial state, one utterance per step
                start_token = np.array([sos], np.int32)
                scores = np.array([0.0] + [-float("inf")] * (beam_size - 1), np.float32)
                end_flag = np.array([0.0] * beam_size, np.float32)
                base_index = np.arange(xs.shape[0], dtype=np.int32).reshape(-1, 1)
                hyps, _ = recognize(net, xs, masks, start_token, base_index, scores, end_flag, beam_size, eos, None, True)
                hyps = [hyp.tolist() for hyp in hyps]
            else:
                hyps, _ = attention_rescoring(net, rescore, xs, masks, None, sos, eos, beam_size, ctc_weight)
            content = ids_to_text(hyps[0], eos, char_dict)
            truth = [char_dict[w + 2] for w in tokens]
            log("Labs (%d/%d): %s %s" % (count, len(samples), uttid, "".join(str(c) for c in truth)))
            log("Hyps (%d/%d): %s %s" % (count, len(samples), uttid, "".join(str(c) for c in content)))
            if not content:
                raise ValueError("The Hypothesis utterance should not be empty")  # predict.py:164-165
            cer = wer(truth, content)
            log("cer : %.3f" % cer)
            result_file.write("{} {}\n".format(uttid, "".join(str(c) for c in content)))
            result_file.flush()
            results.append((uttid, "".join(str(c) for c in content), cer))
            total += cer
    mean = total / max(len(results), 1)
    log("cer_average : %f" % mean)
    return mean, results


def main(argv=None):
    from .train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    ap.add_argument("--test_data")
    ap.add_argument("--dict")
    ap.add_argument("--exp_name")
    ap.add_argument("--decode_ckpt")
    ap.add_argument("--decode_mode")
    ap.add_argument("--beam_size", type=int)
    ap.add_argument("--ctc_weight", type=float)
    ap.add_argument("--full_graph", action="store_const", const=True, help="decode_mode attention: the device-resident search")
    a = ap.parse_args(argv)
    over = {k: v for k, v in vars(a).items() if k != "config_path" and v is not None}
    predict(load_config(a.config_path, over))


if __name__ == "__main__":
    main()
