"""`python -m mindaudio_amd.deepspeech2.eval --config_path deepspeech2.yaml` - the counterpart of examples/deepspeech2/eval.py.

Reads the example's yaml keys (SpectConfig, ModelConfig, EvalConfig, Pretrained_model, labels), builds DeepSpeechModel inside
PredictWithSoftmax, loads the MindSpore checkpoint, and for every batch of the evaluation manifest decodes greedily and prints the
reference's lines: `Ref:`, `Hyp:`, `WER: x CER: y` per utterance and at the end
`Test Summary \\tAverage WER {:.3f}\\tAverage CER {:.3f}\\t` in percent (WER over the reference's words, CER over its characters
without spaces)."""
import argparse

import numpy as np


def build_model(config):
    from ..models.deepspeech2 import DeepSpeechModel, PredictWithSoftmax

    net = DeepSpeechModel(batch_size=int(config["EvalConfig"]["batch_size"]), rnn_hidden_size=int(config["ModelConfig"]["hidden_size"]),
                          nb_layers=int(config["ModelConfig"]["hidden_layers"]), labels=config["labels"],
                          rnn_type=config["ModelConfig"]["rnn_type"], audio_conf=config["SpectConfig"], bidirectional=True)
    net.load_checkpoint(str(config["Pretrained_model"]))
    return PredictWithSoftmax(net.cuda().eval())


def split_targets(target_indices, targets):
    """eval.py:90-101: the flat label_values cut into one list per utterance by the first column of target_indices."""
    out = []
    start, count, last_id = 0, 0, 0
    for i in range(np.shape(targets)[0]):
        if target_indices[i, 0] == last_id:
            count += 1
        else:
            out.append(list(targets[start:count]))
            last_id += 1
            start = count
            count += 1
    out.append(list(targets[start:]))
    return out


def evaluate(config, model=None, log=print):
    """eval.py:36-132 on a config mapping; returns (WER, CER) as fractions.  `model`: a callable (inputs (b, 1, F, 3500), input_length)
    -> (probabilities (b, T1, classes), output sizes) used as it is, instead of the one built from the config."""
    from .. import _host
    from ..models.decoders import MSGreedyDecoder
    from .dataset import ASRDataset

    _host.require_gpu()
    labels = config["labels"]
    if model is None:
        model = build_model(config)
        log("Successfully loading the pre-trained model")
    ds_eval = ASRDataset(audio_conf=config["SpectConfig"], manifest_filepath=config["EvalConfig"]["test_manifest"], labels=labels,
                         normalize=True, batch_size=int(config["EvalConfig"]["batch_size"]), is_training=False)
    decoder = MSGreedyDecoder(labels=labels, blank_index=labels.index("_"))
    target_decoder = MSGreedyDecoder(labels, blank_index=labels.index("_"))
    total_cer, total_wer, num_tokens, num_chars = 0, 0, 0, 0
    for index in range(len(ds_eval)):
        inputs, input_length, target_indices, targets = ds_eval[index]
        out, output_sizes = model(inputs, input_length)
        decoded_output, _ = decoder.decode(out, output_sizes)
        target_strings = target_decoder.convert_to_strings(split_targets(target_indices, targets))
        for doutput, toutput in zip(decoded_output, target_strings):
            transcript, reference = doutput[0], toutput[0]
            wer_inst = decoder.wer(transcript, reference)
            cer_inst = decoder.cer(transcript, reference)
            total_wer += wer_inst
            total_cer += cer_inst
            num_tokens += len(reference.split())
            num_chars += len(reference.replace(" ", ""))
            log("Ref:", reference.lower())
            log("Hyp:", transcript.lower())
            log("WER:", float(wer_inst) / len(reference.split()), "CER:", float(cer_inst) / len(reference.replace(" ", "")), "\n")
    wer = float(total_wer) / num_tokens
    cer = float(total_cer) / num_chars
    log("Test Summary \tAverage WER {wer:.3f}\tAverage CER {cer:.3f}\t".format(wer=wer * 100, cer=cer * 100))
    return wer, cer


def main(argv=None):
    from ..conformer.train import load_config

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_path", required=True)
    ap.add_argument("--Pretrained_model")
    a = ap.parse_args(argv)
    return evaluate(load_config(a.config_path, {"Pretrained_model": a.Pretrained_model}))


if __name__ == "__main__":
    main()
