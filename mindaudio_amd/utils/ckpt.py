"""MindSpore `.ckpt` -> this package's modules: the importer that lets the released Conformer checkpoint
(examples/conformer/readme.md:118-136) be evaluated here; examples/conformer/predict.py:66-67 does
`load_param_into_net(network, load_checkpoint(path))`.

The checkpoint format belongs to MindSpore 2.3.0 (requirements.txt:1), which is not vendored and not installed here, so this
file restates its published layout — **parity unpinned** (no reference checkpoint can be produced or fetched in this
container; the tests round-trip through the writer below):

    message Checkpoint { message Value { required string tag = 1; required TensorProto tensor = 2; } repeated Value value = 1; }
    message TensorProto { repeated int64 dims = 1; required string tensor_type = 2; required bytes tensor_content = 3; }

`save_checkpoint` writes one serialised Checkpoint per parameter slice back to back (a protobuf stream concatenates), large
parameters split along axis 0 into several values with the same tag.  Parsed here with a 40-line wire-format reader: no protobuf
schema compilation, no MindSpore.

Parameter names follow the reference's cell attributes (mindaudio/models/conformer.py, mindaudio/models/layers/*.py):
wrappers `Dense.dense`, `Conv1d.conv1d`, `Conv2d.conv2d`, `nn.SequentialCell` indices, BatchNorm `gamma/beta/moving_*`,
`nn.Embedding.embedding_table`; `convert_names` maps them onto the names of mindaudio_amd.conformer.asr_model.ASRModel.
`convert_ecapa_names` / `ecapa_to_reference_names` do the same for EcapaTDNN (mindaudio/models/ecapatdnn.py), which
`load_mindspore_checkpoint` picks when it is handed that module, and `convert_conv_tasnet_names` /
`conv_tasnet_to_reference_names` for ConvTasNet (mindaudio/models/conv_tasnet.py), `convert_tasnet_names` /
`tasnet_to_reference_names` for TasNet (mindaudio/models/tasnet.py).
"""
import re

import numpy as np

__all__ = ["read_mindspore_ckpt", "write_mindspore_ckpt", "convert_names", "to_reference_names", "read_epoch_num",
           "load_mindspore_checkpoint", "convert_ecapa_names", "ecapa_to_reference_names", "convert_conv_tasnet_names",
           "conv_tasnet_to_reference_names", "convert_tasnet_names", "tasnet_to_reference_names"]

_DTYPES = {"Float32": np.float32, "Float16": np.float16, "Float64": np.float64, "Int32": np.int32, "Int64": np.int64,
           "Int16": np.int16, "Int8": np.int8, "UInt8": np.uint8, "UInt16": np.uint16, "UInt32": np.uint32,
           "UInt64": np.uint64, "Bool": np.bool_}
_NAMES = {np.dtype(v).name: k for k, v in _DTYPES.items()}


def _varint(buf, pos):
    val, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        val |= (b & 0x7F) << shift
        if not b & 0x80:
            return val, pos
        shift += 7


def _fields(buf):
    """(field number, wire type, value) of one message; value = int (varint / fixed) or memoryview (length-delimited)."""
    pos, end = 0, len(buf)
    while pos < end:
        key, pos = _varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            val, pos = _varint(buf, pos)
        elif wt == 2:
            n, pos = _varint(buf, pos)
            val = buf[pos:pos + n]
            if len(val) != n:
                raise ValueError("truncated checkpoint")
            pos += n
        elif wt == 1:
            val = int.from_bytes(buf[pos:pos + 8], "little")
            pos += 8
        elif wt == 5:
            val = int.from_bytes(buf[pos:pos + 4], "little")
            pos += 4
        else:
            raise ValueError("unsupported protobuf wire type %d (encrypted or corrupt checkpoint?)" % wt)
        yield num, wt, val


def _signed(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def read_mindspore_ckpt(path):
    """{parameter name: ndarray} of a MindSpore checkpoint file, slices of one parameter joined along axis 0."""
    with open(path, "rb") as f:
        buf = memoryview(f.read())
    parts = {}
    for num, wt, val in _fields(buf):
        if num != 1 or wt != 2:
            continue
        tag, tensor = None, None
        for n2, w2, v2 in _fields(val):
            if n2 == 1 and w2 == 2:
                tag = bytes(v2).decode("utf-8")
            elif n2 == 2 and w2 == 2:
                tensor = v2
        if tag is None or tensor is None:
            raise ValueError("checkpoint value without tag / tensor")
        dims, ttype, content = [], None, b""
        for n3, w3, v3 in _fields(tensor):
            if n3 == 1 and w3 == 0:
                dims.append(_signed(v3))
            elif n3 == 1 and w3 == 2:  # packed encoding
                p = 0
                while p < len(v3):
                    d, p = _varint(v3, p)
                    dims.append(_signed(d))
            elif n3 == 2 and w3 == 2:
                ttype = bytes(v3).decode("utf-8")
            elif n3 == 3 and w3 == 2:
                content = v3
        if ttype == "BFloat16":
            arr = (np.frombuffer(content, np.uint16).astype(np.uint32) << 16).view(np.float32)
        elif ttype in _DTYPES:
            arr = np.frombuffer(content, _DTYPES[ttype])
        else:
            raise ValueError("unsupported tensor_type %r for %s" % (ttype, tag))
        shape = tuple(dims) if dims and dims != [0] else ()
        parts.setdefault(tag, []).append(arr.reshape(shape) if shape else arr.reshape(()) if arr.size == 1 else arr)
    return {k: (v[0] if len(v) == 1 else np.concatenate(v, axis=0)).copy() for k, v in parts.items()}


def _enc_varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _ld(num, payload):
    return _enc_varint(num << 3 | 2) + _enc_varint(len(payload)) + payload


def write_mindspore_ckpt(path, params, slice_bytes=512 * 1024 * 1024):
    """Serialise {name: ndarray} in the layout above (the exporter of `ConformerCTCTrainStep.sync_to_module()` weights, and
    what the importer's tests read back)."""
    with open(path, "wb") as f:
        for name, arr in params.items():
            arr = np.asarray(arr, order="C")  # (ascontiguousarray would turn a scalar into shape (1,))
            n_slices = max(1, -(-arr.nbytes // slice_bytes)) if arr.ndim else 1
            for piece in (np.array_split(arr, n_slices) if n_slices > 1 else [arr]):
                dims = b"".join(_enc_varint(1 << 3 | 0) + _enc_varint(d) for d in (piece.shape or (0,)))
                tensor = dims + _ld(2, _NAMES[piece.dtype.name].encode()) + _ld(3, piece.tobytes())
                f.write(_ld(1, _ld(1, name.encode()) + _ld(2, tensor)))


_SKIP = re.compile(r"^(moments?\d*\.|moment[12]\.|adam_[mv]\.|accu_grads\.|global_step$|learning_rate$|scale_sense$|step$|"
                   r"epoch_num$|step_num$|loss_scale$|cur_step$|beta[12]_power$|current_iterator_step$|"
                   r"last_overflow_iterator_step$)")
_PREFIXES = ("network.", "_backbone.", "acc_net.", "net.", "model.")


def convert_names(ref_params):
    """Reference (MindSpore cell) parameter names -> names of this package's ASRModel / ConformerEncoder state dict.
    Optimizer / loss-scale state is dropped; conv1d weights lose MindSpore's extra unit axis ((out, in, 1, k) -> (out, in, k))."""
    out = {}
    for name, arr in ref_params.items():
        while name.startswith(_PREFIXES):
            name = name[len(next(p for p in _PREFIXES if name.startswith(p))):]
        if _SKIP.match(name):
            continue
        n = name
        n = n.replace(".dense.", ".")                              # layers/dense.py:51
        n = re.sub(r"\.embed\.conv\.0\.conv2d\.", ".embed.conv1.", n)   # layers/subsampling.py:40-45, layers/conv2d.py:55
        n = re.sub(r"\.embed\.conv\.2\.conv2d\.", ".embed.conv2.", n)
        if ".conv1d." in n:                                          # layers/conv1d.py:73
            n = n.replace(".conv1d.", ".")
            if arr.ndim == 4 and arr.shape[2] == 1:
                arr = arr[:, :, 0, :]
        if ".conv_module.norm." in n:                                # layers/convolution.py:63 (BatchNorm1d)
            n = (n.replace(".norm.gamma", ".norm.weight").replace(".norm.beta", ".norm.bias")
                 .replace(".norm.moving_mean", ".norm.running_mean").replace(".norm.moving_variance", ".norm.running_var"))
        n = n.replace("decoder.embed.0.embedding_table", "decoder.embed.weight")  # models/conformer.py:555-558
        out[n] = arr
    return out


def to_reference_names(state, prefix=""):
    """Inverse of `convert_names` for the modules of this package: {state_dict name: tensor / ndarray} -> {the name and layout
    MindSpore gives the same parameter in the reference's cells: ndarray}, so that a file written from it loads with the reference's
    `load_param_into_net` (Dense.dense, Conv1d.conv1d with the unit axis, Conv2d.conv2d inside the SequentialCell, BatchNorm
    gamma / beta / moving_mean / moving_variance as Parameters, Embedding.embedding_table).  `num_batches_tracked` has no MindSpore
    counterpart and is dropped; GlobalCMVN's statistics are constructor data, never parameters (layers/cmvn.py)."""
    out = {}
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            continue
        a = v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        n = k
        if ".embed.conv1." in n or ".embed.conv2." in n:
            n = n.replace(".embed.conv1.", ".embed.conv.0.conv2d.").replace(".embed.conv2.", ".embed.conv.2.conv2d.")
        elif ".conv_module." in n and ("pointwise_conv" in n or "depthwise_conv" in n):
            n = n.replace(".weight", ".conv1d.weight").replace(".bias", ".conv1d.bias")
            if a.ndim == 3:
                a = a[:, :, None, :]
        elif ".conv_module.norm." in n:
            n = (n.replace(".norm.weight", ".norm.gamma").replace(".norm.bias", ".norm.beta")
                 .replace("running_mean", "moving_mean").replace("running_var", "moving_variance"))
        elif n == "decoder.embed.weight":
            n = "decoder.embed.0.embedding_table"
        elif n.startswith("ctc.ctc_lo.") or n.endswith((".gamma", ".beta", "pos_bias_u", "pos_bias_v")):
            pass  # loss/ctc_loss.py builds a bare nn.Dense; LayerNorm and the attention biases are plain Parameters
        else:  # layers/dense.py: every other weight / bias sits inside the Dense wrapper
            n = n.replace(".weight", ".dense.weight").replace(".bias", ".dense.bias")
        out[prefix + n] = a
    return out


_BN_REF = (("gamma", "weight"), ("beta", "bias"), ("moving_mean", "running_mean"), ("moving_variance", "running_var"))


def _strip(name):
    while name.startswith(_PREFIXES):
        name = name[len(next(p for p in _PREFIXES if name.startswith(p))):]
    return name


def convert_ecapa_names(ref_params):
    """Reference EcapaTDNN (mindaudio/models/ecapatdnn.py) parameter names -> mindaudio_amd.models.EcapaTDNN's state dict.
    The cell attributes already carry this package's names (blocks.N.conv, .tdnn1, .res2net_block.blocks.M, .se_block.conv1, mfa,
    asp.tdnn, asp.conv, asp_bn, fc); what differs is MyBatchNorm1d's wrapped BatchNorm2d (`<bn>.norm2d.gamma / beta / moving_mean /
    moving_variance` -> `<bn>.weight / bias / running_mean / running_var`) and the unit axis MindSpore's nn.Conv1d keeps in its
    weight ((out, in, 1, k) -> (out, in, k)).  Optimizer state and the training classifier's parameters are not the model's: the
    former is dropped here, the latter is reported as unexpected by the loader."""
    out = {}
    for name, arr in ref_params.items():
        n = _strip(name)
        if _SKIP.match(n):
            continue
        if ".norm2d." in n:
            head, leaf = n.rsplit(".norm2d.", 1)
            n = head + "." + dict(_BN_REF).get(leaf, leaf)
        elif n.endswith(".weight") and arr.ndim == 4 and arr.shape[2] == 1:
            arr = arr[:, :, 0, :]
        out[n] = arr
    return out


def ecapa_to_reference_names(state, prefix=""):
    """Inverse of `convert_ecapa_names`: an EcapaTDNN state dict of this package -> {reference name: ndarray in MindSpore's
    layout}, so that a file written from it loads in the reference.  `num_batches_tracked` has no MindSpore counterpart."""
    own_bn = {b: a for a, b in _BN_REF}
    out = {}
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            continue
        a = v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        head, leaf = k.rsplit(".", 1)
        if head.endswith(".norm") or head == "asp_bn":
            k = head + ".norm2d." + own_bn[leaf]
        elif leaf == "weight" and a.ndim == 3:
            a = a[:, :, None, :]
        out[prefix + k] = a
    return out


def _is_ecapa(module):
    return type(module).__name__ == "EcapaTDNN"


_TASNET_ALIAS = re.compile(r"(^|\.)(network|net)\.")


def convert_conv_tasnet_names(ref_params):
    """Reference ConvTasNet (mindaudio/models/conv_tasnet.py) parameter names -> mindaudio_amd.models.ConvTasNet's state dict.
    The cell attributes already carry this package's names (encoder.conv1d_U, separator.bottleneck_conv1x1,
    separator.temporal_conv_net.<r>.<x>.{conv1x1, prelu, dsconv.depthwise_conv, dsconv.prelu, dsconv.pointwise_conv},
    separator.mask_conv1x1, decoder.basis_signals); what differs is nn.PReLU's leaf (`w` -> `weight`) and the unit axis MindSpore's
    nn.Conv1d keeps in its weight ((out, in, 1, k) -> (out, in, k); (out, in, k) is accepted as it is).  The reference registers the
    same cells a second time inside SequentialCells (`separator.network.*`, `<block>.net.*`): a checkpoint that carries those
    duplicate names has them ignored, like the optimizer state.  The global layer norm's gamma / beta are NumPy constants in the
    reference, not parameters, so no name exists for them.
    Not verified against a file MindSpore wrote (none can be produced here): which of the duplicate paths it saves is inferred from
    the cell definitions."""
    out = {}
    for name, arr in ref_params.items():
        n = _strip(name)
        if _SKIP.match(n) or _TASNET_ALIAS.search(n):
            continue
        if n.endswith(".prelu.w"):
            n = n[:-1] + "weight"
        elif n.endswith(".weight") and arr.ndim == 4 and arr.shape[2] == 1:
            arr = arr[:, :, 0, :]
        out[n] = arr
    return out


def conv_tasnet_to_reference_names(state, prefix=""):
    """Inverse of `convert_conv_tasnet_names`: a ConvTasNet state dict of this package -> {reference name: ndarray in MindSpore's
    layout} (Conv1d weights with the unit axis, the PReLU leaf `w`)."""
    out = {}
    for k, v in state.items():
        a = v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if k.endswith(".prelu.weight"):
            k = k[:-len("weight")] + "w"
        elif k.endswith(".weight") and a.ndim == 3:
            a = a[:, :, None, :]
        out[prefix + k] = a
    return out


def _is_conv_tasnet(module):
    return type(module).__name__ == "ConvTasNet"


def convert_deepspeech2_names(ref_params):
    """Reference DeepSpeechModel (mindaudio/models/deepspeech2.py) parameter names -> mindaudio_amd.models.DeepSpeechModel's state
    dict.  The module keeps the reference's cell names and layouts (conv.conv1.weight, conv.bn1.gamma / beta / moving_mean /
    moving_variance, conv.conv2.weight, conv.bn2.*, RNN.lstms.<k>.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0 and their
    `_reverse` twins, fc.module.weight), so only wrapper prefixes and optimizer state are removed.  MaskConv registers its cells a second
    time in `conv.module_list.<i>`: those duplicates are ignored.
    Not verified against a file MindSpore wrote (none can be produced here): the names, and the per-direction split of nn.LSTM's
    weights, are inferred from the cell definitions."""
    out = {}
    for name, arr in ref_params.items():
        n = _strip(name)
        if _SKIP.match(n) or ".module_list." in n:
            continue
        out[n] = arr
    return out


def deepspeech2_to_reference_names(state, prefix=""):
    """Inverse of `convert_deepspeech2_names`: the names and layouts are already the reference's."""
    return {prefix + k: (v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in state.items()}


def _is_deepspeech2(module):
    return type(module).__name__ == "DeepSpeechModel"


_TASNET_UNUSED = "separator.new_lstm."  # tasnet.py:111: Dense(500, 512), never called by construct()


def convert_tasnet_names(ref_params):
    """Reference TasNet (mindaudio/models/tasnet.py) parameter names -> mindaudio_amd.models.TasNet's state dict.  The cell
    attributes already carry this package's names: encoder.conv1d_U|V.weight|bias, separator.layer_norm.gamma|beta,
    separator.lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l<k>, separator.fc.weight|bias, decoder.basis_signals.weight|bias.  What
    differs is the unit axis MindSpore's nn.Conv1d keeps in its weight ((N, L, 1, 1) -> (N, L, 1)), handled as for Conv-TasNet.
    `separator.new_lstm.*`, the reference's unused Dense(500, 512), is accepted and ignored, like the optimizer state.
    Not verified against a file MindSpore wrote (none can be produced here): the names, and nn.LSTM's per-layer split of its
    weights, are inferred from the cell definitions."""
    out = {}
    for name, arr in ref_params.items():
        n = _strip(name)
        if _SKIP.match(n) or n.startswith(_TASNET_UNUSED):
            continue
        if n.endswith(".weight") and np.ndim(arr) == 4 and np.shape(arr)[2] == 1:
            arr = np.asarray(arr)[:, :, 0, :]
        out[n] = arr
    return out


def tasnet_to_reference_names(state, prefix="", new_lstm=None):
    """Inverse of `convert_tasnet_names`: a TasNet state dict of this package -> {reference name: ndarray in MindSpore's layout}
    (Conv1d weights with the unit axis).  `separator.new_lstm.weight` (512, 500) and `.bias` (512) are written back so that the
    reference's load_param_into_net finds every parameter of its cell: from `new_lstm` = (weight, bias) when given, zeros otherwise
    (the layer is never called)."""
    out = {}
    for k, v in state.items():
        a = v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if k.endswith(".weight") and a.ndim == 3:
            a = a[:, :, None, :]
        out[prefix + k] = a
    w, b = new_lstm if new_lstm is not None else (np.zeros((512, 500), np.float32), np.zeros((512,), np.float32))
    out[prefix + _TASNET_UNUSED + "weight"], out[prefix + _TASNET_UNUSED + "bias"] = np.asarray(w, np.float32), np.asarray(b, np.float32)
    return out


def _is_tasnet(module):
    return type(module).__name__ == "TasNet"


def convert_wavegrad_names(ref_params):
    """Reference WaveGrad (mindaudio/models/wavegrad/wavegrad_v190.py) parameter names -> mindaudio_amd.models.WaveGrad's state dict.
    The cell attributes already carry this package's names (DBlock.0, DBlock.<n>.{residual_dense, conv.1|3|5, downscale1,
    downscale2}, FiLM.<n>.{input_conv, output_conv}, UBlock.<n>.{block1, block2_a, block2_b, block3_a, block3_b}, first_conv,
    last_conv, each with .weight / .bias); what differs is the unit axis MindSpore's nn.Conv1d keeps in its weight ((out, in, 1, k) ->
    (out, in, k); (out, in, k) is accepted as it is).  `cur_step`, the optimizer's `moment*` and `global_step` are ignored.
    Not verified against a file MindSpore wrote (none can be produced here): the names are inferred from the cell definitions."""
    out = {}
    for name, arr in ref_params.items():
        n = _strip(name)
        if _SKIP.match(n):
            continue
        if n.endswith(".weight") and np.ndim(arr) == 4 and np.shape(arr)[2] == 1:
            arr = np.asarray(arr)[:, :, 0, :]
        out[n] = arr
    return out


def wavegrad_to_reference_names(state, prefix=""):
    """Inverse of `convert_wavegrad_names`: a WaveGrad state dict of this package -> {reference name: ndarray in MindSpore's layout}
    (Conv1d weights with the unit axis)."""
    out = {}
    for k, v in state.items():
        a = v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if k.endswith(".weight") and a.ndim == 3:
            a = a[:, :, None, :]
        out[prefix + k] = a
    return out


def _is_wavegrad(module):
    return type(module).__name__ == "WaveGrad"


_FS2_BINS = {"pitch_bins_log": "pitch_bins", "pitch_bins": "pitch_bins", "energy_bins_log": "energy_bins", "energy_bins": "energy_bins"}


def convert_fastspeech2_names(ref_params):
    """Reference FastSpeech2 (mindaudio/models/fastspeech2/fastspeech2_v190.py) parameter names -> mindaudio_amd.models.FastSpeech2's
    state dict.  The cell attributes already carry this package's names ({encoder, expanded_encoder, decoder}.layer_stack.<n>.
    {slf_attn.{w_qs, w_ks, w_vs, fc, layer_norm}, pos_ffn.{w_1, w_2, layer_norm}}, variance_adaptor.<x>_predictor.{conv1.0, norm1,
    conv2.0, norm2, linear_layer}, mel_linear).  What differs: nn.Embedding's leaf (`embedding_table` -> `weight`), the unit axis
    MindSpore's nn.Conv1d keeps in its weight ((out, in, 1, k) -> (out, in, k)), and the explicitly named bin parameters
    (`pitch_bins_log` / `pitch_bins`, `energy_bins` / `energy_bins_log`, with or without the `variance_adaptor.` prefix) ->
    variance_adaptor.pitch_bins / energy_bins.  A checkpoint without bins leaves the module's own (computed from `stats`).
    Not verified against a file MindSpore wrote (none can be produced here): the names are inferred from the cell definitions."""
    out = {}
    for name, arr in ref_params.items():
        n = _strip(name)
        if _SKIP.match(n):
            continue
        leaf = n.rsplit(".", 1)[-1]
        if leaf in _FS2_BINS and n in (leaf, "variance_adaptor." + leaf):
            n = "variance_adaptor." + _FS2_BINS[leaf]
        elif leaf == "embedding_table":
            n = n[:-len(leaf)] + "weight"
        elif leaf == "weight" and np.ndim(arr) == 4 and np.shape(arr)[2] == 1:
            arr = np.asarray(arr)[:, :, 0, :]
        out[n] = arr
    return out


def fastspeech2_to_reference_names(state, prefix="", pitch_quantization="log", energy_quantization="linear"):
    """Inverse of `convert_fastspeech2_names`: a FastSpeech2 state dict of this package -> {reference name: ndarray in MindSpore's
    layout}; the bins go out under the names the reference gives them for the two quantization settings."""
    out = {}
    for k, v in state.items():
        a = v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if k == "variance_adaptor.pitch_bins":
            k = "variance_adaptor.pitch_bins" + ("_log" if pitch_quantization == "log" else "")
        elif k == "variance_adaptor.energy_bins":
            k = "variance_adaptor.energy_bins" + ("_log" if energy_quantization == "log" else "")
        elif k.endswith(("src_word_emb.weight", "_embedding.weight")):
            k = k[:-len("weight")] + "embedding_table"
        elif k.endswith(".weight") and a.ndim == 3:
            a = a[:, :, None, :]
        out[prefix + k] = a
    return out


def _is_fastspeech2(module):
    return type(module).__name__ == "FastSpeech2"


def read_epoch_num(path):
    """`int(param_dict.get("epoch_num", 0))` of examples/conformer/train.py:121 - the number of finished epochs the reference's
    ModelCheckpoint appends to every file (`append_info=[{"epoch_num": ...}]`, train.py:157-163)."""
    v = read_mindspore_ckpt(path).get("epoch_num")
    return int(np.asarray(v).reshape(-1)[0]) if v is not None else 0


def load_mindspore_checkpoint(module, path, strict=True):
    """load_checkpoint + load_param_into_net (examples/conformer/predict.py:66-67) for a module of this package.
    Returns (missing, unexpected) like torch's load_state_dict; raises on shape mismatches."""
    import torch

    raw = read_mindspore_ckpt(path)
    if _is_conv_tasnet(module):
        params = convert_conv_tasnet_names(raw)
    elif _is_deepspeech2(module):
        params = convert_deepspeech2_names(raw)
    elif _is_tasnet(module):
        params = convert_tasnet_names(raw)
    elif _is_wavegrad(module):
        params = convert_wavegrad_names(raw)
    elif _is_fastspeech2(module):
        params = convert_fastspeech2_names(raw)
    else:
        params = convert_ecapa_names(raw) if _is_ecapa(module) else convert_names(raw)
    own = module.state_dict()
    state, unexpected = {}, []
    for k, v in params.items():
        if k not in own:
            unexpected.append(k)
            continue
        t = torch.from_numpy(np.ascontiguousarray(v))
        if tuple(t.shape) != tuple(own[k].shape):
            raise ValueError("shape mismatch for %s: checkpoint %s, module %s" % (k, tuple(t.shape), tuple(own[k].shape)))
        state[k] = t.to(own[k].dtype)
    missing = [k for k in own if k not in state and not k.endswith("num_batches_tracked")]
    if _is_fastspeech2(module):  # a checkpoint without bins keeps the ones the module computed from `stats`
        missing = [k for k in missing if k not in ("variance_adaptor.pitch_bins", "variance_adaptor.energy_bins")]
    if strict and (missing or unexpected):
        raise KeyError("checkpoint does not match the module: missing %s, unexpected %s" % (missing[:8], unexpected[:8]))
    # (ConformerEncoder / CTC drop their bf16 / packed weight copies in load_state_dict post-hooks)
    module.load_state_dict(state, strict=False)
    return missing, unexpected
