"""mindaudio/models/decoders/greedydecoder.py: MSGreedyDecoder.  The per-frame arg-max runs on the device
(ma_ctc_greedy_search_f32's `best`; the arg-max of log_softmax(p) is the arg-max of p, first index on ties as np.argmax); the string
work is host logic.  The reference imports the `Levenshtein` module for its error counts; here they come from metric.wer's edit
distance."""
import numpy as np

from ...metric.wer import edit_distance

__all__ = ["Decoder", "GreedyDecoder", "MSGreedyDecoder"]


class Decoder:
    def __init__(self, labels, blank_index=0):
        self.labels = labels
        self.int_to_char = {i: c for (i, c) in enumerate(labels)}
        self.blank_index = blank_index
        space_index = len(labels)  # an out-of-bounds index when there is no space label
        if " " in labels:
            space_index = labels.index(" ")
        self.space_index = space_index

    def wer(self, s1, s2):
        """Word-level edit distance (a count, not a rate) between two space-separated sentences."""
        return edit_distance(s1.split(), s2.split())

    def cer(self, s1, s2):
        """Character-level edit distance (a count) with the spaces removed."""
        return edit_distance(s1.replace(" ", ""), s2.replace(" ", ""))

    def decode(self, probs, sizes=None):
        raise NotImplementedError


class GreedyDecoder(Decoder):
    def convert_to_strings(self, sequences, sizes=None, remove_repetitions=False, return_offsets=False):
        strings = []
        offsets = [] if return_offsets else None
        for x in range(len(sequences)):
            seq_len = sizes[x] if sizes is not None else len(sequences[x])
            string, string_offsets = self.process_string(sequences[x], seq_len, remove_repetitions)
            strings.append([string])  # one path only
            if return_offsets:
                offsets.append([string_offsets])
        if return_offsets:
            return strings, offsets
        return strings


class MSGreedyDecoder(GreedyDecoder):
    def process_string(self, sequence, size, remove_repetitions=False):
        """Blanks are dropped; with remove_repetitions a character equal to the PREVIOUS FRAME's character is dropped (so `A _ A` keeps
        both and `A A` collapses); the space label becomes " "."""
        string = ""
        offsets = []
        blank = self.int_to_char[self.blank_index]
        space = self.labels[self.space_index] if self.space_index < len(self.labels) else None
        for i in range(int(size)):
            char = self.int_to_char[int(sequence[i])]
            if char != blank:
                if remove_repetitions and i != 0 and char == self.int_to_char[int(sequence[i - 1])]:
                    pass
                elif char == space:
                    string += " "
                    offsets.append(i)
                else:
                    string = string + char
                    offsets.append(i)
        return string, offsets

    def argmax(self, probs):
        """(B, T, C) probabilities -> (B, T) int arg-max: on the device for a device tensor, np.argmax for NumPy."""
        if isinstance(probs, np.ndarray):
            return np.argmax(probs, axis=-1)
        from ... import ops

        B, T, C = probs.shape
        p = probs.contiguous().reshape(B * T, C)
        best, _, _, _ = ops.ctc_greedy_search(p, B, T, C, None, self.blank_index)
        return best.cpu().numpy()

    def decode(self, probs, sizes=None):
        max_probs = self.argmax(probs)
        if sizes is not None:
            sizes = np.asarray(sizes.detach().cpu() if hasattr(sizes, "detach") else sizes)
        return self.convert_to_strings(max_probs, sizes, remove_repetitions=True, return_offsets=True)
