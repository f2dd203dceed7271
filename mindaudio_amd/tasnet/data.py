"""The utterance list of the TasNet example's evaluation data (what examples/tasnet/data.py produces, without MindSpore).

`mix_clean.json`, `s1.json` and `s2.json` each hold [wav path, #samples] pairs.  The behaviour restated here, pinned by
tests/test_tasnet_cpu.py:
  * each list is ordered by (#samples, path), DESCENDING - the longest first, equal lengths in reverse path order - and position i of
    the three lists names one utterance (their lengths must agree);
  * every utterance is zero-padded to 3320 segments of L samples (132 800 samples at the example's L = 40) and reshaped to (3320, L);
    the two sources are stacked to (2, 3320, L);
  * the length that travels with an item is the number of SEGMENTS, always 3320 (`mix.shape[0]` of the padded array), not the
    utterance's own length: the reference's loss therefore never masks anything.
The reference groups utterances by `batch_size` only to pad each group to its longest member; every member already has the same shape,
so the grouping has no effect and is not restated.  Host-side NumPy; the wavs are read once each."""
import json
import os

import numpy as np

from ..data import io

__all__ = ["DatasetGenerator", "SEGMENTS"]

SEGMENTS = 3320  # data.py:104-111: pad_len = 132800 = 3320 * 40
_LISTS = ("mix_clean.json", "s1.json", "s2.json")


class DatasetGenerator:
    """DatasetGenerator(json_dir, batch_size, sample_rate=8000, L=40, segments=3320): item i is (mixture (segments, L) float32,
    segments, sources (2, segments, L) float32).  `segments` is this package's addition (the reference hard-codes 3320 and, with it,
    L = 40).  An utterance longer than segments * L samples raises ValueError (the reference fails on a negative pad length)."""

    def __init__(self, json_dir, batch_size, sample_rate=8000, L=int(8000 * 0.005), segments=SEGMENTS):
        self.batch_size, self.sample_rate, self.L, self.segments = batch_size, sample_rate, L, segments
        mix, s1, s2 = (self._ordered(os.path.join(json_dir, name)) for name in _LISTS)
        if not len(mix) == len(s1) == len(s2):
            raise ValueError("mix_clean.json, s1.json and s2.json do not list the same number of utterances")
        pad_len = segments * L
        self.mixture, self.len, self.sources = [], [], []
        for infos in zip(mix, s1, s2):
            if not infos[0][1] == infos[1][1] == infos[2][1]:
                raise ValueError("mix_clean.json, s1.json and s2.json do not list the same lengths")
            rows = []
            for path, _ in infos:
                w = np.asarray(io.read(path)[0], np.float32)
                if w.ndim != 1 or w.shape[0] > pad_len:
                    raise ValueError("%s: not a mono file of at most %d samples" % (path, pad_len))
                rows.append(np.concatenate([w, np.zeros((pad_len - w.shape[0],), np.float32)]).reshape(segments, L))
            self.mixture.append(rows[0])
            self.len.append(segments)
            self.sources.append(np.stack(rows[1:]))

    @staticmethod
    def _ordered(path):
        with open(path) as fh:
            entries = [(p, int(n)) for p, n in json.load(fh)]
        return sorted(entries, key=lambda e: (e[1], e[0]), reverse=True)

    def __getitem__(self, index):
        return self.mixture[index], self.len[index], self.sources[index]

    def __len__(self):
        return len(self.mixture)
