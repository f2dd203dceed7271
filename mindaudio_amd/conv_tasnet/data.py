"""The segment list of the Conv-TasNet example's evaluation data (what examples/conv_tasnet/data.py produces, without MindSpore).

`mix_clean.json`, `s1.json` and `s2.json` each hold [wav path, #samples] pairs.  The behaviour restated here, pinned by
tests/test_conv_tasnet_cpu.py:
  * each list is ordered longest first, entries of equal length keeping their file order (the three lists hold the same lengths, so
    position i of each names one utterance);
  * an utterance shorter than one segment is dropped; the others are cut into floor(len / segment) back-to-back segments plus, when a
    remainder is left, one more that holds the LAST segment samples (it overlaps its predecessor);
  * utterances are taken in groups whose segment count stays within `batch_size`: an utterance that would overflow a group closes it
    and opens the next; one that overflows an empty group - more segments than `batch_size` on its own - is left out altogether.
    Grouping changes which utterances appear, not their order.
Host-side NumPy; the wavs are read once each."""
import json
import os

import numpy as np

from ..data import io

__all__ = ["DatasetGenerator", "plan_groups", "segment_starts"]

_LISTS = ("mix_clean.json", "s1.json", "s2.json")


def segment_starts(n_samples, seg):
    """First sample of every segment of an utterance of n_samples >= seg."""
    starts = list(range(0, n_samples - seg + 1, seg))
    if n_samples % seg:
        starts.append(n_samples - seg)
    return starts


def plan_groups(lengths, seg, limit):
    """Positions (into `lengths`, already ordered) of the utterances of each group, under the rule in the module docstring."""
    groups, pos = [], 0
    while pos < len(lengths):
        first, members, count = pos, [], 0
        while pos < len(lengths) and count < limit:
            if lengths[pos] >= seg:
                count += len(segment_starts(lengths[pos], seg))
                if count > limit:
                    pos += pos == first  # alone too large: passed over; otherwise it opens the next group
                    break
                members.append(pos)
            pos += 1
        if members:
            groups.append(members)
    return groups


class DatasetGenerator:
    """DatasetGenerator(json_dir, batch_size, sample_rate=8000, segment=4.0): item i is (mixture (seg,) float32, seg,
    sources (2, seg) float32), seg = int(segment * sample_rate).  `segment` must be positive (the reference's full-utterance mode,
    segment = -1, is not built).  `dropped` counts the utterances shorter than one segment; the reference's line about them goes to
    `log`."""

    def __init__(self, json_dir, batch_size, sample_rate=8000, segment=4.0, cv_maxlen=8.0, log=print):
        seg = int(segment * sample_rate)
        if seg <= 0:
            raise NotImplementedError("segment must be positive: the full-utterance mode is not built")
        mix, s1, s2 = (self._ordered(os.path.join(json_dir, name)) for name in _LISTS)
        lengths = [n for _, n in mix]
        if [n for _, n in s1] != lengths or [n for _, n in s2] != lengths:
            raise ValueError("mix_clean.json, s1.json and s2.json do not list the same lengths")
        short = [n for n in lengths if n < seg]
        self.dropped = len(short)
        log("Drop {} utts({:.2f} h) which is short than {} samples".format(self.dropped, sum(short) / sample_rate / 36000, seg))
        self.items = []
        for group in plan_groups(lengths, seg, batch_size):
            for u in group:
                waves = [np.asarray(io.read(infos[u][0])[0]) for infos in (mix, s1, s2)]
                if any(w.ndim != 1 or w.shape[0] != lengths[u] for w in waves):
                    raise ValueError("%s: not a mono file of the listed %d samples" % (mix[u][0], lengths[u]))
                both = np.stack(waves[1:]).astype(np.float32)
                for a in segment_starts(lengths[u], seg):
                    self.items.append((waves[0][a:a + seg].astype(np.float32), seg, both[:, a:a + seg]))

    @staticmethod
    def _ordered(path):
        with open(path) as fh:
            entries = [(p, int(n)) for p, n in json.load(fh)]
        return sorted(entries, key=lambda e: -e[1])  # stable: equal lengths keep their file order

    def __getitem__(self, index):
        return self.items[index]

    def __len__(self):
        return len(self.items)
