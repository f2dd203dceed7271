#!/usr/bin/env python3
"""Generate tests/golden/fastspeech2_symbols.txt: the names in THE REFERENCE's `all_symbols` (examples/fastspeech2/text/symbols.py), one
per line in id order, and tests/golden/fastspeech2_ids.json: the ids its `text_to_sequence` gives for a few phoneme strings.

Runs only where the reference tree exists; nothing of it travels - the `text` package is imported from the example's directory and
only the list of names and the recorded ids are stored.  The space symbol is written as the word <space> (a line cannot end in one).

usage: python tests/golden/gen_fastspeech2_symbols.py <reference root>   (or MINDAUDIO_REFERENCE=<reference root>)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PHRASES = ["{HH AH0 L OW1}", "{HH AH0 L OW1 sp W ER1 L D}", "{sil}"]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MINDAUDIO_REFERENCE")
    if not root:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.join(root, "examples", "fastspeech2"))
    import types

    for name, attrs in (("unidecode", {"unidecode": lambda s: s}), ("inflect", {"engine": lambda: None})):
        try:  # the cleaners' imports; with cleaner_names = [] none of them is called
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    from text import text_to_sequence
    from text.symbols import all_symbols

    assert len(set(all_symbols)) == len(all_symbols) and not any("\n" in s or s == "<space>" for s in all_symbols)
    with open(os.path.join(HERE, "fastspeech2_symbols.txt"), "w") as fh:
        for s in all_symbols:
            fh.write(("<space>" if s == " " else s) + "\n")
    with open(os.path.join(HERE, "fastspeech2_ids.json"), "w") as fh:
        json.dump({p: [int(i) for i in text_to_sequence(p, [])] for p in PHRASES}, fh, indent=1)
        fh.write("\n")
    print("%d symbols" % len(all_symbols))


if __name__ == "__main__":
    main()
