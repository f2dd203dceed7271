"""FastSpeech2 example (examples/fastspeech2/generate.py): ids / phonemes / text -> mel, optionally -> audio through WaveGrad.
Run as `python -m mindaudio_amd.fastspeech2.generate`."""
