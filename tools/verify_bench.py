#!/usr/bin/env python3
"""Stage times of the speaker-verification recipe (mindaudio_amd/ecapa/speaker_verification_cosine.py) at the VoxCeleb1-O shape:
about 4.7 k utterances, 37 720 trials, a cohort of 400 000 training embeddings, cohort_size 20 000, 192 dimensions.

  embeddings         EcapaTDNN forward over --utts utterances of --frames frames, 16 per batch (random features)
  running mean       emb_mean: three passes over the trial embeddings and one over the cohort
  cohort statistics  ma_cohort_stats_f32 (the hot path), quoted against the float32 matrix floor: 2 E N D flop at 155 TFLOP/s
  trial scores       ma_trial_scores_f32, s-norm
  host EER           metric.EER on the host (a host clock; the other stages are device events)

The scoring stages run on random embeddings with a speaker-cluster structure (the model's weights are random here, so its own
embeddings would not spread).  Each device stage: warm-up runs, then the median of --repeats runs timed with device events.

Reference baseline: a NumPy restatement of the example's evaluate2 loop (per trial: two cosine_similarity calls against the whole
cohort - each of which L2-normalises the cohort again, as sklearn does - two np.partition, mean, std) timed on the host over
--ref-trials trials and EXTRAPOLATED to the full trial list; the tool prints that it is extrapolated.

Not part of bench.py.  usage: python tools/verify_bench.py [--utts 4708 --trials 37720 --cohort 400000 --cohort-size 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 155e12  # measured v_mfma_f32_32x32x2_f32 rate of one MI355X, flop/s


def device_ms(fn, warmup, repeats):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def reference_trial_seconds(emb, cohort, enrol, test, k, n):
    """evaluate2's work for n trials, as the example does it (float32, one trial at a time)."""
    def cosine_similarity(x, y):
        xn = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), np.finfo(np.float32).tiny)
        yn = y / np.maximum(np.sqrt((y * y).sum(1, keepdims=True)), np.finfo(np.float32).tiny)
        return xn @ yn.T

    t0 = time.perf_counter()
    for i in range(n):
        e, t = emb[enrol[i]], emb[test[i]]
        se = np.squeeze(cosine_similarity(e.reshape(1, -1), cohort))
        se = np.partition(se, kth=-k)[-k:]
        me, sde = np.mean(se), np.std(se)
        st = np.squeeze(cosine_similarity(t.reshape(1, -1), cohort))
        st = np.partition(st, kth=-k)[-k:]
        mt, sdt = np.mean(st), np.std(st)
        s = cosine_similarity(e.reshape(1, -1), t.reshape(1, -1)).item()
        s = 0.5 * ((s - me) / sde + (s - mt) / sdt)
    return (time.perf_counter() - t0) / n, s


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--utts", type=int, default=4708)
    ap.add_argument("--trials", type=int, default=37720)
    ap.add_argument("--cohort", type=int, default=400000)
    ap.add_argument("--cohort-size", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=192)
    ap.add_argument("--frames", type=int, default=301)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--block-rows", type=int, default=None, help="query rows per pass of the cohort statistics (default: the library's 512)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ref-trials", type=int, default=3)
    ap.add_argument("--skip-embeddings", action="store_true")
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd import ops
    from mindaudio_amd.metric import EER
    from mindaudio_amd.models import EcapaTDNN

    if not torch.cuda.is_available():
        raise SystemExit("verify_bench needs a HIP device: there is nothing to measure without one")
    E, N, K, D, T = a.utts, a.cohort, a.cohort_size, a.dim, a.trials
    g = torch.Generator(device="cuda").manual_seed(1)
    n_spk = max(E // 4, 2)
    centres = torch.randn(n_spk, D, device="cuda", generator=g)
    spk = torch.randint(0, n_spk, (E,), device="cuda", generator=g)
    emb = centres[spk] + 1.5 * torch.randn(E, D, device="cuda", generator=g) + 0.5
    cc = torch.randn(6000, D, device="cuda", generator=g)
    cohort = cc[torch.randint(0, 6000, (N,), device="cuda", generator=g)] + 1.5 * torch.randn(N, D, device="cuda", generator=g) + 0.5
    enrol = torch.randint(0, E, (T,), device="cuda", generator=g)
    test = torch.where(torch.rand(T, device="cuda", generator=g) < 0.5, enrol.roll(1), torch.randint(0, E, (T,), device="cuda", generator=g))
    labels = (spk[enrol] == spk[test]).cpu().numpy()

    rows = []
    if not a.skip_embeddings:
        c = a.channels
        model = EcapaTDNN(80, channels=(c, c, c, c, 3 * c), lin_neurons=D).cuda().eval()
        feats = torch.randn(16, a.frames, 80, device="cuda", generator=g)
        n_batches = -(-E // 16)

        def embed():
            for _ in range(n_batches):
                model(feats)
        ms = device_ms(embed, 1, max(a.repeats // 2, 3))
        rows.append(("embeddings (%d x %d frames, C = %d)" % (n_batches * 16, a.frames, c), ms))

    state = {}

    def mean_sub():
        gm, cnt = None, 0
        for _ in range(3):
            y, gm, cnt = ops.running_mean_sub(emb, gm, cnt)
        cy, gm, cnt = ops.running_mean_sub(cohort, gm, cnt)
        state["emb"], state["cohort"] = y, cy
    rows.append(("running mean (3 x %d + %d rows)" % (E, N), device_ms(mean_sub, a.warmup, a.repeats)))

    def stats():
        state["mean"], state["std"] = ops.cohort_stats(state["emb"], state["cohort"], K, block_rows=a.block_rows)
    ms_stats = device_ms(stats, a.warmup, a.repeats)
    rows.append(("cohort statistics (%d x %d, K = %d)" % (E, N, K), ms_stats))

    def score():
        state["scores"] = ops.trial_scores(state["emb"], enrol, test, state["mean"], state["std"], "s-norm")
    rows.append(("trial scores (%d, s-norm)" % T, device_ms(score, a.warmup, a.repeats)))

    sc = state["scores"].cpu().numpy()
    host = []
    for _ in range(max(a.repeats // 2, 3)):
        t0 = time.perf_counter()
        eer = EER(sc[labels], sc[~labels])
        host.append(1e3 * (time.perf_counter() - t0))
    rows.append(("host EER (%d scores)" % T, (float(np.median(host)), min(host), max(host))))

    per_trial, s_ref = reference_trial_seconds(state["emb"].cpu().numpy(), state["cohort"].cpu().numpy(), enrol.cpu().numpy(),
                                               test.cpu().numpy(), K, a.ref_trials)
    ref_ms = 1e3 * per_trial * T
    floor_ms = 1e3 * 2.0 * E * N * D / F32_MATRIX_PEAK
    print("stage                                              median ms      min      max")
    for name, (med, lo, hi) in rows:
        print("%-50s %9.3f %8.3f %8.3f" % (name, med, lo, hi))
    print("cohort statistics vs the float32 matrix floor (%.2f ms for 2 E N D = %.3f Tflop at 155 TFLOP/s): %.2f x"
          % (floor_ms, 2.0 * E * N * D / 1e12, ms_stats[0] / floor_ms))
    print("reference evaluate2 loop on this host: %.3f s per trial over %d timed trials -> %.0f s for %d trials (EXTRAPOLATED, not run)"
          % (per_trial, a.ref_trials, ref_ms / 1e3, T))
    print("last timed reference trial: score %.6f, device %.6f" % (s_ref, sc[a.ref_trials - 1]))
    scoring = sum(med for name, (med, _, _) in rows if not name.startswith("embeddings"))
    print(json.dumps({"utts": E, "trials": T, "cohort": N, "cohort_size": K, "dim": D, "eer": float(eer),
                      "stages_ms": {name: med for name, (med, _, _) in rows}, "scoring_ms": scoring,
                      "cohort_stats_floor_ms": floor_ms, "reference_loop_ms_extrapolated": ref_ms,
                      "reference_trials_timed": a.ref_trials}))


if __name__ == "__main__":
    main()
