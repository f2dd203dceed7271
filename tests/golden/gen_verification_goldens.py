#!/usr/bin/env python3
"""Golden results of the speaker-verification scoring: the reference's own functions run in THIS container.

  mindaudio/metric/eer.py::get_eer_from_scores          loaded by path (sklearn and scipy are installed here)
  examples/ECAPA-TDNN/speaker_verification_cosine.py::evaluate, evaluate2, EER, emb_mean
      the script cannot be imported (mindspore, wget, import-time argparse), so only these `def`s are compiled from its syntax
      tree at run time, into a namespace holding np, cosine, cosine_similarity, get_eer_from_scores, datetime and a silent print.
      No text of the reference is written anywhere.  The namespace's `np` forwards to NumPy and records what evaluate2 hands to
      np.mean / np.std: that is how the per-utterance cohort statistics of the reference are captured.

Writes tests/golden/verification_goldens.npz: seeds, shapes and results only.  The inputs are rebuilt from
numpy.random.RandomState(seed) by the `make_*` functions below, which the tests load from this file (they need neither the
reference nor sklearn).  Every case is run on float32 inputs (what the example computes) and on the same inputs cast to float64;
`tol_<family>` = 4 x the largest |float32 result - float64 result| of the reference over the family (the factor 4 because the
device's summation order differs from BLAS's):

  tol_mean / tol_std                cohort statistics with K > 2
  tol_mean_smallk / tol_std_smallk  K <= 2 (the statistic is one or two raw scores)
  tol_score_raw                     un-normalised trial scores
  tol_score_norm                    z- / t- / s-normalised trial scores
  tol_emb_mean                      emb_mean outputs and running mean

The reference cannot run N = 1 (np.partition of the 0-d array np.squeeze leaves raises), so no statistics golden has N = 1; the
GPU test covers it with its float64 restatement.  sklearn / scipy / numpy versions are recorded in the file.

tests/golden/ecapa_param_names.txt (the reference-side parameter names of EcapaTDNN, one per line with its shape for the
C = 512 default) is NOT produced here: it is hand-derived by reading mindaudio/models/ecapatdnn.py and cannot be verified without
MindSpore, which is not installed in this container.

usage: python tests/golden/gen_verification_goldens.py
"""
import ast
import datetime
import os
import tempfile
import types
import warnings

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

# ---- inputs (shared with the tests) ---------------------------------------------------------------------------------------------
EER_CASES = [  # (name, seed)
    ("overlap", 11), ("separable", 12), ("rounded", 13), ("one_positive", 14), ("all_equal", 15), ("overlap_large", 16),
    ("no_negative", 17),
]


def make_eer_case(name, seed):
    """(scores float64, labels int) of one EER case."""
    rng = np.random.RandomState(seed)
    if name in ("overlap", "overlap_large"):
        n = 400 if name == "overlap" else 5000
        labels = (rng.rand(n) < 0.3).astype(np.int64)
        scores = rng.randn(n) + 1.5 * labels
    elif name == "separable":
        labels = (rng.rand(300) < 0.4).astype(np.int64)
        scores = rng.rand(300) + 2.0 * labels
    elif name == "rounded":  # heavy ties
        labels = (rng.rand(600) < 0.3).astype(np.int64)
        scores = np.round(0.4 * rng.randn(600) + 0.5 * labels, 1)
    elif name == "one_positive":
        labels = np.zeros(21, np.int64)
        labels[rng.randint(0, 21)] = 1
        scores = rng.randn(21)
    elif name == "all_equal":
        labels = (rng.rand(50) < 0.5).astype(np.int64)
        scores = np.full(50, 0.25)
    elif name == "no_negative":
        labels = np.ones(30, np.int64)
        scores = rng.randn(30)
    else:
        raise KeyError(name)
    return scores.astype(np.float64), labels


def clustered(rng, n, d, centres, spread=2.0):
    """Gaussian clusters around `centres` (S, d): speaker-like structure, so that the largest cohort scores are not noise."""
    return (centres[rng.randint(0, centres.shape[0], n)] + spread * rng.randn(n, d)).astype(np.float32)


# (seed, E, N, D, K, kind): kind 0 plain, 1 duplicated cohort rows tying across the K-th position of query 0, 2 a zero-norm query
# (row 1 % E), 3 a zero-norm cohort row
STATS_CASES = (
    [(100 + 10 * i + j, 7, n, d, k, 0) for i, (n, d) in enumerate([(63, 32), (63, 192), (63, 512), (4097, 32), (4097, 192), (4097, 512)])
     for j, k in enumerate((1, 2))]
    + [(200, 300, 63, 192, 1, 0), (201, 300, 63, 192, 2, 0), (202, 1, 63, 32, 1, 0), (203, 7, 63, 512, 3, 0),
       (204, 7, 63, 192, 62, 0), (205, 7, 63, 32, 63, 0), (206, 1, 4097, 192, 204, 0), (207, 7, 4097, 512, 4096, 0),
       (208, 300, 4097, 192, 204, 0), (209, 7, 50000, 192, 2500, 0), (210, 300, 50000, 192, 2500, 0),
       (211, 7, 50000, 32, 50000, 0), (212, 7, 50000, 512, 49999, 0), (213, 7, 4097, 192, 204, 1), (214, 7, 4097, 192, 204, 2),
       (215, 7, 63, 192, 3, 3), (216, 7, 4097, 32, 4097, 1), (217, 300, 4097, 512, 204, 3)]
)


def make_stats_case(seed, E, N, D, K, kind):
    """(queries (E, D) float32, cohort (N, D) float32) of one cohort-statistics case."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(24, D)
    q = clustered(rng, E, D, centres)
    c = clustered(rng, N, D, centres)
    if kind == 1 and N >= 8:
        q0 = q[0].astype(np.float64)
        cd = c.astype(np.float64)
        s = (cd @ q0) / np.linalg.norm(cd, axis=1)
        order = np.argsort(-s, kind="stable")
        kth = order[K - 1]
        for r in range(max(K - 3, 0), min(K + 3, N)):  # ranks K-2 .. K+3 now hold the same row: the tie straddles position K
            c[order[r]] = c[kth]
    elif kind == 2:
        q[1 % E] = 0
    elif kind == 3:
        c[N // 2] = 0
    return q, c


# (seed, E, N, D, K or 0 = no cohort_size, n_trials)
TRIAL_CASES = [(300, 60, 500, 192, 50, 240), (301, 33, 257, 64, 0, 150), (302, 90, 1000, 512, 100, 300)]
TRIAL_MODES = ("none", "z-norm", "t-norm", "s-norm")


def make_trial_case(seed, E, N, D, K, n_trials):
    """(embeddings (E, D) f32, cohort (N, D) f32, labels, enrol index, test index) of one evaluate2 case: 6 utterances per speaker."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(max(E // 6, 2), D)
    spk = np.arange(E) % centres.shape[0]
    emb = (centres[spk] + 1.2 * rng.randn(E, D)).astype(np.float32)
    cohort = clustered(rng, N, D, rng.randn(40, D), 1.2)
    enrol = rng.randint(0, E, n_trials)
    test = rng.randint(0, E, n_trials)
    test[test == enrol] = (test[test == enrol] + 1) % E
    labels = (spk[enrol] == spk[test]).astype(np.int64)
    return emb, cohort, labels, enrol, test


def trial_lines(labels, enrol, test):
    return ["%d utt%05d.wav utt%05d.wav\n" % (lab, e, t) for lab, e, t in zip(labels, enrol, test)]


# (seed, N1, N2, D, rows stored per call or 0 = all): three chained calls over X1, a fourth over X2
EMB_MEAN_CASES = [(400, 40, 60, 32, 0), (401, 1, 1, 64, 0), (402, 700, 1000, 192, 24)]


def make_emb_mean_case(seed, N1, N2, D, _rows):
    rng = np.random.RandomState(seed)
    off = rng.randn(D)
    return (off + rng.randn(N1, D)).astype(np.float32), (off + rng.randn(N2, D)).astype(np.float32)


def stored_rows(n, rows):
    return np.arange(n) if rows == 0 or rows >= n else np.linspace(0, n - 1, rows).astype(np.int64)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
class _RecordingNp:
    """Forwards to NumPy; remembers the results of mean / std (evaluate2's cohort statistics)."""

    def __init__(self):
        self.means, self.stds = [], []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, a, *args, **kw):
        r = np.mean(a, *args, **kw)
        self.means.append(float(r))
        return r

    def std(self, a, *args, **kw):
        r = np.std(a, *args, **kw)
        self.stds.append(float(r))
        return r


def load_reference_functions():
    import importlib.util

    from scipy.spatial.distance import cosine
    from sklearn.metrics.pairwise import cosine_similarity

    spec = importlib.util.spec_from_file_location("ref_eer", os.path.join(REF, "mindaudio/metric/eer.py"))
    eer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eer)
    path = os.path.join(REF, "examples/ECAPA-TDNN/speaker_verification_cosine.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    rec = _RecordingNp()
    ns = {"np": rec, "cosine": cosine, "cosine_similarity": cosine_similarity, "get_eer_from_scores": eer.get_eer_from_scores,
          "datetime": datetime, "print": lambda *a, **k: None}
    wanted = {"evaluate", "evaluate2", "EER", "emb_mean"}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in wanted:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    assert wanted <= set(ns)
    return eer, ns, rec


def _run_evaluate2(ns, rec, emb, cohort, lines, score_norm, cohort_size):
    d = {"utt%05d" % i: emb[i] for i in range(emb.shape[0])}
    params = types.SimpleNamespace()
    if score_norm != "none":
        params.score_norm = score_norm
    if cohort_size:
        params.cohort_size = cohort_size
    rec.means, rec.stds = [], []
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.writelines(lines)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pos, neg = ns["evaluate2"](d, d, cohort, params, f.name)
    finally:
        os.unlink(f.name)
    return np.asarray(pos, np.float64), np.asarray(neg, np.float64)


def main():
    import scipy
    import sklearn

    eer, ns, rec = load_reference_functions()
    out = {"versions": np.array([sklearn.__version__, scipy.__version__, np.__version__])}
    tol = {}

    def bump(family, a, b):
        d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
        d = d[np.isfinite(d)]
        if d.size:
            tol[family] = max(tol.get(family, 0.0), float(d.max()))

    # EER
    for name, seed in EER_CASES:
        scores, labels = make_eer_case(name, seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                e, th = eer.get_eer_from_scores(scores, labels)
                out["eer_%s" % name] = np.array([e, th])
                out["eer_%s_raises" % name] = np.array("")
            except Exception as exc:  # the golden records the exception type
                out["eer_%s" % name] = np.array([np.nan, np.nan])
                out["eer_%s_raises" % name] = np.array(type(exc).__name__)
            pos, neg = scores[labels == 1], scores[labels == 0]
            if pos.size and neg.size:
                out["EER_%s" % name] = np.float64(ns["EER"](pos, neg))
        print("eer", name, out["eer_%s" % name], out["eer_%s_raises" % name], out.get("EER_%s" % name))

    # cohort statistics through evaluate2 (z-norm; the scores themselves are not kept)
    for i, (seed, E, N, D, K, kind) in enumerate(STATS_CASES):
        q, c = make_stats_case(seed, E, N, D, K, kind)
        pairs = [(a, min(a + 1, E - 1)) for a in range(0, E, 2)]
        lines = trial_lines([1] * len(pairs), [p[0] for p in pairs], [p[1] for p in pairs])
        res = {}
        for tag, cast in (("32", np.float32), ("64", np.float64)):
            _run_evaluate2(ns, rec, q.astype(cast), c.astype(cast), lines, "z-norm", K)
            mean, std = np.zeros(E), np.zeros(E)
            for t, (a, b) in enumerate(pairs):  # evaluate2 takes enrol's statistics, then test's
                mean[a], std[a] = rec.means[2 * t], rec.stds[2 * t]
                mean[b], std[b] = rec.means[2 * t + 1], rec.stds[2 * t + 1]
            res[tag] = (mean, std)
            out["stats%d_mean%s" % (i, tag)] = mean
            out["stats%d_std%s" % (i, tag)] = std
        small = "_smallk" if K <= 2 else ""
        bump("mean" + small, res["32"][0], res["64"][0])
        bump("std" + small, res["32"][1], res["64"][1])
        print("stats", i, (seed, E, N, D, K, kind), "diff mean %.2e std %.2e" % (
            np.abs(res["32"][0] - res["64"][0]).max(), np.abs(res["32"][1] - res["64"][1]).max()), flush=True)
    out["stats_cases"] = np.array(STATS_CASES, np.int64)

    # trial scores: evaluate2 in every mode, evaluate
    for i, (seed, E, N, D, K, n_trials) in enumerate(TRIAL_CASES):
        emb, cohort, labels, enrol, test = make_trial_case(seed, E, N, D, K, n_trials)
        lines = trial_lines(labels, enrol, test)
        for mode in TRIAL_MODES:
            r = {}
            for tag, cast in (("32", np.float32), ("64", np.float64)):
                r[tag] = _run_evaluate2(ns, rec, emb.astype(cast), cohort.astype(cast), lines, mode, K)
                out["trial%d_%s_pos%s" % (i, mode, tag)] = r[tag][0]
                out["trial%d_%s_neg%s" % (i, mode, tag)] = r[tag][1]
            fam = "score_raw" if mode == "none" else "score_norm"
            bump(fam, r["32"][0], r["64"][0])
            bump(fam, r["32"][1], r["64"][1])
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            f.writelines(lines)
        d32 = {"utt%05d" % k: emb[k] for k in range(E)}
        out["trial%d_evaluate_eer" % i] = np.float64(ns["evaluate"](d32, d32, f.name))
        os.unlink(f.name)
        print("trial", i, "eer", out["trial%d_evaluate_eer" % i], flush=True)
    out["trial_cases"] = np.array(TRIAL_CASES, np.int64)

    # emb_mean: three chained calls over X1, a fourth over X2
    for i, (seed, N1, N2, D, rows) in enumerate(EMB_MEAN_CASES):
        x1, x2 = make_emb_mean_case(seed, N1, N2, D, rows)
        r = {}
        for tag, cast in (("32", np.float32), ("64", np.float64)):
            g, cnt, ys = np.zeros(1, cast), 0, []
            for call, x in enumerate((x1, x1, x1, x2)):
                d = {k: x[k].astype(cast) for k in range(x.shape[0])}
                dm, g, cnt = ns["emb_mean"](g, cnt, d)
                y = np.stack([dm[k] for k in range(x.shape[0])])
                ys.append(y[stored_rows(x.shape[0], rows)].astype(np.float64))
                out["embmean%d_y%d_%s" % (i, call, tag)] = ys[-1] if tag == "64" else ys[-1].astype(np.float32)
                out["embmean%d_g%d_%s" % (i, call, tag)] = np.asarray(g, np.float64)
            out["embmean%d_count" % i] = np.int64(cnt)
            r[tag] = (ys, g)
        for a, b in zip(r["32"][0], r["64"][0]):
            bump("emb_mean", a, b)
        bump("emb_mean", r["32"][1], r["64"][1])
    out["emb_mean_cases"] = np.array(EMB_MEAN_CASES, np.int64)

    for k, v in tol.items():
        out["tol_" + k] = np.float64(4.0 * v)
        print("tol_%s = %.3e" % (k, 4.0 * v))
    path = os.path.join(HERE, "verification_goldens.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
