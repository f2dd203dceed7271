"""GPU: cohort statistics, running-mean subtraction, trial scores and the ECAPA verification recipe end to end, against the
reference's own results (tests/golden/verification_goldens.npz) and float64 restatements written here.

Tolerances are the generator's: 4 x the largest |float32 - float64| difference of the REFERENCE over each case family (see
tests/golden/gen_verification_goldens.py); none comes from the kernels.  Every test prints its figures before it asserts."""
import importlib.util
import os
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_verification_goldens", os.path.join(GOLDEN, "gen_verification_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "verification_goldens.npz"))


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- float64 restatements --------------------------------------------------------------------------------------------------------
def _unit(x):
    x = np.asarray(x, np.float64)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return np.divide(x, n, out=np.zeros_like(x), where=n > 0)


def _stats64(q, c, k):
    s = _unit(q) @ _unit(c).T
    top = np.partition(s, -k, axis=1)[:, -k:]
    return top.mean(1), top.std(1)


def _emb_mean64(g, cnt, x):
    y = np.empty_like(x)
    for i in range(x.shape[0]):
        if cnt == 0:
            g = x[i].copy()
        else:
            w = 1 / (cnt + 1)
            g = (1 - w) * g + w * x[i]
        y[i] = x[i] - g
        cnt += 1
    return y, g, cnt


def _norm64(s, me, se, mt, st, mode):
    if mode == "z-norm":
        return (s - me) / se
    if mode == "t-norm":
        return (s - mt) / st
    if mode == "s-norm":
        return 0.5 * ((s - me) / se + (s - mt) / st)
    return s


def _tols(gold, k):
    small = "_smallk" if k <= 2 else ""
    return float(gold["tol_mean" + small]), float(gold["tol_std" + small])


# ---- cohort statistics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(GEN.STATS_CASES)))
def test_cohort_stats_matches_reference(gold, i):
    from mindaudio_amd import ops

    seed, E, N, D, K, kind = GEN.STATS_CASES[i]
    assert tuple(gold["stats_cases"][i]) == (seed, E, N, D, K, kind)
    q, c = GEN.make_stats_case(seed, E, N, D, K, kind)
    mean, std = ops.cohort_stats(_dev(q), _dev(c), K)
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    tm, ts = _tols(gold, K)
    em = np.abs(mean - gold["stats%d_mean64" % i]).max()
    es = np.abs(std - gold["stats%d_std64" % i]).max()
    wm, wsd = _stats64(q, c, K)
    rm, rs = np.abs(mean - wm).max(), np.abs(std - wsd).max()
    print("case", GEN.STATS_CASES[i], "vs reference f64: mean %.3e (tol %.3e) std %.3e (tol %.3e); vs restatement: %.3e %.3e"
          % (em, tm, es, ts, rm, rs))
    assert em <= tm and es <= ts
    assert rm <= tm and rs <= ts


GRID_E, GRID_N, GRID_D = (1, 7, 300), (1, 63, 4097, 50000), (32, 192, 512)


def _grid_ks(n):
    return sorted({k for k in (1, 2, n // 20, n - 1, n) if 1 <= k <= n})


@pytest.mark.parametrize("N", GRID_N)
@pytest.mark.parametrize("D", GRID_D)
def test_cohort_stats_grid(gold, N, D):
    """Every E x K of the grid at this (N, D), none of them tile multiples, against the float64 np.partition restatement."""
    from mindaudio_amd import ops

    worst = {}
    failures = []
    for E in GRID_E:
        rng = np.random.RandomState(1000 + 7 * N + D + E)
        centres = rng.randn(24, D)
        q = GEN.clustered(rng, E, D, centres)
        c = GEN.clustered(rng, N, D, centres)
        qd, cd = _dev(q), _dev(c)
        s = _unit(q) @ _unit(c).T
        for K in _grid_ks(N):
            mean, std = ops.cohort_stats(qd, cd, K)
            top = np.partition(s, -K, axis=1)[:, -K:]
            em = np.abs(mean.cpu().numpy() - top.mean(1)).max()
            es = np.abs(std.cpu().numpy() - top.std(1)).max()
            tm, ts = _tols(gold, K)
            print("E %d N %d K %d D %d: mean %.3e (tol %.3e) std %.3e (tol %.3e)" % (E, N, K, D, em, tm, es, ts))
            fam = "smallk" if K <= 2 else "large"
            w = worst.get(fam, (0.0, 0.0))
            worst[fam] = (max(w[0], em / tm), max(w[1], es / ts))
            if not (em <= tm and es <= ts):
                failures.append((E, N, K, D, em, es))
    print("worst error / tolerance per family:", worst)
    assert not failures, failures


@pytest.mark.parametrize("kind", (1, 2, 3))
def test_cohort_stats_ties_and_zero_rows(gold, kind):
    """Planted duplicates tying across the K-th position (query 0), a zero-norm query, a zero-norm cohort row."""
    from mindaudio_amd import ops

    for seed, E, N, D, K in ((31, 7, 4097, 192, 204), (32, 300, 50000, 192, 2500), (33, 7, 63, 512, 3), (34, 7, 4097, 32, 4096)):
        q, c = GEN.make_stats_case(seed, E, N, D, K, kind)
        mean, std = ops.cohort_stats(_dev(q), _dev(c), K)
        mean, std = mean.cpu().numpy(), std.cpu().numpy()
        wm, wsd = _stats64(q, c, K)
        tm, ts = _tols(gold, K)
        print("kind", kind, (E, N, D, K), "mean %.3e (tol %.3e) std %.3e (tol %.3e)" % (np.abs(mean - wm).max(), tm,
                                                                                       np.abs(std - wsd).max(), ts))
        assert np.abs(mean - wm).max() <= tm and np.abs(std - wsd).max() <= ts
        if kind == 1:  # the tie really straddles position K for query 0
            s0 = np.sort((_unit(q[:1]) @ _unit(c).T)[0])[::-1]
            assert abs(s0[K - 1] - s0[K]) < 1e-12 and abs(s0[K - 1] - s0[K - 2]) < 1e-12
        if kind == 2:
            assert mean[1 % E] == 0.0 and std[1 % E] == 0.0  # a zero-norm row scores 0 against everything


def test_cohort_stats_voxceleb_shape(gold):
    """E = 4 700, N = 400 000, K = 20 000 (19 row blocks, 3 125 x 2 score tiles each): 64 sampled rows against the restatement."""
    import torch

    from mindaudio_amd import ops

    E, N, K, D = 4700, 400000, 20000, 192
    rng = np.random.RandomState(77)
    centres = rng.randn(1200, D).astype(np.float32)
    q = centres[rng.randint(0, 1200, E)] + 1.5 * rng.standard_normal((E, D)).astype(np.float32)
    c = centres[rng.randint(0, 1200, N)] + 1.5 * rng.standard_normal((N, D)).astype(np.float32)
    mean, std = ops.cohort_stats(_dev(q), _dev(c), K)
    torch.cuda.synchronize()
    rows = np.unique(np.concatenate(([0, 255, 256, 4607, 4608, 4699], rng.randint(0, E, 58))))[:64]
    wm, wsd = _stats64(q[rows], c, K)
    tm, ts = _tols(gold, K)
    em = np.abs(mean.cpu().numpy()[rows] - wm).max()
    es = np.abs(std.cpu().numpy()[rows] - wsd).max()
    print("rows %d: mean %.3e (tol %.3e) std %.3e (tol %.3e)" % (len(rows), em, tm, es, ts))
    assert em <= tm and es <= ts
    assert np.isfinite(mean.cpu().numpy()).all() and (std.cpu().numpy() > 0).all()


def test_cohort_stats_is_deterministic():
    import torch

    from mindaudio_amd import ops

    q, c = GEN.make_stats_case(55, 300, 50000, 192, 2500, 1)
    qd, cd = _dev(q), _dev(c)
    m1, s1 = ops.cohort_stats(qd, cd, 2500)
    m2, s2 = ops.cohort_stats(qd, cd, 2500)
    m3, s3 = ops.cohort_stats(qd, cd, 2500, block_rows=37)  # another blocking of the rows: the same bits per row
    assert torch.equal(m1, m2) and torch.equal(s1, s2)
    assert torch.equal(m1, m3) and torch.equal(s1, s3)


def test_cohort_stats_rejects_bad_arguments():
    import torch

    from mindaudio_amd import ops

    q, c = torch.zeros(3, 192, device="cuda"), torch.zeros(10, 192, device="cuda")
    for k in (0, 11, -1):
        with pytest.raises(ValueError):
            ops.cohort_stats(q, c, k)
    with pytest.raises(ValueError):
        ops.cohort_stats(torch.zeros(3, 48, device="cuda"), torch.zeros(10, 48, device="cuda"), 2)
    with pytest.raises(ValueError):
        ops.cohort_stats(q, torch.zeros(10, 64, device="cuda"), 2)
    m, s = ops.cohort_stats(q, c)  # all-zero rows: every score is 0
    assert float(m.abs().max()) == 0.0 and float(s.abs().max()) == 0.0


# ---- running mean ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(GEN.EMB_MEAN_CASES)))
def test_running_mean_sub_matches_reference(gold, i):
    """Three chained calls over X1 and a fourth over X2 with the state carried (case 1: N = 1; every case starts at count 0)."""
    from mindaudio_amd import ops

    seed, N1, N2, D, rows = GEN.EMB_MEAN_CASES[i]
    x1, x2 = GEN.make_emb_mean_case(seed, N1, N2, D, rows)
    tol = float(gold["tol_emb_mean"])
    g, cnt = None, 0
    g64, cnt64 = np.zeros(D), 0
    for call, x in enumerate((x1, x1, x1, x2)):
        y, g, cnt = ops.running_mean_sub(_dev(x), g, cnt)
        sel = GEN.stored_rows(x.shape[0], rows)
        ey = np.abs(y.cpu().numpy()[sel] - gold["embmean%d_y%d_64" % (i, call)]).max()
        eg = np.abs(g.cpu().numpy() - gold["embmean%d_g%d_64" % (i, call)]).max()
        w, g64, cnt64 = _emb_mean64(g64, cnt64, x.astype(np.float64))
        er = np.abs(y.cpu().numpy() - w).max()
        print("case %d call %d: y %.3e g %.3e vs reference f64, y %.3e vs restatement (tol %.3e)" % (i, call, ey, eg, er, tol))
        assert ey <= tol and eg <= tol and er <= tol
        assert cnt == cnt64
    assert cnt == int(gold["embmean%d_count" % i])


def test_running_mean_ignores_mean_at_count_zero():
    import torch

    from mindaudio_amd import ops

    x = torch.randn(5, 64, device="cuda")
    y0, g0, c0 = ops.running_mean_sub(x)
    y1, g1, c1 = ops.running_mean_sub(x, torch.full((64,), 7.0, dtype=torch.float64, device="cuda"), 0)
    assert torch.equal(y0, y1) and torch.equal(g0, g1) and c0 == c1 == 5
    assert float(y0[0].abs().max()) == 0.0  # g = x[0] at count 0


def test_sentence_mean_norm():
    import torch

    from mindaudio_amd import ops

    x = torch.randn(3, 301, 80, device="cuda") * 20 - 40
    got = ops.sentence_mean_norm(x)
    want = x.double() - x.double().mean(1, keepdim=True)
    err = float((got.double() - want).abs().max())
    print("sentence mean norm: max err %.3e" % err)
    assert err <= 2.0 ** -23 * 128  # one float32 rounding of values below 128


# ---- trial scores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(GEN.TRIAL_CASES)))
def test_trial_scores_match_reference(gold, tmp_path, i):
    """All four modes against evaluate2's positive / negative lists (case 1: no cohort_size, the whole cohort); the same scores
    from cohort_stats + NumPy on the host; evaluate's equal error rate."""
    from mindaudio_amd import ops
    from mindaudio_amd.ecapa import speaker_verification_cosine as sv

    seed, E, N, D, K, n_trials = GEN.TRIAL_CASES[i]
    emb, cohort, labels, enrol, test = GEN.make_trial_case(seed, E, N, D, K, n_trials)
    trials = tmp_path / "trials.txt"
    trials.write_text("".join(GEN.trial_lines(labels, enrol, test)))
    table = sv.EmbeddingTable(["utt%05d" % k for k in range(E)], _dev(emb))
    cd = _dev(cohort)
    mean, std = ops.cohort_stats(table.emb, cd, K or None)
    raw = ops.trial_scores(table.emb, enrol, test).cpu().numpy()
    m, s = mean.cpu().numpy(), std.cpu().numpy()
    for mode in GEN.TRIAL_MODES:
        params = {} if mode == "none" else {"score_norm": mode}
        if K:
            params["cohort_size"] = K
        pos, neg = sv.evaluate2(table, table, cd, params, str(trials), log=lambda *a: None)
        tol = float(gold["tol_score_raw" if mode == "none" else "tol_score_norm"])
        ep = np.abs(pos - gold["trial%d_%s_pos64" % (i, mode)]).max()
        en = np.abs(neg - gold["trial%d_%s_neg64" % (i, mode)]).max()
        host = _norm64(raw, m[enrol], s[enrol], m[test], s[test], mode)
        got = ops.trial_scores(table.emb, enrol, test, mean, std, None if mode == "none" else mode).cpu().numpy()
        eh = np.abs(got - host).max() / max(1.0, np.abs(host).max())
        print("case %d %s: pos %.3e neg %.3e (tol %.3e); vs cohort_stats + NumPy %.3e" % (i, mode, ep, en, tol, eh))
        assert pos.shape == gold["trial%d_%s_pos64" % (i, mode)].shape and ep <= tol and en <= tol
        assert eh <= 1e-14
        assert np.array_equal(got[labels == 1], pos) and np.array_equal(got[labels == 0], neg)
    eer = sv.evaluate(table, table, str(trials))
    print("evaluate eer", eer, float(gold["trial%d_evaluate_eer" % i]))
    assert abs(eer - float(gold["trial%d_evaluate_eer" % i])) <= 1e-9


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _make_corpus(root, tag, speakers, per_speaker, rng):
    """Tone mixtures keyed by speaker, three different lengths; returns the csv path and [(ID, speaker)]."""
    os.makedirs(root / tag, exist_ok=True)
    rows, ids = [], []
    lengths = (16000, 20800, 27200)
    for spk in speakers:
        f0 = 90.0 + 37.0 * spk
        for u in range(per_speaker):
            n = lengths[(spk + u) % 3]
            t = np.arange(n + 800) / 16000.0
            x = sum(a * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28)) for h, a in ((1, 0.3), (2, 0.2), (3 + spk % 3, 0.15)))
            x = x + 0.02 * rng.randn(t.size)
            uid = "id%03d/%s/%05d" % (spk, tag, u)
            path = root / tag / ("%03d_%05d.wav" % (spk, u))
            _write_wav(path, x)
            rows.append("%s, %s, %d, %d\n" % (uid, path, 400, 400 + n))  # a segment of the file, as the example's csv rows
            ids.append((uid, spk))
    csv_path = root / (tag + ".csv")
    csv_path.write_text("ID, wav, start, stop\n" + "".join(rows))
    return str(csv_path), ids


@pytest.fixture(scope="module")
def recipe(tmp_path_factory):
    import torch

    from mindaudio_amd.ecapa import speaker_verification_cosine as sv
    from mindaudio_amd.models import EcapaTDNN

    root = tmp_path_factory.mktemp("sv")
    rng = np.random.RandomState(9)
    enrol_csv, enrol_ids = _make_corpus(root, "enrol", range(6), 4, rng)
    train_csv, _ = _make_corpus(root, "train", range(6, 18), 4, rng)
    sv.compute_feat_loop(enrol_csv, str(root / "feat_eval"), log=lambda *a: None)
    sv.compute_feat_loop(train_csv, str(root / "feat_norm"), log=lambda *a: None)
    lines = []
    for a in range(len(enrol_ids)):
        for b in rng.choice(len(enrol_ids), 5, replace=False):
            if a != b:
                lines.append("%d %s.wav %s.wav\n" % (int(enrol_ids[a][1] == enrol_ids[b][1]), enrol_ids[a][0], enrol_ids[b][0]))
    veri = root / "veri.txt"
    veri.write_text("".join(lines))
    torch.manual_seed(4)
    model = EcapaTDNN(80, channels=(512, 512, 512, 512, 1536), lin_neurons=192)
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    model = model.cuda().eval()
    cfg = dict(in_channels=80, channels=512, emb_size=192, eval_data_path=str(root / "feat_eval"),
               train_norm_path=str(root / "feat_norm"), veri_file_path=str(veri), score_norm="s-norm", cohort_size=20,
               cut_wav=False, n_train_snts=400000, npy_file_path=str(root / "npys"), embed_batch_size=1)
    return dict(root=root, cfg=cfg, model=model, veri=str(veri), sv=sv)


def test_feature_folder(recipe):
    """compute_feat_loop: the reference's folder layout, (1, frames, 80) float32 with a zero mean over time, three lengths."""
    sv = recipe["sv"]
    ds = sv.DatasetGenerator(recipe["cfg"]["eval_data_path"], False)
    assert len(ds) == 24 and len(sv.DatasetGenerator(recipe["cfg"]["eval_data_path"])) == 23
    frames = set()
    for i in range(len(ds)):
        data, label = ds[i]
        assert data.dtype == np.float32 and data.shape[0] == 1 and data.shape[2] == 80 and label.startswith("id")
        assert np.abs(data.astype(np.float64).mean(1)).max() < 1e-4
        frames.add(data.shape[1])
    assert frames == {101, 131, 171}


def test_recipe_end_to_end(recipe, gold):
    import torch

    from mindaudio_amd.metric import EER, get_eer_from_scores
    from mindaudio_amd.utils import ckpt

    sv, cfg, model = recipe["sv"], recipe["cfg"], recipe["model"]
    logs, details = [], {}
    eers = sv.eval_impl(cfg, log=logs.append, model=model, details=details)
    text = "\n".join(str(x) for x in logs)
    print(text)
    for words in ("size of enroll, test: 24", "eer baseline: ", "Sub mean...", "eer with sub mean: ", "steps_per_epoch_train: 48",
                  "norm data len: 48", "train_cohort shape: (48, 192)", "EER with norm: "):
        assert words in text, words

    # float64 host recomputation from the model's own B = 1 embeddings
    def embed(path):
        ds = sv.DatasetGenerator(path, False)
        names, out = [], []
        for i in range(len(ds)):
            data, label = ds[i]
            names.append(label)
            out.append(model(torch.from_numpy(data).cuda()).reshape(-1).cpu().numpy())
        return names, np.stack(out).astype(np.float64)

    names, e64 = embed(cfg["eval_data_path"])
    _, t64 = embed(cfg["train_norm_path"])
    assert names == details["enroll"].names
    assert np.array_equal(details["enroll"].emb.cpu().numpy(), e64.astype(np.float32))  # embed_batch_size 1: the same forward
    index = {n: i for i, n in enumerate(names)}
    labels, enrol, test = sv.parse_trials(cfg["veri_file_path"], index, index)
    g, cnt = np.zeros(192), 0
    for _ in range(3):
        em, g, cnt = _emb_mean64(g, cnt, e64)
    tm, g, cnt = _emb_mean64(g, cnt, t64)
    raw = (_unit(em)[enrol] * _unit(em)[test]).sum(1)
    m, s = _stats64(em, tm, cfg["cohort_size"])
    want = _norm64(raw, m[enrol], s[enrol], m[test], s[test], "s-norm")
    tol = float(gold["tol_score_norm"])
    ep = np.abs(details["pos"] - want[labels == 1]).max()
    en = np.abs(details["neg"] - want[labels == 0]).max()
    print("s-norm scores vs float64 host recomputation: pos %.3e neg %.3e (tol %.3e), scores in [%.2f, %.2f]"
          % (ep, en, tol, want.min(), want.max()))
    assert ep <= tol and en <= tol
    assert want.max() - want.min() > 0.5  # the synthetic speakers spread the scores

    # the three equal error rates are the host metrics of the device's own scores
    base = sv._trial_scores(details["enroll"], details["enroll"], cfg["veri_file_path"])[0]
    sub = sv._trial_scores(details["enroll_mean"], details["enroll_mean"], cfg["veri_file_path"])[0]
    assert np.abs(base - (_unit(e64)[enrol] * _unit(e64)[test]).sum(1)).max() <= float(gold["tol_score_raw"])
    assert np.abs(sub - raw).max() <= float(gold["tol_score_raw"])
    assert eers[0] == get_eer_from_scores(base, labels)[0]
    assert eers[1] == get_eer_from_scores(sub, labels)[0]
    assert eers[2] == EER(details["pos"], details["neg"])
    assert all(0.0 <= v <= 1.0 for v in eers)

    # the checkpoint-file path gives what the in-memory model gives (second run: the cohort embeddings come from the cache)
    path = str(recipe["root"] / "ecapa.ckpt")
    ckpt.write_mindspore_ckpt(path, ckpt.ecapa_to_reference_names(model.state_dict()))
    logs2, details2 = [], {}
    eers2 = sv.eval_impl(dict(cfg, model_path=path), log=logs2.append, details=details2)
    assert eers2 == eers
    assert np.array_equal(details2["pos"], details["pos"]) and np.array_equal(details2["neg"], details["neg"])
    assert any("find cache file" in str(x) for x in logs2) and path in "\n".join(str(x) for x in logs2)


def test_same_length_batching_matches_one_at_a_time(recipe):
    """Utterances of one frame count embedded as a batch: the embeddings of the one-at-a-time forward within 1e-4 relative (the
    project's allowance for GEMMs over 1 or n utterances), in the same order, nothing padded."""
    sv, cfg, model = recipe["sv"], recipe["cfg"], recipe["model"]
    ds = sv.DatasetGenerator(cfg["eval_data_path"], False)
    one = sv.compute_embeddings(model, ds, dur=len(ds), batch_size=1, log=lambda *a: None)
    many = sv.compute_embeddings(model, ds, dur=len(ds), batch_size=16, log=lambda *a: None)
    skip = sv.compute_embeddings(model, ds, dur=len(ds), exc_set={1, 5}, cut_wav=True, batch_size=16, log=lambda *a: None)
    assert one.names == many.names and len(skip) == len(one) - 2 and ds[1][1] not in skip.index
    a, b = one.emb.cpu().numpy().astype(np.float64), many.emb.cpu().numpy().astype(np.float64)
    rel = np.abs(a - b).max() / np.abs(a).max()
    print("batched vs one at a time: max |d| / max |x| = %.3e" % rel)
    assert rel <= 1e-4
    assert not np.array_equal(a[0], a[1])


def test_unknown_score_norm_and_oversized_cohort(recipe):
    sv, cfg, model = recipe["sv"], recipe["cfg"], recipe["model"]
    with pytest.raises(ValueError):
        sv.eval_impl(dict(cfg, score_norm="q-norm"), log=lambda *a: None, model=model)
    with pytest.raises(ValueError):
        sv.eval_impl(dict(cfg, cohort_size=49), log=lambda *a: None, model=model)
