#!/usr/bin/env python3
"""bench.py — headline benchmark of the mindaudio hot path on MI355X.

Metric (BASELINE.json): utterances/s (16 kHz x 10 s), fbanks + Conformer forward.

One "step" = one pass of the hot path over one synthetic batch resident in HBM:
  waves (64, 160000) f32 --features.fbank(n_fft=512, hop=160, n_mels=80)--> (64, 80, 1001) dB
  --> (64, 1000, 80) --> Conformer-small encoder forward (12 blocks, d=256, 4 heads, ff=2048, k=15; eval mode,
  bf16 MFMA matmuls with float32 accumulation) --> (64, 249, 256).
N GPUs = N independent shards of 64 utterances (weak scaling; inference forward has no data-path collective and
the reference's batch-global top_db floor is per call, i.e. per rank — SURVEY §8e).

  python bench.py [--gpus N --steps K --warmup W]      N > 1 without WORLD_SIZE in the environment: this process starts
                                                        `python -m torch.distributed.run --nproc-per-node N bench.py ...`
                                                        as a child BEFORE anything touches the GPU and relays its output
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (how the driver launches N > 1)

A plain run sets up, warms up, times the K steps and prints the headline (`--train` makes the cfg-4 data-parallel CTC
training step of Conformer-small the headline instead).  `--full` adds everything else: `sustained` (the same step timed
over >= 2 s, after the burst figure), the two rooflines and their probes, cfg 3 and cfg 5, `train_dp` (the training step
with the bucketed RCCL gradient all-reduce, its bus bandwidth and the exposed communication time), the hybrid and
bucket-cycling training legs, and at N = 1 the CPU baselines.  `--dump-outputs DIR` writes what the timed path returned in
its last step as DIR/<name>.npy (float32; the inputs and weights are seeded, so two builds can be compared output for
output).  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BATCH, SAMPLES, N_FFT, HOP, N_MELS, SR = 64, 160000, 512, 160, 80, 16000
FRAMES = 1000
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_BF16_PEAK_TF = 2500.0  # MI355X_MICROARCH.md: ~2.5 PFLOP/s dense bf16
XGMI_LINK_GBS = 153.0       # per xGMI link, 7 links per GPU
FBANK_KW = dict(n_mels=N_MELS, n_fft=N_FFT, hop_length=HOP)
TRAIN_BATCH, TRAIN_FRAMES, TRAIN_VOCAB = 40, 1024, 4233  # conformer.yaml bucket 1024 -> 40 utterances per rank, AISHELL vocabulary


def synth_batch(seed, n=BATCH):
    return (0.1 * np.random.RandomState(seed).randn(n, SAMPLES)).astype(np.float32)


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(out_dir, **arrays):
    """--dump-outputs: each array (a tensor on any device) as out_dir/<name>.npy in float32."""
    import torch

    arrays = {k: v.detach().to(torch.float32).cpu().numpy() for k, v in arrays.items()}
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_BYTES_MAX
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ======================================================================================================================
# CPU baselines (oracle = CPU restatement of the reference; baseline only, never the product path)
# ======================================================================================================================
def _cpu_fbank_r(x):
    from oracle import speech_features as O

    return O.fbank_ref_cost(x[None], n_mels=N_MELS, n_fft=N_FFT, sample_rate=SR, hop_length=HOP).shape


def _cpu_fbank_v(x):
    from oracle import speech_features as O

    return O.fbank(x[None], **FBANK_KW).shape


def cpu_baseline():
    """fbank in two flavours — (R) the reference's own cost structure (float64 framing loop + per-column
    rFFT + mel matmul + amplitude_to_dB) and (V) vectorised NumPy — each as one process and as Pool(min(8, nproc)) over
    utterances (the reference's own parallelism, examples/conformer/dataset.py:449,479); Conformer-small forward =
    PyTorch-CPU float32 eager oracle at batch 64 on all host threads.  `value` = fastest (R) fbank followed by that
    encoder, end to end."""
    import multiprocessing as mp

    import torch

    from oracle import conformer_oracle as C

    nproc = os.cpu_count() or 1
    n_fb = 16
    rows = list(synth_batch(1234, n_fb))
    fb = {}
    pool_n = min(8, nproc)
    ctx = mp.get_context("spawn")  # never fork a process that holds a HIP context
    with ctx.Pool(pool_n) as pool:
        for name, fn in (("R", _cpu_fbank_r), ("V", _cpu_fbank_v)):
            fn(rows[0])
            t0 = time.perf_counter()
            for r in rows:
                fn(r)
            fb[name + "_1proc"] = n_fb / (time.perf_counter() - t0)
            pool.map(fn, rows[:pool_n])
            t0 = time.perf_counter()
            pool.map(fn, rows)
            fb[name + "_pool%d" % pool_n] = n_fb / (time.perf_counter() - t0)
    torch.manual_seed(0)
    enc = C.ConformerEncoder(80, 256, 4, 2048, 12).eval()
    xs = torch.randn(BATCH, FRAMES, 80)
    mask = C.subsample_mask(torch.ones(BATCH, 1, FRAMES))
    with torch.no_grad():
        enc(xs[:4], mask[:4])
        t0 = time.perf_counter()
        enc(xs, mask)
        enc_rate = BATCH / (time.perf_counter() - t0)
    best_r = max(v for k, v in fb.items() if k.startswith("R"))
    e2e = 1.0 / (1.0 / best_r + 1.0 / enc_rate)
    return {"value": round(e2e, 3), "unit": "utterances/s", "cores": nproc, "kind": "port",
            "fbank_utt_per_s": {k: round(v, 2) for k, v in fb.items()},
            "encoder_utt_per_s": round(enc_rate, 3), "encoder_threads": torch.get_num_threads(),
            "sample": "fbank: %d utterances (10 s @16 kHz) per flavour — R = oracle.fbank_ref_cost (reference cost structure, "
                      "NumPy float64), V = oracle.fbank (vectorised NumPy); 1 process and Pool(%d) each.  Encoder: one batch "
                      "of %d x %d x 80 through the oracle Conformer-small (PyTorch-CPU float32 eager, %d threads).  value = "
                      "fastest R fbank + encoder, end to end" % (n_fb, pool_n, BATCH, FRAMES, torch.get_num_threads())}


# ======================================================================================================================
# launcher: N > 1 ranks as fresh children (decided before any HIP call in this process)
# ======================================================================================================================
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n):
    """Start `torch.distributed.run` with n ranks of this script as a CHILD process (this process has not initialised
    the GPU and never does), pass its output through and return its exit code."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


# ======================================================================================================================
# cfg 4: data-parallel CTC training step
# ======================================================================================================================
def synth_train_batch(rank, dev, b=TRAIN_BATCH, t=TRAIN_FRAMES, vocab=TRAIN_VOCAB):
    """AISHELL-shaped synthetic bucket-1024 batch for one rank: the 11 columns of examples/conformer/train.py:38-50."""
    import torch

    rng = np.random.RandomState(1234 + rank)
    xs = torch.from_numpy(rng.randn(b, t, 80).astype(np.float32)).to(dev)
    lens = rng.randint(int(0.7 * t), t + 1, b)
    lens[0] = t
    t2 = ((t - 3) // 2 + 1 - 3) // 2 + 1
    masks = torch.zeros(b, 1, t2)
    for i, n in enumerate(lens):
        masks[i, 0, :(n - 1) // 4] = 1  # frames 4j < n (dataset.py:625)
        xs[i, n:] = 0
    ylens = rng.randint(5, 31, b).astype(np.int32)
    ys = np.full((b, 30), -1, np.int32)
    for i, n in enumerate(ylens):
        ys[i, :n] = rng.randint(1, vocab - 1, n)
    sos = eos = vocab - 1
    ys_in = np.full((b, 31), eos, np.int32)
    ys_out = np.full((b, 31), -1, np.int32)
    ys_m = np.zeros((b, 1, 31), np.float32)
    for i, n in enumerate(ylens):
        ys_in[i, 0] = sos
        ys_in[i, 1:n + 1] = ys[i, :n]
        ys_out[i, :n] = ys[i, :n]
        ys_out[i, n] = eos
        ys_m[i, 0, :n + 1] = 1
    ys_sub = (ys_m.astype(bool) & np.tril(np.ones((31, 31), bool))[None]).astype(np.float32)
    d = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return (xs, d(ys), d(ys_in), d(ys_out), None, None, masks.to(dev), d(ys_sub), d(ys_m), d(ylens), None)


def train_step_flops(b, t, vocab, d=256, hidden=2048, blocks=12, heads=4, ks=15, dec_blocks=0):
    """Algorithmic FLOPs of one cfg-4 optimizer step (2 x multiply-adds of every contraction; backward = 2 x forward: one product
    for the input gradient, one for the weight gradient), per rank.  Forward per utterance at t = 1024: 23.86 GFLOP."""
    t1, f1 = (t - 3) // 2 + 1, (80 - 3) // 2 + 1
    t2, f2 = (t1 - 3) // 2 + 1, (f1 - 3) // 2 + 1
    dk = d // heads
    front = 2 * 9 * d * t1 * f1 + 2 * 9 * d * d * t2 * f2 + 2 * f2 * d * d * t2
    layer = 2 * (2 * t2 * d * hidden * 2) + 2 * t2 * d * 3 * d + heads * (2 * t2 * t2 * 2 * dk + 2 * t2 * t2 * dk) + 2 * t2 * d * d \
        + 2 * t2 * d * 2 * d + 2 * t2 * d * ks + 2 * t2 * d * d
    fwd = front + blocks * layer + 2 * t2 * d * vocab
    if dec_blocks:  # TransformerDecoder on 31 tokens per utterance: self-attn (qkv, o), source attention (q, kv over T', o), FFN, output layer
        lt = 31
        dec_layer = 2 * lt * (4 * d * d + 2 * d * d + 2 * d * hidden) + 2 * t2 * 2 * d * d + heads * (4 * lt * lt * dk + 4 * lt * t2 * dk)
        fwd += dec_blocks * dec_layer + 2 * lt * d * vocab
    return 3.0 * b * fwd


def comm_metrics(res, eng, world, force_collective, steps, timed, barrier):
    """The N > 1 part of the train_dp object (also exercised on CPU / gloo by tests/test_bench_launcher_cpu.py through MA_BENCH_DRY):
    ms_per_step_no_allreduce, exposed_comm_ms, allreduce{ms, bytes, buckets, bus_GBps, ...}."""
    import torch.distributed as tdist

    # (i) the step without its collective: exposed communication = ms_per_step - ms_per_step_no_comm
    eng.reducer.world, eng.reducer.force = 1, False
    dt0, _ = timed(max(3, steps // 2))
    eng.reducer.world, eng.reducer.force = world, force_collective
    res["ms_per_step_no_allreduce"] = round(dt0 / max(3, steps // 2) * 1e3, 3)
    res["exposed_comm_ms"] = round(res["ms_per_step"] - res["ms_per_step_no_allreduce"], 3)
    # (ii) the all-reduce alone, same buckets: bus bandwidth = 2 (N-1)/N x bytes / t  (ring-equivalent)
    from mindaudio_amd.train.engine import bucket_spans

    spans = bucket_spans(eng.fp, eng.L)
    reps = 5
    barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        works = [tdist.all_reduce(eng.fp.grad[lo:hi], async_op=True) for lo, hi in spans]
        for w in works:
            w.wait()
    barrier()
    ar = (time.perf_counter() - t0) / reps
    nbytes = sum(hi - lo for lo, hi in spans) * 4
    bus = 2.0 * (world - 1) / max(world, 1) * nbytes / ar / 1e9
    res["allreduce"] = {"ms": round(ar * 1e3, 3), "bytes": nbytes, "buckets": len(spans),
                        "bus_GBps": round(bus, 1), "xgmi_link_GBps": XGMI_LINK_GBS,
                        "frac_of_one_link": round(bus / XGMI_LINK_GBS, 3)}


def train_leg(rank, world, dev, dist, steps, warmup, barrier, force_collective=False, digest=False, ctc_weight=1.0,
              default_stream=False, full=True, dump_dir=None):
    """cfg 4: `steps` optimizer steps of ConformerCTCTrainStep on a (40, 1024, 80) batch per rank, gradients
    all-reduced over RCCL in per-block buckets overlapped with the backward pass.  With `full`, also times the host side of
    one step, the same all-reduce alone (bus bandwidth) and the step with communication disabled (exposed communication).
    `dump_dir`: write the last timed step's loss and a fixed sample of the trained float32 masters there."""
    import torch

    from mindaudio_amd.conformer.asr_model import create_asr_model
    from mindaudio_amd.train.engine import ConformerCTCTrainStep

    torch.manual_seed(777)  # same initial weights on every rank (examples/conformer/train.py:56)
    hybrid = ctc_weight != 1.0  # the shipped conformer.yaml: ctc_weight 0.3, 6-block TransformerDecoder, label smoothing 0.1

    def make_model():
        torch.manual_seed(777)
        return create_asr_model(80, TRAIN_VOCAB, dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12),
                                ctc_weight=ctc_weight,
                                decoder_conf=dict(attention_heads=4, linear_units=2048, num_blocks=6, dropout_rate=0.1,
                                                  positional_dropout_rate=0.1) if hybrid else None,
                                lsm_weight=0.1 if hybrid else 0.0).to(dev)

    model = make_model()
    # (own_stream: with RCCL in play the engine runs the step on a stream of its own - RCCL's stream was seen sharing the hardware
    # queue of torch's default stream; --train-default-stream is the A/B switch)
    eng = ConformerCTCTrainStep(model, dropout_rate=0.1, positional_dropout_rate=0.1, world_size=world, rank=rank,
                                force_collective=force_collective, own_stream=False if default_stream else "auto")
    cols = synth_train_batch(rank, dev)

    def timed(n):
        barrier()
        t0 = time.perf_counter()
        for _ in range(n):
            out = eng.step(*cols)
        barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt, out

    first = [float(eng.step(*cols)[0]) for _ in range(max(warmup, 1))]
    dt, out = timed(steps)
    if dump_dir is not None:  # (all masters are 138 MB: a seeded sample of 4 Mi of them)
        idx = torch.from_numpy(np.random.RandomState(0).randint(0, eng.fp.size, 1 << 22)).to(dev)
        dump_outputs(dump_dir, loss=out[0].reshape(1), masters_sample=eng.fp.master[idx])
    res = {"utterances_per_s": round(world * TRAIN_BATCH * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
           "steps": steps, "global_batch": TRAIN_BATCH * world, "frames": TRAIN_FRAMES, "vocab": TRAIN_VOCAB,
           "workload": "Conformer-small (12 blocks) %s training step: forward + backward + bucketed gradient "
                       "all-reduce + Adam/ASRWarmupLR/dynamic loss scale, dropout 0.1, bf16 matmuls, float32 masters" %
                       ("hybrid (0.3 CTC + 0.7 attention, 6-block TransformerDecoder, label smoothing 0.1: the shipped conformer.yaml)"
                        if hybrid else "pure-CTC"),
           "first_loss": round(first[0], 3), "last_loss": round(float(out[0]), 3), "loss_scale": out[2],
           "overflow_last_step": bool(out[3]), "grad_bytes": eng.fp.size * 4}
    flops = train_step_flops(TRAIN_BATCH, TRAIN_FRAMES, TRAIN_VOCAB, dec_blocks=6 if hybrid else 0)
    tf = world * flops / (dt / steps) / 1e12
    res["roofline"] = {"bound": "mfma", "algorithmic_flops_per_step": int(world * flops), "achieved": round(tf, 1),
                       "peak": MFMA_BF16_PEAK_TF * world, "unit": "TFLOP/s", "frac": round(tf / (MFMA_BF16_PEAK_TF * world), 4)}
    if full:
        # host side of one step: the time to ENQUEUE it (Python + ctypes + launches) with the GPU kept busy, so that no call waits for
        # the device; the step is GPU-bound while this stays below ms_per_step (8 ranks share one host)
        enq = []
        for _ in range(3):  # (median of three: the CPU baseline's child process may be busy on the same cores)
            torch.cuda.synchronize()
            torch.cuda._sleep(int(1e8))  # ~50 ms of GPU time in front of the step
            t0 = time.perf_counter()
            pending = eng.enqueue_step(*cols)
            enq.append((time.perf_counter() - t0) * 1e3)
            eng.finish_step(*pending)
        res["host_enqueue_ms"] = round(sorted(enq)[1], 3)
    if force_collective:
        res["force_collective"] = True
    if digest:  # bit pattern of the trained masters (tests/test_rccl_world1_gpu.py compares runs with and without the collective)
        import hashlib

        res["masters_sha16"] = hashlib.sha256(eng.fp.master.cpu().numpy().tobytes()).hexdigest()[:16]
    if full and (world > 1 or force_collective):
        comm_metrics(res, eng, world, force_collective, steps, timed, barrier)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: sustained figure, rooflines and probes, cfg3 / cfg5, training legs, CPU baselines "
                         "(the --no-* switches below thin this out)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed path returned in its last step as DIR/<name>.npy (float32, seeded inputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-only", action="store_true", help="(internal) print the cpu_baseline object and exit")
    ap.add_argument("--train", action="store_true", help="headline = the cfg-4 data-parallel training step")
    ap.add_argument("--no-train-leg", action="store_true", help="skip the train_dp object")
    ap.add_argument("--no-sustained", action="store_true")
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--force-collective", action="store_true",
                    help="issue the gradient all-reduces through RCCL even at world size 1 (stream-ordering check on one GPU)")
    ap.add_argument("--train-digest", action="store_true", help="add a hash of the trained masters to train_dp")
    ap.add_argument("--no-cfg3", action="store_true", help="skip the cfg-3 (32 x 1000 x 80 encoder forward) object")
    ap.add_argument("--no-cfg5", action="store_true", help="skip the cfg-5 (ECAPA-TDNN forward, 256 x 300 x 80) object")
    ap.add_argument("--no-hybrid-leg", action="store_true", help="skip the train_dp_hybrid object (ctc_weight 0.3 training step)")
    ap.add_argument("--no-bucket-leg", action="store_true", help="skip the train_bucket_cycle object (the hybrid step over the yaml's "
                    "16 buckets, a different bucket every step)")
    ap.add_argument("--step-only", action="store_true",
                    help="(profiling) the plain run even with --full: only the warm-up + timed steps of the headline, so that the "
                         "kernel stats of this run are the step's launches and nothing else")
    ap.add_argument("--train-default-stream", action="store_true",
                    help="run the data-parallel training leg on torch's default stream instead of a stream of its own (A/B of the "
                         "hardware-queue sharing with RCCL's stream)")
    args = ap.parse_args()
    if args.step_only:
        args.full = False

    # ---- N > 1: one process per GPU.  Either we already are a rank (WORLD_SIZE set by torch.distributed.run) or this
    #      process becomes the launcher — decided here, before torch.cuda / any HIP call. ------------------------------
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1 and not args.cpu_baseline_only:
            sys.exit(launch_ranks(args.gpus))
        world = 1
    else:
        world = int(os.environ["WORLD_SIZE"])
        if world != args.gpus:
            sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d; launch with --nproc-per-node %d (or drop WORLD_SIZE and let "
                     "bench.py start the ranks itself)" % (args.gpus, world, args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dry = os.environ.get("MA_BENCH_DRY") == "1"  # launcher check on a box without GPUs: gloo ranks, no kernels

    # The CPU baselines run in a CHILD process, before this one touches the GPU: they use a process pool and every host thread
    # (the PyTorch-CPU oracle's OpenMP team), and a team left behind in this process slowed the launch-bound training leg by 20 %.
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline()))
        return
    cpu = None
    if world == 1 and args.full and not args.no_cpu_baseline and not dry:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only"], stdout=subprocess.PIPE, check=True)
        cpu = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])

    import torch

    dist = None
    if world > 1 or (args.force_collective and not dry):
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        if dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
            t = torch.tensor([float(rank + 1)])
            dist.all_reduce(t)
            # the N > 1 fields of train_dp, computed by the same function as on the GPU over a stand-in engine (flat gradient of the
            # real model's layout is not needed for the plumbing: 14 spans of a small flat buffer)
            from types import SimpleNamespace

            from mindaudio_amd.train import engine as _eng

            fake_fp = SimpleNamespace(grad=torch.ones(14 * 1000), spans14=[(i * 1000, (i + 1) * 1000) for i in range(14)])
            real_spans = _eng.bucket_spans
            _eng.bucket_spans = lambda fp, L: fp.spans14
            try:
                fake = SimpleNamespace(fp=fake_fp, L=12, reducer=SimpleNamespace(world=world, force=False))
                tdp = {"ms_per_step": 1.0}
                comm_metrics(tdp, fake, world, False, 2, lambda n: (1e-3 * n, None), lambda: dist.barrier())
            finally:
                _eng.bucket_spans = real_spans
            if rank == 0:
                print(json.dumps({"dry": True, "n_gpus": world, "ranks_sum": float(t.item()), "train_dp_multi": tdp,
                                  "grad_sum": float(fake_fp.grad.sum().item())}))
            dist.destroy_process_group()
            return
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    elif dry:
        print(json.dumps({"dry": True, "n_gpus": 1}))
        return
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)

    import mindaudio_amd as ma
    from mindaudio_amd import _host, _lib, ops
    from mindaudio_amd.models import ConformerEncoder

    lib = _lib.load()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(dt):
        if dist is not None:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt

    t2 = ((FRAMES - 3) // 2 + 1 - 3) // 2 + 1
    train = None
    if not args.train:
        torch.manual_seed(777)  # examples/conformer/train.py:56
        enc = ConformerEncoder(80, 256, 4, 2048, 12).eval().to(dev).prepare()
        x = torch.from_numpy(synth_batch(1234 + rank)).to(dev)
        masks = torch.ones(BATCH, 1, t2, device=dev)

        def step():
            feats = ma.fbank(x, **FBANK_KW)                             # (64, 80, 1001) dB
            xs = feats.transpose(1, 2)[:, :FRAMES]                      # (64, 1000, 80) VIEW of the (64, 80, 1001) fbank output
            return enc(xs, masks)[0]

        for _ in range(args.warmup):
            out = step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        barrier()
        dt = max_over_ranks(time.perf_counter() - t0)
        assert tuple(out.shape) == (BATCH, t2, 256)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, encoder_out=out)  # (64, 249, 256): 16 MB

        sustained = None
        if args.full and not args.no_sustained:
            # the same step over >= 2 s: the chip reaches its power limit within ~1 s (DVFS), the K-step figure above is a burst
            n_sus = max(args.steps, int(2.2 / (dt / args.steps)) + 1)
            barrier()
            t0 = time.perf_counter()
            for _ in range(n_sus):
                out = step()
            barrier()
            ds = max_over_ranks(time.perf_counter() - t0)
            sustained = {"value": round(world * BATCH * n_sus / ds, 1), "unit": "utterances/s", "steps": n_sus,
                         "seconds": round(ds, 3), "ms_per_step": round(ds / n_sus * 1e3, 4)}
    else:
        train = train_leg(rank, world, dev, dist if world > 1 else None, args.steps, args.warmup, barrier, args.force_collective,
                          args.train_digest, default_stream=args.train_default_stream, full=args.full,
                          dump_dir=args.dump_outputs if rank == 0 else None)

    def headline():
        if args.train:
            return {
                "metric": "utterances/s, Conformer-small CTC training step (fwd + bwd + RCCL all-reduce + Adam), 1/2/4/8 MI355X",
                "value": train["utterances_per_s"], "unit": "utterances/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": train["ms_per_step"], "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {"workload": train["workload"], "global_batch": TRAIN_BATCH * world, "frames": TRAIN_FRAMES,
                           "sharding": "data parallel by utterance, bucketed all-reduce (SUM) of the flat float32 gradient"},
                "train_dp": {k: v for k, v in train.items() if k not in ("utterances_per_s", "ms_per_step", "workload")},
            }
        return {
            "metric": "utterances/s (16 kHz×10 s) fbanks+Conformer fwd, 1/2/4/8 MI355X",
            "value": round(world * BATCH * args.steps / dt, 1),
            "unit": "utterances/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {"workload": "features.fbank (n_fft=512 hop=160 n_mels=80, batch-global top_db) on 64 x (10 s "
                                   "@16 kHz) synthetic waves per GPU -> Conformer-small encoder forward (12 blocks, "
                                   "d=256, 4 heads, ff=2048, conv k=15, eval mode) on the (64, 1000, 80) features; "
                                   "random-init weights",
                       "global_batch": BATCH * world, "frames": FRAMES,
                       "sharding": "independent utterance shards per rank, no collective",
                       "encoder_tflops": round(world * BATCH * args.steps * 23.12e9 / dt / 1e12, 1)},
        }

    if not args.full:
        if rank == 0:
            print(json.dumps(headline()))
        if dist is not None:
            dist.destroy_process_group()
        return

    def event_time(fn, reps):
        for _ in range(5):
            fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(reps):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / reps * 1e-3  # seconds per launch

    # ---- roofline of the dominant kernel: ffn_packed_kernel (MFMA bound; ~45 % of the step), timed in the form the encoder
    #      launches it 11 times per forward: the last FFN of a block + the macaron FFN of the next + the three LayerNorms
    #      around them + linear_q/k/v of the next attention, one launch (the other 2 launches per forward are single FFNs).
    #      Algorithmic FLOPs per launch = 2 FFNs x 2 M (256*2048 + 2048*256) + 2 M 256*768, M = 64*249 rows. ---------------
    m, hid, nqkv = BATCH * t2, 2048, 768
    gen = torch.Generator(device=dev).manual_seed(99)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)  # noqa: E731
    wa1, wb1 = (rnd(hid, 256) / 16).bfloat16(), (rnd(hid, 256) / 16).bfloat16()
    wa2, wb2 = (rnd(256, hid) / 45).bfloat16(), (rnd(256, hid) / 45).bfloat16()
    wq, bq = (rnd(nqkv, 256) / 16).bfloat16(), rnd(nqkv)
    b1, b2 = rnd(hid), rnd(256)
    xres = rnd(m, 256)
    pa, pb, pq = ops.ffn_pack_weights(wa1, wa2), ops.ffn_pack_weights(wb1, wb2), ops.ffn_qkv_pack(wq)
    ln = (torch.ones(256, device=dev), torch.zeros(256, device=dev))
    gemm_s = event_time(lambda: ops.ffn_packed_pair(pa, b1, b2, pb, b1, b2, xres, ln, ln, ln, ln, alpha=0.5, qkv=(pq, bq)),
                        max(args.steps, 50))
    ffn_flops = 2 * (2.0 * m * 256 * hid * 2) + 2.0 * m * 256 * nqkv
    gemm_tf = ffn_flops / gemm_s / 1e12
    # The same launch timed IN the step (an event pair around each of the encoder's 11 pair + qkv launches over a few steps, outside
    # the timed region above): there its activations come from the convolution module's launch and its weights were last read a block
    # ago - the back-to-back figure above is the kernel's own rate, this one is what the headline step pays for it.
    in_step = None
    if not args.train:
        enc._pair_events = []
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) * 1e-3 for a, b in enc._pair_events)
        del enc._pair_events
        # what an event pair costs with NOTHING between its two records, behind a busy stream: subtracted, so that in_step is comparable
        # with rocprofv3's kernel-trace duration of the launch (profiles/r0N_bench_kernel_stats.csv)
        empty = []
        for _ in range(60):
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.ffn_packed_pair(pa, b1, b2, pb, b1, b2, xres, ln, ln, ln, ln, alpha=0.5, qkv=(pq, bq))  # a busy stream in front
            a_.record()
            b_.record()
            empty.append((a_, b_))
        torch.cuda.synchronize()
        ev_cost = sorted(a_.elapsed_time(b_) * 1e-3 for a_, b_ in empty)[len(empty) // 2]
        if ts:
            raw = ts[len(ts) // 2]
            mid = max(raw - ev_cost, 1e-9)
            in_step = {"kernel_ms": round(mid * 1e3, 5), "achieved": round(ffn_flops / mid / 1e12, 1),
                       "frac": round(ffn_flops / mid / 1e12 / MFMA_BF16_PEAK_TF, 4), "launches_timed": len(ts),
                       "event_pair_ms": round(raw * 1e3, 5), "empty_event_pair_ms": round(ev_cost * 1e3, 5),
                       "note": "median over the pair + qkv launches of 3 headline steps, one HIP event pair per launch on the step's "
                               "stream, minus the median cost of an empty event pair behind a busy stream (the timed region of `value` "
                               "has no events)"}
    # What bounds that kernel's main loops: every workgroup (= every CU: 249 workgroups of 64 rows) streams ALL
    # packed weights of the launch (2 x 2 MiB + 384 KiB) L2 -> registers, with 4 MFMAs (the workgroup's 4 row tiles) per 1 KiB
    # fragment; more rows per workgroup would need a second 64 x 256 accumulator tile per wave (512 registers) and M = 15 936 gives
    # the 256 CUs only 62 rows each.  The probe measures what one CU sustains in exactly that pattern with every CU doing the same:
    # floor = weight bytes per workgroup / that rate; the launch cannot be faster than this however the loop is scheduled.
    ws_buf = torch.zeros(2 << 20, dtype=torch.uint8, device=dev)
    ws_sink = torch.zeros(4, device=dev)
    ws_rounds = 128  # 2 MiB per wave, 8 MiB per CU per launch
    ws_s = event_time(lambda: lib.ma_weight_stream_probe(_host.ptr(ws_buf), ws_buf.numel(), ws_rounds, _host.ptr(ws_sink),
                                                         _host.current_stream_ptr()), 20)
    ws_gbs_cu = 4 * ws_rounds * 16 * 1024 / ws_s / 1e9
    ws_bytes_wg = int(pa.numel() * pa.element_size() + pb.numel() * pb.element_size() + pq.numel() * pq.element_size())
    weight_stream = {"bytes_per_workgroup": ws_bytes_wg, "probe_GBps_per_cu": round(ws_gbs_cu, 1),
                     "floor_us": round(ws_bytes_wg / ws_gbs_cu / 1e3, 2),
                     "frac_of_floor": round(ws_bytes_wg / ws_gbs_cu / 1e3 / (gemm_s * 1e6), 4),
                     "note": "packed weight bytes every workgroup streams L2 -> VGPR per launch / the rate ONE CU sustains on that "
                             "pattern (1 KiB fragments, 16-slot ring, 4 MFMAs per fragment, all CUs streaming; ma_weight_stream_probe, "
                             "measured live), over the kernel time"}

    # ---- roofline of the fbank kernel (HBM bound): algorithmic bytes = waves in + features out, at the headline batch (64)
    #      and at 512 utterances (where the launch's fixed cost is amortised) ----------------------------------------------
    n_frames = 1 + SAMPLES // HOP
    win = _host.device_window("hann", N_FFT, N_FFT, dev)
    bank = _host.device_htk_bank(N_FFT, 0.0, float(SR // 2), N_MELS, SR, dev)
    stream = _host.current_stream_ptr()

    def fbank_roofline(nb):
        xb = torch.from_numpy(synth_batch(4321 + rank)).to(dev).repeat(nb // BATCH, 1) if nb != BATCH else \
            torch.from_numpy(synth_batch(1234 + rank)).to(dev)
        ws = torch.empty(lib.ma_fbank_workspace_bytes(nb, n_frames), dtype=torch.uint8, device=dev)
        fo = torch.empty((nb, N_MELS, n_frames), device=dev)

        def launch():
            rc = lib.ma_fbank_db_f32(_host.ptr(xb), nb, SAMPLES, xb.stride(0), N_FFT, HOP, _host.ptr(win), 1, 1,
                                     bank.ref(), 2.0, 10.0, 1e-10, 0.0, -1.0, _host.ptr(fo), _host.ptr(ws), ws.numel(),
                                     stream)
            assert rc == 0

        s = event_time(launch, max(args.steps, 50) if nb == BATCH else 20)
        nbytes = nb * SAMPLES * 4 + nb * N_MELS * n_frames * 4  # 61 460 480 B at 64 utterances
        return s, nbytes

    fb_s, fb_bytes = fbank_roofline(BATCH)
    fb_gbs = fb_bytes / fb_s / 1e9
    fb512_s, fb512_bytes = fbank_roofline(512)
    fb512_gbs = fb512_bytes / fb512_s / 1e9

    # ---- the fbank kernel's SECOND roofline: vector-instruction issue.  DESIGN 4.1 says the kernel is bound by VALU issue + its
    #      per-wave dependency chain, not by HBM bytes; this makes the statement checkable: (VALU wave-instructions per launch, PMC
    #      constant of profiles/traffic.json) x (issue time of one wave-instruction per SIMD, measured LIVE on this chip at the
    #      kernel's occupancy of 3 waves per SIMD by ma_valu_issue_probe) / 1024 SIMDs = the time the vector pipes need for the
    #      instructions alone; frac_of_floor = that floor / the measured kernel time. ------------------------------------------
    fb_valu = None
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as fh:
            n_valu = int(json.load(fh)["feat512_kernel"]["valu_wave_insts"])
        sink = torch.zeros(4, device=dev)
        iters, wgs = 2000, 3
        probe_s = event_time(lambda: lib.ma_valu_issue_probe(wgs, iters, _host.ptr(sink), stream), 10)
        ns_inst = probe_s * 1e9 / (16 * iters * wgs)
        n_simd = torch.cuda.get_device_properties(dev).multi_processor_count * 4
        floor_us = n_valu / n_simd * ns_inst * 1e-3
        fb_valu = {"wave_insts": n_valu, "issue_ns_per_inst": round(ns_inst, 4), "simds": n_simd, "floor_us": round(floor_us, 3),
                   "frac_of_floor": round(floor_us / (fb_s * 1e6), 4),
                   "note": "VALU wave-instructions per launch (PMC SQ_INSTS_VALU) x live issue time per wave-instruction per SIMD "
                           "(16 x 2000 independent v_fma_f32 per wave, 3 waves per SIMD) / SIMDs, over the kernel time"}
    except (OSError, KeyError, ValueError):
        pass

    def pmc_traffic(kernel):
        """(HBM bytes per launch of `kernel`, where that was measured) from the committed PMC summary: rocprofv3 cannot run inside
        the bench, so the figure is a constant of the commit `traffic_measured_at` names; `traffic_source_current` says whether the
        kernel's source file still hashes to what was profiled (false = the constant is stale)."""
        import hashlib

        try:
            with open(os.path.join(ROOT, "profiles", "traffic.json")) as fh:
                tr = json.load(fh)
            ent = tr[kernel]
            cur = None
            if ent.get("source") and ent.get("source_sha16"):
                with open(os.path.join(ROOT, ent["source"]), "rb") as fh:
                    cur = hashlib.sha256(fh.read()).hexdigest()[:16] == ent["source_sha16"]
            return int(ent["bytes"]), {"traffic_measured_at": tr.get("measured_at_commit"), "traffic_source_current": cur}
        except (OSError, KeyError, ValueError):
            return None, {"traffic_measured_at": None, "traffic_source_current": None}

    # ---- cfg 3 (BASELINE.json configs[2]): Conformer-small forward at its stated batch, 32 x 1000 x 80 (features resident, no
    #      fbank), eval mode and training-mode forward (dropout 0.1, BatchNorm batch statistics).  Own encoder instance: the
    #      training-mode forward moves the BatchNorm running statistics. ----------------------------------------------------
    cfg3 = None
    if not args.train and not args.no_cfg3:
        torch.manual_seed(777)
        enc3 = ConformerEncoder(80, 256, 4, 2048, 12).eval().to(dev).prepare()
        x3 = torch.randn(32, FRAMES, 80, device=dev, generator=gen)
        m3 = torch.ones(32, 1, t2, device=dev)
        flops3 = 32 * 23.12e9
        ev = event_time(lambda: enc3(x3, m3), 30)
        cfg3 = {"workload": "Conformer-small (12 blocks) encoder forward, 32 x 1000 x 80, bf16 matmuls",
                "eval": {"ms": round(ev * 1e3, 4), "utt_s": round(32 / ev, 1), "tflops": round(flops3 / ev / 1e12, 1)}}
        enc3.train()
        # (the train-mode forward is walked from Python, ~150 launches in 2.4 ms: host-bound, and the CPU baseline child may be busy beside
        # it: one 10-step measurement gave 2.4 - 3.2 ms run to run).  Reported: the MEDIAN of three short measurements, like every other
        # figure of this line; the three are kept next to it (a best-of-N is biased downward)
        tr3s = sorted(event_time(lambda: enc3(x3, m3), 10) for _ in range(3))
        tr3 = tr3s[1]
        enc3.eval()
        cfg3["train_mode_forward"] = {"ms": round(tr3 * 1e3, 4), "utt_s": round(32 / tr3, 1),
                                      "tflops": round(flops3 / tr3 / 1e12, 1), "stat": "median of 3 x 10 steps",
                                      "ms_all": [round(t * 1e3, 4) for t in tr3s]}
        del enc3, x3

    # ---- cfg 5 (BASELINE.json configs[4]): ECAPA-TDNN forward, 256 x 300 x 80, eval-mode BatchNorm, C = 512 (class default) and
    #      C = 1024 (the example's size).  hbm_frac = HBM bytes per forward (PMC constant of profiles/traffic.json) / time / 8 TB/s. --
    cfg5 = None
    if not args.train and not args.no_cfg5 and world == 1:
        from mindaudio_amd.models import EcapaTDNN

        cfg5 = {"workload": "EcapaTDNN forward, 256 x 300 x 80, eval-mode BatchNorm, bf16 matmuls"}
        x5 = torch.randn(256, 300, 80, device=dev, generator=gen)
        for c, fl in ((512, 2.88e9), (1024, 10.78e9)):
            torch.manual_seed(0)
            m5 = EcapaTDNN(80, channels=(c, c, c, c, 3 * c)).eval().to(dev).prepare()
            s5 = event_time(lambda: m5(x5), 20)
            nb, meta = pmc_traffic("ecapa_c%d" % c)
            cfg5["c%d" % c] = {"ms": round(s5 * 1e3, 4), "utt_s": round(256 / s5, 1), "tflops": round(256 * fl / s5 / 1e12, 1),
                               "mfma_frac": round(256 * fl / s5 / 1e12 / MFMA_BF16_PEAK_TF, 4), "hbm_bytes": nb,
                               "hbm_frac": None if nb is None else round(nb / s5 / 1e9 / HBM_PEAK_GBS, 4)}
            del m5
        del x5

    hybrid = bucket_cycle = None
    if not args.train and not args.no_train_leg:
        train = train_leg(rank, world, dev, dist if world > 1 else None, args.train_steps, 2, barrier, args.force_collective,
                          args.train_digest, default_stream=args.train_default_stream)
        if not args.no_hybrid_leg and world == 1 and not args.force_collective:
            import gc

            gc.collect()  # (an engine is a reference cycle: the first leg's launch tables and tape must not stay allocated - and be
            torch.cuda.empty_cache()  # walked by a collection in the middle of a timed step - under the second leg)
            hybrid = train_leg(rank, world, dev, None, max(5, args.train_steps // 2), 2, barrier, ctc_weight=0.3)
            if not args.no_bucket_leg:
                # what an epoch of real data looks like to the step: another batch shape every time (round 6: tools/bucket_cycle_bench.py)
                gc.collect()
                torch.cuda.empty_cache()
                try:
                    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
                    import bucket_cycle_bench

                    # (settle: the caching allocator still grows in the first cycling rounds - five device allocations inside two timed
                    # rounds made this leg read 10.4-10.7 ms against 9.5 in steady state; the object reports them)
                    bucket_cycle = bucket_cycle_bench.run(0.3, rounds=4, settle=5, single_warm=3, single_timed=3)
                except Exception as e:  # (a reported leg, never the reason the headline line is missing)
                    bucket_cycle = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
                gc.collect()
                torch.cuda.empty_cache()

    if rank == 0:
        res = headline()
        if not args.train and sustained is not None:
            res["sustained"] = sustained
        res["roofline"] = {"bound": "mfma", "kernel": "ffn_packed_kernel, pair + qkv form (2 x [w_1 -> Swish -> w_2 + residual] + 4 LayerNorms + linear_q/k/v, "
                                                      "M=%d d=256 hidden=%d)" % (m, hid),
                           "achieved": round(gemm_tf, 1), "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s",
                           "frac": round(gemm_tf / MFMA_BF16_PEAK_TF, 4), "traffic": pmc_traffic("ffn_packed_kernel")[0],
                           "algorithmic_flops_per_launch": int(ffn_flops), "kernel_ms": round(gemm_s * 1e3, 5),
                           "timed": "back to back (the kernel's own rate); in_step = the same launch inside the headline step",
                           "in_step": in_step, "weight_stream": weight_stream}
        res["roofline"].update(pmc_traffic("ffn_packed_kernel")[1])
        res["roofline_fbank"] = {"bound": "hbm", "kernel": "feat512_kernel<mel>", "achieved": round(fb_gbs, 1),
                                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(fb_gbs / HBM_PEAK_GBS, 4),
                                 "traffic": pmc_traffic("feat512_kernel")[0], "algorithmic_bytes_per_launch": fb_bytes,
                                 "kernel_ms": round(fb_s * 1e3, 5),
                                 "batch512": {"achieved": round(fb512_gbs, 1), "frac": round(fb512_gbs / HBM_PEAK_GBS, 4),
                                              "algorithmic_bytes_per_launch": fb512_bytes,
                                              "kernel_ms": round(fb512_s * 1e3, 5)}}
        res["roofline_fbank"].update(pmc_traffic("feat512_kernel")[1])
        if fb_valu is not None:
            res["roofline_fbank"]["valu"] = fb_valu
        if cfg3 is not None:
            res["cfg3"] = cfg3
        if cfg5 is not None:
            res["cfg5"] = cfg5
        if train is not None and not args.train:
            res["train_dp"] = train
            if hybrid is not None:
                res["train_dp_hybrid"] = hybrid
            if bucket_cycle is not None:
                res["train_bucket_cycle"] = bucket_cycle
        if cpu is not None:
            res["cpu_baseline"] = cpu
        print(json.dumps(res))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
