#!/usr/bin/env python3
"""Headline benchmark: faces/s for 224×224 embed + match (BASELINE.json), MI355X.

A "step" = one pass of the hot path over one batch of synthetic faces already resident in HBM:
fp32 NCHW batch → ResNet-18 embedding (HIP kernels, bf16 MFMA) → L2-normalise → top-1 match against the
gallery.  Default execution: the step is captured once into a HIP graph and replayed, the batch split into
two micro-batches on concurrent streams (`frmap_amd.GraphedEmbedMatch`); `--graph 0 --streams 1` runs the
same kernels as plain eager launches on one stream (the mode the committed rocprofv3 profiles are taken in).

Workloads (BASELINE.json `configs`):
  N = 1   configs[1]: ResNet18 ('cnn') bf16 embed+match, batch 256, 36-ID gallery  (the driver's BENCH line)
  N > 1   configs[3]: ResNet18-ArcFace, 1024 faces per GPU (8192 on 8 GPUs), 10 000-ID gallery, one RCCL
          all-gather of the 8-byte (id, distance) records per step (weak scaling: faces shard embarrassingly)
  `--model/--batch/--gallery` override either.

Launch: under `torch.distributed.run` (RANK / WORLD_SIZE in the environment) every rank runs `worker()`;
`--gpus N` must then equal WORLD_SIZE.  Started plainly with `--gpus N > 1`, this process becomes a
LAUNCHER: it never touches the GPU (no torch.cuda / HIP call), spawns N fresh rank processes with
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set, relays their output (rank 0 prints
the JSON line) and exits non-zero if any rank does.  `FRMAP_BENCH_BACKEND=gloo` rehearses the N > 1 control
flow on a box with fewer GPUs than ranks (ranks share devices; the collective runs over gloo on host copies).

A plain run sets up, runs the settle and warm-up steps, times exactly `--steps` steps, writes the last timed step's outputs
when `--dump-outputs DIR` is given, and prints the result line.  Everything else it can measure or check (roofline, cpu_baseline,
fp16_value / u8_input_value, scale_ref; shard_check / local_only at N > 1) runs only under `--full`; without it those fields are
null or absent.

`--dump-outputs DIR` writes what the timed step returns to its caller, from the last timed step (rank 0: the gathered records of
every rank at N > 1): `DIR/top1_index.npy` (float64; the matched gallery row, or the unknown id) and `DIR/top1_distance.npy`
(float32), one entry per face.  The inputs, weights and gallery are seeded, so the same arguments give the same inputs in every run.

Prints ONE JSON line on rank 0 (contract in the task statement) with:
  ms_per_step   — wall time of the timed region ÷ `--steps` (host clock, synchronised at both ends).
  roofline      — (--full) the dominant kernel (conv3x3_pp_kernel<BF16>: the 3×3 stride-1 implicit-GEMM
                  convolutions of layers 2-4): algorithmic FLOPs per launch ÷ its average launch duration,
                  measured with HIP events on the launch stream in an instrumented pass after the timed region
                  ('cnn' / 'arcface': the model handle's own per-launch trace, frmap_model_trace; other families: the per-op wrappers)
                  (standalone eager launches at the full per-GPU batch on one stream: per-kernel durations are not
                  defined for kernels that share the GPU with another stream's, and rocprofv3 serialises the
                  streams).  peak = 2.5 PFLOP/s dense bf16.  `layerwise` lists every kernel of the step with its
                  algorithmic FLOPs / bytes, measured µs and roof time max(FLOP/peak, bytes/8 TB/s);
                  `frac_layerwise` = Σ roof time ÷ measured.  `traffic` is the STORED rocprofv3 PMC measurement
                  (profiles/*.json; PMC counters cannot be read from inside the process).
  cpu_baseline  — (--full) the CPU oracle (oracle/face_oracle.py, fp32 PyTorch restatement of the reference's forward)
                  timed on this box's host cores on a bounded sample (rank 0, N = 1 only).
  fp16_value    — (--full) the same step in fp16 (the precision the north-star's 1e-3 / identical-top-1 tolerance is stated
                  for), timed after the bf16 region in the same process (N = 1 only).
  settle_steps  — untimed steps run BEFORE the W warm-up steps (clock / power-state ramp of a fresh process).
  step_ms       — median / p10 / p90 / min / max of the per-step durations of the timed region (HIP events between the steps).
  scale_ref     — (--full, N = 1) the N > 1 workload's per-GPU shape on this one GPU: the like-for-like denominator of a scaling curve.
  shard_check / local_only — (--full, N > 1) identical inputs gave bit-identical records on every rank (the run aborts otherwise); the same
                  per-GPU step without the collective.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0   # dense bf16/fp16, MI355X_MICROARCH.md
# what a tuned bf16 GEMM sustains on RANDOM operands on this part (MI355X_MICROARCH.md 'DVFS give-back' (1): 1 247 TFLOP/s at
# 1.90-1.95 GHz; 1 483 on zeros): context for `frac`, which stays priced against the nominal peak
MFMA_PRACTICAL_TFLOPS = 1247.0
HBM_PEAK_GBS = 8000.0       # HBM3E spec, MI355X_MICROARCH.md (≈6.3 TB/s achievable)
TRAFFIC_PROFILE = "r03_hbm_traffic_pmc.json"


def step_stats(ms):
    """Spread of the per-step durations (HIP events recorded between the steps of the timed region)."""
    v = sorted(float(t) for t in ms)
    if not v:
        return None

    def q(f):
        i = f * (len(v) - 1)
        lo = int(i)
        hi = min(lo + 1, len(v) - 1)
        return v[lo] + (v[hi] - v[lo]) * (i - lo)
    return {"n": len(v), "median": round(q(0.5), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4),
            "min": round(v[0], 4), "max": round(v[-1], 4)}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--settle-steps", type=int, default=150, dest="settle_steps",
                    help="untimed steady-state settling steps before the warm-up steps (clock / power-state ramp); "
                         "reported as `settle_steps` in the JSON")
    ap.add_argument("--batch", type=int, default=None, help="faces per GPU per step (default 256 at N=1, 1024 at N>1)")
    ap.add_argument("--gallery", type=int, default=None, help="gallery identities (default 36 at N=1, 10000 at N>1)")
    ap.add_argument("--model", default=None, choices=["cnn", "arcface", "baseline", "siamese", "hybrid", "attention"],
                    help="default: cnn at N=1 (configs[1]), arcface at N>1 (configs[3])")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--input", default="f32", choices=["f32", "u8"],
                    help="f32: fp32 NCHW crops (the reference's tensor layout, headline); u8: uint8 HWC crops normalised inside the stem")
    ap.add_argument("--streams", type=int, default=2, help="split the per-GPU batch over this many concurrent HIP streams")
    ap.add_argument("--graph", type=int, default=1, help="1: replay the step from a captured HIP graph (0: eager launches)")
    ap.add_argument("--full", action="store_true",
                    help="also run the side measurements and checks after the timed steps: roofline + per-kernel table, CPU baseline, "
                         "fp16 / uint8-input variants, scale_ref (N = 1); shard_check before and local_only after the timed steps (N > 1)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", dest="dump_outputs",
                    help="write the last timed step's outputs (top-1 index and distance per face) to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline pass")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the fp16 / uint8-input / scale_ref side measurements")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """Write ``name -> numpy array`` as ``out_dir/<name>.npy``.  All arrays share their leading (per-face) axis; if together they
    exceed DUMP_LIMIT_BYTES, the same fixed, seeded sample of faces is taken from each and its face numbers go to
    ``sample_index.npy``."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    n = len(next(iter(arrays.values())))
    per_face = sum(a.nbytes for a in arrays.values()) / max(n, 1)
    keep = int(DUMP_LIMIT_BYTES // max(per_face + 8, 1))
    if n > keep:
        idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
        arrays["sample_index"] = idx.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


# ------------------------------------------------------------------------------------------------
# launcher (parent of the rank processes): must not touch the GPU
# ------------------------------------------------------------------------------------------------
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int, argv, worker_cmd=None, timeout: float = None) -> int:
    """Spawn ``n`` rank processes of ``worker_cmd + argv`` (default: this script) with the torch.distributed
    environment (RANK, LOCAL_RANK, WORLD_SIZE, LOCAL_WORLD_SIZE, MASTER_ADDR=127.0.0.1, MASTER_PORT) and wait.
    stdout/stderr are inherited (rank 0 prints the JSON line).  Returns 0 iff every rank exited 0; on the first
    failure the remaining ranks (exactly the PIDs started here) are terminated."""
    cmd = list(worker_cmd) if worker_cmd else [sys.executable, os.path.abspath(__file__)]
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), FRMAP_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen(cmd + list(argv), env=env))
    t0 = time.time()
    rc = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench launcher: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr, flush=True)
        if rc != 0 or (timeout is not None and time.time() - t0 > timeout):
            if rc == 0:
                rc = 124
            for r in live:
                procs[r].terminate()
            for r in live:
                try:
                    procs[r].wait(15)
                except subprocess.TimeoutExpired:
                    procs[r].kill()
            break
        if live:
            time.sleep(0.05)
    return rc


# ------------------------------------------------------------------------------------------------
# per-kernel instrumentation for the roofline objects
# ------------------------------------------------------------------------------------------------
def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _conv_kernel_name(dt, Cin, k, stride, H, W, ds, Cout=0, B=0):
    """Label of the kernel frmap_conv_igemm dispatches this layer to (the library answers for the second-generation
    kernel; the first-generation rules are restated here for labelling only)."""
    if k == 3 and stride == 1 and not ds:
        from frmap_amd import _lib
        lay = _lib.load().frmap_conv3x3_pp_layout(B, H, W, Cin, Cout)
        if lay:
            return f"conv3x3_pp_kernel<{dt}>"
    if k == 3 and stride == 2 and not ds:
        from frmap_amd import _lib
        if _lib.load().frmap_conv3x3s2_pp_layout(B, H, W, Cin, Cout):
            return f"conv3x3s2_pp_kernel<{dt}>"
    if ds:
        return f"conv3x3_fast_kernel<{dt}, true>"
    if k == 1:
        from frmap_amd import _lib
        if Cin >= 128 and _lib.load().frmap_conv1x1_pp_layout(B, H, W, Cin, Cout, stride):
            return f"conv1x1_pp_kernel<{dt}>"
        return f"conv1x1_kernel<{dt}>"
    if stride == 2:
        return f"conv3x3s2_fast_kernel<{dt}>"
    if Cin == 64 and H % 8 == 0 and W % 8 == 0:
        return f"conv3x3_c64_wave_kernel<{dt}>"
    return f"conv3x3_fast_kernel<{dt}, false>"


def instrument(ops, torch, dt):
    """Wrap the op wrappers the embed+match step calls with HIP-event timers; returns (records, restore).
    A record = dict(kernel, flop, bytes, e0, e1): algorithmic FLOPs (2·MAC of the contraction) and algorithmic
    bytes (operands read once + output written once) of that launch."""
    records, saved = [], {}

    def wrap(name, describe):
        orig = getattr(ops, name)
        saved[name] = orig

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(*a, **kw)
            e1.record()
            kern, flop, nbytes = describe(out, *a, **kw)
            records.append(dict(kernel=kern, flop=float(flop), bytes=float(nbytes), e0=e0, e1=e1))
            return out
        setattr(ops, name, timed)

    def d_conv(out, x, wpk, shift, Cout, k, stride, pad, relu, residual=None):
        B, H, W, Cin = x.shape
        flop = 2.0 * out.shape[0] * out.shape[1] * out.shape[2] * Cout * Cin * k * k
        return _conv_kernel_name(dt, Cin, k, stride, H, W, False, Cout, B), flop, _nbytes(x) + _nbytes(out) + _nbytes(wpk) + _nbytes(residual)

    def d_conv_ds(out, x, wpk, shift, Cout, x_ds, wpk_ds, ds_stride, relu):
        B, H, W, Cin = x.shape
        M = out.shape[0] * out.shape[1] * out.shape[2]
        flop = 2.0 * M * Cout * (Cin * 9 + x_ds.shape[3])
        gathered = M * x_ds.shape[3] * x_ds.element_size()      # only the strided pixels are needed
        from frmap_amd import _lib
        name = _conv_kernel_name(dt, Cin, 3, 1, H, W, True)
        if _lib.load().frmap_conv3x3_pp_ds_layout(B, H, W, Cin, Cout, x_ds.shape[1], x_ds.shape[2], x_ds.shape[3], ds_stride):
            name = f"conv3x3_pp_kernel<{dt}, DS>"
        return name, flop, _nbytes(x) + _nbytes(out) + _nbytes(wpk) + _nbytes(wpk_ds) + gathered

    def d_stem(out, x, wpk, shift, dtype, pool3=True):
        B, _, H, W = x.shape
        Hc, Wc = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        name = "stem_s2d_kernel" if (pool3 and W % 4 == 0) else "stem_pool_kernel"
        return f"{name}<{dt}>", 2.0 * B * Hc * Wc * 64 * 147, _nbytes(x) + _nbytes(out) + _nbytes(wpk)

    def d_stem_u8(out, x, wpk, shift, mean, std, dtype, pool3=True):
        B, H, W, _ = x.shape
        Hc, Wc = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        return f"stem_pool_u8_kernel<{dt}>", 2.0 * B * Hc * Wc * 64 * 147, _nbytes(x) + _nbytes(out) + _nbytes(wpk)

    def d_gnm(out, fmap, gallery, *a, **kw):
        B, H, W, C = fmap.shape
        G = 0 if gallery is None else gallery.shape[0]
        return f"gap_norm_match_kernel<{dt}>", 2.0 * B * C * G, _nbytes(fmap) + _nbytes(gallery) + 16 * B

    def d_head(out, fmap, wt, scale, shift, eps=1e-12, want_pre=False, relu=False):
        B, H, W, K = fmap.shape
        return f"gap_linear_norm_kernel<{dt}>", 2.0 * B * K * wt.shape[1], _nbytes(fmap) + _nbytes(wt) + _nbytes(out[0])

    def d_pool(out, x):
        return "avgpool_global_kernel", 0.0, _nbytes(x) + _nbytes(out)

    def d_lin(out, x, w, scale=None, shift=None, relu=False):
        return "linear_f32 (gemm_nt_f32_kernel)", 2.0 * x.shape[0] * x.shape[1] * w.shape[0], _nbytes(x) + _nbytes(w) + _nbytes(out)

    def d_l2(out, x, eps=1e-12):
        return "l2_normalize_kernel", 0.0, 2 * _nbytes(x)

    def d_match(out, emb, gallery, thresh=None, packed=False, prepared=None):
        G = 0 if gallery is None else gallery.shape[0]
        if prepared is not None and G >= ops.MATCH_MFMA_MIN_G:   # fp16 (hi, lo) split: 3 MFMA products per fp32 one
            return ("match_top1 (conv1x1_pp_kernel<F16, MATCH> + finalize)", 6.0 * emb.shape[0] * emb.shape[1] * G,
                    _nbytes(emb) + _nbytes(prepared.packed) + 16 * emb.shape[0])
        return "match_top1 (gemm_nt_f32_kernel + finalize)", 2.0 * emb.shape[0] * emb.shape[1] * G, _nbytes(emb) + _nbytes(gallery) + 16 * emb.shape[0]

    # the other model families' ops (bench.py --model baseline / siamese / hybrid / attention): generic descriptions - the
    # algorithmic bytes are the operand and result tensors, the FLOPs those of the contraction (0 for pure data movement)
    def _tensors(*xs):
        return sum(_nbytes(x) for x in xs if isinstance(x, torch.Tensor))

    def d_pool2(out, x, wpk, shift, Cout, relu):
        B, H, W, Cin = x.shape
        form = {3: "conv3x3_pp_kernel<PL>", 2: "conv3x3_c64_wave_kernel<POOL>", 1: "conv_igemm_kernel<POOL>"}.get(ops.conv_pool2_form(B, H, W, Cin, Cout), "conv+pool")
        return f"{form}<{dt}> (conv3x3 + 2x2 max-pool)", 2.0 * B * H * W * Cout * Cin * 9, _tensors(x, wpk, out)

    def d_c3pool(out, x4, wpk, shift, Cout, relu):
        B, H, W, _ = x4.shape
        return f"conv_small_cin_kernel<{dt}, POOL>", 2.0 * B * H * W * Cout * 27, _tensors(x4, wpk, out)

    def d_c3(out, x4, wpk, shift, Cout, k, stride, pad, relu):
        return f"conv_small_cin_kernel<{dt}>", 2.0 * out.shape[0] * out.shape[1] * out.shape[2] * Cout * 3 * k * k, _tensors(x4, wpk, out)

    def d_linmfma(out, x2d, wpk, shift, N, act=0, residual=None):
        return f"linear_mfma<{dt}> (1x1 MFMA kernels)", 2.0 * x2d.shape[0] * x2d.shape[1] * N, _tensors(x2d, wpk, out, residual)

    def d_move(label):
        def f(out, *a, **kw):
            outs = out if isinstance(out, (tuple, list)) else (out,)
            return label, 0.0, _tensors(*a) + _tensors(*outs)
        return f

    def d_mha(out, qkv, H):
        B, L, D3 = qkv.shape
        return f"mha_tokens_kernel<{dt}>", 4.0 * B * L * L * (D3 // 3), _tensors(qkv, out)

    for name, fn in (("conv_igemm_pool2", d_pool2), ("conv_small_cin_pool2", d_c3pool), ("conv_small_cin", d_c3), ("linear_mfma", d_linmfma),
                     ("maxpool", d_move("maxpool_kernel")), ("avgpool_adaptive", d_move("avgpool_adaptive_kernel")),
                     ("pack_input", d_move("pack_input_kernel")), ("add_pos_layernorm", d_move("add_pos_layernorm_kernel")),
                     ("mean_layernorm", d_move("mean_layernorm_kernel")), ("mha_tokens", d_mha),
                     ("cnn_attention", d_move("cnn_attention_kernel")), ("cast_to_f32", d_move("cast_to_f32_kernel"))):
        if hasattr(ops, name):
            wrap(name, fn)

    for name, fn in (("conv_igemm", d_conv), ("conv_igemm_ds", d_conv_ds), ("stem7x7_maxpool", d_stem),
                     ("stem7x7_maxpool_u8", d_stem_u8), ("gap_norm_match", d_gnm), ("gap_linear_norm", d_head), ("avgpool_global", d_pool),
                     ("linear_f32", d_lin), ("l2_normalize", d_l2), ("match_top1", d_match)):
        if hasattr(ops, name):
            wrap(name, fn)

    def restore():
        for k, v in saved.items():
            setattr(ops, k, v)
    return records, restore


def stored_traffic():
    """HBM traffic per bench-label from the committed rocprofv3 PMC passes (separate FETCH_SIZE / WRITE_SIZE runs of
    `bench.py --graph 0 --streams 1`, FETCH_SIZE doubled per the gfx950 correction).  The profile is keyed by the full
    template instantiation (e.g. `conv3x3_pp_kernel<BF16, 7, 2, 3, 1, false, false>`); a bench label such as
    `conv3x3_pp_kernel<BF16>` covers several of them, so the lookup returns, per label, the average HBM bytes per
    LAUNCH over the instantiations it covers, weighted by how often each was launched in the profiled run."""
    for name in (TRAFFIC_PROFILE, "r02_hbm_traffic_pmc.json", "r01_hbm_traffic_pmc.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                kernels = json.load(f)["kernels"]
        except Exception:
            continue

        def lookup(label):
            if label in kernels:
                return kernels[label]["hbm_bytes_per_launch"]
            head = label[:-1] + "," if label.endswith(">") else label      # "kernel<BF16>" -> "kernel<BF16,"
            want_ds = None
            if label.startswith("conv3x3_pp_kernel"):
                want_ds = ", DS>" in label
                head = label.split(",")[0].rstrip(">") + ","
            tot = n = 0
            for k, v in kernels.items():
                if not k.startswith(head):
                    continue
                if want_ds is not None and k.startswith("conv3x3_pp_kernel<"):
                    targs = k[k.index("<") + 1:].rstrip(">").split(", ")     # <T, MI, WM, NHP, KS, DS, IM[, PL, RI]>
                    if (len(targs) > 5 and targs[5] == "true") != want_ds:
                        continue
                c = max(v.get("launches_FETCH_SIZE", 0), 1)
                tot += v["hbm_bytes_per_launch"] * c
                n += c
            return int(tot / n) if n else None
        return name, lookup
    return None, (lambda label: None)


# ------------------------------------------------------------------------------------------------
# one rank
# ------------------------------------------------------------------------------------------------
def worker(args) -> int:
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus N` "
                         f"(spawns N ranks itself) or under torch.distributed.run with --nproc-per-node equal to --gpus")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    backend = os.environ.get("FRMAP_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > ndev:
        raise SystemExit(f"bench.py: {world} ranks but {ndev} visible GPU(s); RCCL needs one GPU per rank "
                         "(FRMAP_BENCH_BACKEND=gloo rehearses the control flow with shared devices)")
    local_dev = local_rank % ndev
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    rccl_ranks = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        world = dist.get_world_size()
        if backend == "nccl":
            # what RCCL itself saw: one int per rank through a real collective
            probe = torch.ones(1, device=dev, dtype=torch.int32)
            dist.all_reduce(probe)
            rccl_ranks = int(probe.item())

    import frmap_amd
    from frmap_amd import dist as fdist
    from frmap_amd import ops, synth

    cfg_multi = world > 1
    model_type = args.model or ("arcface" if cfg_multi else "cnn")
    B = args.batch or (1024 if cfg_multi else 256)
    G = args.gallery or (10000 if cfg_multi else 36)
    seeds = {"cnn": (1002, 2002, 3002), "arcface": (1004, 2004, 3004), "baseline": (1001, 2001, 3001), "siamese": (1006, 2006, 3006),
             "hybrid": (1005, 2005, 3005), "attention": (1007, 2007, 3007)}.get(model_type, (1002, 2002, 3002))
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    D = 256 if model_type == "siamese" else 512

    def build_model(dt):
        m = frmap_amd.get_model(model_type, 36)
        sd_ = synth.calibrated_state_dict(model_type, synth.shapes_of(m), seeds[0])   # = the parity tests' weights
        m.load_state_dict(sd_)
        return m.to(dev).eval().set_compute_dtype(dt), sd_

    model, sd = build_model(dtype)
    gallery = frmap_amd.Gallery([f"id{i}" for i in range(G)], synth.unit_rows(seeds[2], G, D), dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seeds[1] + rank)
    if args.input == "u8":   # uint8 HWC crops; ToTensor + Normalize happen inside the stem
        x = torch.randint(0, 256, (B, 224, 224, 3), device=dev, dtype=torch.uint8, generator=gen)
    else:
        x = torch.randn((B, 3, 224, 224), device=dev, dtype=torch.float32, generator=gen)  # resident in HBM
    need_norm = model_type in ("cnn", "baseline", "hybrid", "attention")
    total = B * world

    def make_local_step(mdl, xin, use_graph, nstreams, gallery=gallery, need_norm=need_norm):
        graphed, note = None, ""
        if use_graph:
            try:
                graphed = frmap_amd.GraphedEmbedMatch(mdl, gallery, xin, 1.0, normalize=need_norm, streams=nstreams)
            except Exception as e:  # capture refused: same kernels, eager launches
                note = f" (graph capture failed: {type(e).__name__}; eager launches)"
                torch.cuda.synchronize()
        side = [torch.cuda.Stream(device=dev) for _ in range(max(nstreams - 1, 0))]
        xs = list(xin.chunk(nstreams)) if nstreams > 1 else [xin]
        rec = torch.empty((xin.shape[0], 2), dtype=torch.int32, device=dev)

        def local_records():
            """int32 [B, 2] (id-or-unknown, bits(dist)) records of this rank's faces."""
            if graphed is not None:
                return graphed()
            if nstreams == 1:
                return frmap_amd.embed_and_match(mdl, xin, gallery, 1.0, normalize=need_norm, packed=rec)
            # micro-batches on concurrent streams, each writing its slice of the record buffer
            main = torch.cuda.current_stream()
            lo = xs[0].shape[0]
            for st, xi in zip(side, xs[1:]):
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    frmap_amd.embed_and_match(mdl, xi, gallery, 1.0, normalize=need_norm, packed=rec[lo: lo + xi.shape[0]])
                lo += xi.shape[0]
            frmap_amd.embed_and_match(mdl, xs[0], gallery, 1.0, normalize=need_norm, packed=rec[: xs[0].shape[0]])
            for st in side:
                main.wait_stream(st)
            return rec
        return local_records, graphed is not None, note

    local_records, is_graphed, graph_note = make_local_step(model, x, bool(args.graph), args.streams)

    # N > 1: the all-gather of step i (8 B/face, pure latency) runs on its own stream under step i+1's kernels;
    # the records are first copied out of the step's buffer (the next replay overwrites it)
    overlap = world > 1 and backend == "nccl" and os.environ.get("FRMAP_BENCH_OVERLAP_GATHER", "1") == "1"
    if overlap:
        comm = torch.cuda.Stream(device=dev)
        staging = [torch.empty((B, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        gathered = [torch.empty((world * B, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        ready_ev = [torch.cuda.Event() for _ in range(2)]
        copied_ev = [torch.cuda.Event() for _ in range(2)]
    state = {"n": 0}

    def step():
        if world == 1:
            r = local_records()
            return r[:, 0], r.view(torch.float32)[:, 1]
        if not overlap:
            return fdist.gather_packed(local_records())
        k = state["n"] & 1
        main = torch.cuda.current_stream()
        if state["n"] > 0:
            main.wait_event(copied_ev[k ^ 1])  # the previous step's records have left the buffer this step overwrites
        r = local_records()
        ready_ev[k].record(main)
        with torch.cuda.stream(comm):
            comm.wait_event(ready_ev[k])
            staging[k].copy_(r)
            copied_ev[k].record(comm)
            dist.all_gather_into_tensor(gathered[k], staging[k])
        state["n"] += 1
        return gathered[k][:, 0], gathered[k].view(torch.float32)[:, 1]

    if overlap:
        # self-check on the live system: one overlapped step must return exactly what the plain gather returns
        with torch.no_grad():
            try:
                ids_o, d_o = step()
                torch.cuda.synchronize()
                ids_p, d_p = fdist.gather_packed(local_records())
                torch.cuda.synchronize()
                same = bool(torch.equal(ids_o, ids_p)) and bool(torch.equal(d_o, d_p))
            except Exception:
                same = False
            flag = torch.tensor([1 if same else 0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                overlap = False  # (every rank takes the same decision)

    def timed_region(step_fn, settle, warmup, steps, collective, per_step=None, last=None):
        """settle + warmup untimed steps, then EXACTLY `steps` steps bracketed by barrier + synchronize on both sides.
        `per_step` (a list): receives the duration of every timed step in ms, from HIP events recorded on the launch stream
        between the steps (an event record is a host-side enqueue; nothing waits inside the region).
        `last` (a list): receives what the last timed step returned."""
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] if per_step is not None else None
        with torch.no_grad():
            for _ in range(max(settle, 0)):      # a fixed COUNT: every rank must issue the same number of collectives
                step_fn()
            torch.cuda.synchronize()
            for _ in range(max(warmup, 0)):
                step_fn()
            if collective:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if evs:
                evs[0].record()
            for i in range(steps):
                out = step_fn()
                if evs:
                    evs[i + 1].record()
            torch.cuda.synchronize()
            if collective:
                dist.barrier()
            el = time.perf_counter() - t0
        if evs:
            per_step.extend(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
        if last is not None:
            last.append(out)
        return el

    # N > 1: before anything is timed, every rank runs the SAME faces (one seed) through the same step and the gathered
    # records must hold `world` bit-identical segments: a rank's result does not depend on which GPU computed it.  (Holds
    # because every rank runs the same per-rank batch size, hence the same tile layouts and fp32 summation order; results
    # of DIFFERENT batch sizes agree only to rounding, tests/test_properties_gpu.py.)
    shard_check = None
    if world > 1 and args.full:
        gen_s = torch.Generator(device=dev)
        gen_s.manual_seed(seeds[1] + 4242)
        if args.input == "u8":
            x_same = torch.randint(0, 256, (B, 224, 224, 3), device=dev, dtype=torch.uint8, generator=gen_s)
        else:
            x_same = torch.randn((B, 3, 224, 224), device=dev, dtype=torch.float32, generator=gen_s)
        with torch.no_grad():
            rec_same = frmap_amd.embed_and_match(model, x_same, gallery, 1.0, normalize=need_norm, packed=True)
            ids_all, d_all = fdist.gather_packed(rec_same)
            torch.cuda.synchronize()
        ok = fdist.replicated_shards_identical(ids_all, d_all, world) and \
            bool(torch.equal(ids_all[:B].to(rec_same.device), rec_same[:, 0]))
        flag = torch.tensor([1 if ok else 0], device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            raise SystemExit(f"bench.py rank {rank}: identical inputs gave different top-1 records on different ranks")
        shard_check = {"identical_inputs_on_all_ranks": "bit-identical (id, distance) records from every rank",
                       "faces": B, "condition": "equal per-rank batch size (same tile layouts / fp32 summation order)"}
        del x_same, rec_same

    per_step_ms, last_out = [], []
    local_elapsed = timed_region(step, args.settle_steps, args.warmup, args.steps, world > 1, per_step_ms, last_out)
    if args.dump_outputs and rank == 0:
        ids_last, dist_last = last_out[0]
        dump_outputs(args.dump_outputs, {"top1_index": ids_last.cpu().numpy().astype("float64"),
                                         "top1_distance": dist_last.cpu().numpy().astype("float32")})
    elapsed_t = torch.tensor([local_elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    if world > 1:
        dist.all_reduce(elapsed_t, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed_t.item())
    faces_per_s = total * args.steps / elapsed
    dt = "BF16" if dtype == torch.bfloat16 else "F16"

    # N > 1: the same per-GPU step WITHOUT the collective, all ranks at once (same power / thermal conditions as the
    # timed region): value / (N * local_only) isolates what the all-gather and rank skew cost
    local_only = None
    if world > 1 and args.full:
        t_loc = timed_region(lambda: local_records(), 20, args.warmup, args.steps, True)
        v = torch.tensor([B * args.steps / t_loc], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        vmin = v.clone()
        dist.all_reduce(vmin, op=dist.ReduceOp.MIN)
        local_only = {"per_gpu_value_rank0": round(float(v.item()), 1), "per_gpu_value_slowest_rank": round(float(vmin.item()), 1),
                      "what": "the same step without the all-gather, every rank at once, faces/s per GPU"}

    # ---------------- roofline: per-kernel instrumented pass (not part of `value`) ----------------
    roofline = None
    if rank == 0 and args.full and not args.no_roofline:
        import frmap_amd.face_models as fm
        import frmap_amd.matching as mt_
        assert fm.ops is ops and mt_.ops is ops
        records, restore = instrument(ops, torch, dt)
        # 'cnn' / 'arcface' run on a model handle of the C ABI: its per-launch trace (HIP events recorded by the library around
        # every launch of the forward) supplies the records; the other families are timed through the per-op wrappers
        handle = model.model_handle() if hasattr(model, "model_handle") else None
        if handle is None:   # AttentionNet: its ResNet-18 trunk runs on a 'resnet18_trunk' handle, the attention head through per-op calls
            plan = model._get_plan() if hasattr(model, "_get_plan") else None
            trunk = plan.get("trunk") if isinstance(plan, dict) else None
            handle = getattr(trunk, "handle", None)
        NREP = 5
        try:
            if handle is not None:
                handle.trace(True)
            with torch.no_grad():
                for _ in range(NREP):  # rank-local, eager, one stream, full per-GPU batch
                    frmap_amd.embed_and_match(model, x, gallery, 1.0, normalize=need_norm)
            torch.cuda.synchronize()
        finally:
            restore()
            if handle is not None:
                handle.trace(False)
                records.extend(dict(kernel=k, flop=fl, bytes=nb, us=us) for k, fl, nb, us in handle.trace_read())
        prof_name, pmc = stored_traffic()
        per = {}
        for r in records:
            a = per.setdefault(r["kernel"], dict(launches=0, flop=0.0, bytes=0.0, us=0.0))
            a["launches"] += 1
            a["flop"] += r["flop"]
            a["bytes"] += r["bytes"]
            a["us"] += r["us"] if "us" in r else r["e0"].elapsed_time(r["e1"]) * 1e3
        layerwise, roof_total, meas_total = [], 0.0, 0.0
        for kname, a in per.items():
            n = a["launches"] // NREP
            flop, nbytes, us = a["flop"] / NREP, a["bytes"] / NREP, a["us"] / NREP
            roof_us = max(flop / (MFMA_PEAK_TFLOPS * 1e12), nbytes / (HBM_PEAK_GBS * 1e9)) * 1e6
            roof_total += roof_us
            meas_total += us
            pm = pmc(kname)
            layerwise.append({"kernel": kname, "launches_per_step": n, "flop": flop, "bytes": nbytes, "us": round(us, 2),
                              "roof_us": round(roof_us, 2), "bound": "mfma" if flop / (MFMA_PEAK_TFLOPS * 1e12) >= nbytes / (HBM_PEAK_GBS * 1e9) else "hbm",
                              "tflops": round(flop / us / 1e6, 1) if us > 0 else None, "gbs": round(nbytes / us / 1e3, 1) if us > 0 else None,
                              "pmc_bytes": int(pm * n) if pm is not None else None})
        # the dominant kernel = the one with the largest share of the step's time
        dom_name = max(per, key=lambda kn: per[kn]["us"]) if per else None
        dom = per.get(dom_name)
        if dom:
            dflop_t, dbyte_t = dom["flop"] / (MFMA_PEAK_TFLOPS * 1e12), dom["bytes"] / (HBM_PEAK_GBS * 1e9)
            if dflop_t >= dbyte_t:   # MFMA-bound: algorithmic FLOP / measured time against the dense bf16 peak
                bound, achieved, peak, unit = "mfma", dom["flop"] / dom["us"] / 1e6, MFMA_PEAK_TFLOPS, "TFLOP/s"
            else:                    # HBM-bound: algorithmic bytes / measured time against the HBM peak
                bound, achieved, peak, unit = "hbm", dom["bytes"] / dom["us"] / 1e3, HBM_PEAK_GBS, "GB/s"
            roofline = {"bound": bound, "kernel": dom_name, "achieved": round(achieved, 2), "peak": peak,
                        "unit": unit, "frac": round(achieved / peak, 4),
                        "traffic": pmc(dom_name), "traffic_source": {"stored": f"profiles/{prof_name}"} if prof_name else None,
                        "measured": "standalone eager launches at the full per-GPU batch, one stream (instrumented pass, HIP events)",
                        "launches_per_step": dom["launches"] // NREP, "avg_launch_us": round(dom["us"] / dom["launches"], 2),
                        "flop_per_launch": dom["flop"] / dom["launches"],
                        "layerwise": layerwise,
                        "layerwise_roof_us": round(roof_total, 1), "layerwise_measured_us": round(meas_total, 1),
                        "frac_layerwise": round(roof_total / meas_total, 4) if meas_total > 0 else None,
                        "frac_layerwise_of_step": round(roof_total / (elapsed / args.steps * 1e6), 4),
                        "peaks": {"mfma_tflops": MFMA_PEAK_TFLOPS, "hbm_gbs": HBM_PEAK_GBS,
                                  "mfma_tflops_tuned_gemm_random_data": MFMA_PRACTICAL_TFLOPS},
                        "frac_of_tuned_gemm_rate": round(achieved / MFMA_PRACTICAL_TFLOPS, 4) if bound == "mfma" else None}

    # ---------------- side measurements (N = 1, rank 0; outside the timed region) ----------------
    extras = {}
    if rank == 0 and world == 1 and args.full and not args.no_extras and model_type in ("cnn", "arcface"):
        try:
            if args.dtype == "bf16":
                m16, _ = build_model(torch.float16)
                rec16, _, _ = make_local_step(m16, x, bool(args.graph), args.streams)
                t16 = timed_region(rec16, 50, args.warmup, args.steps, False)
                extras["fp16_value"] = round(B * args.steps / t16, 1)
                del m16, rec16
            if getattr(model, "supports_u8_input", False) and args.input == "f32":
                gen8 = torch.Generator(device=dev)
                gen8.manual_seed(seeds[1] + 77)
                x8 = torch.randint(0, 256, (B, 224, 224, 3), device=dev, dtype=torch.uint8, generator=gen8)
                rec8, _, _ = make_local_step(model, x8, bool(args.graph), args.streams)
                t8 = timed_region(rec8, 50, args.warmup, args.steps, False)
                extras["u8_input_value"] = round(B * args.steps / t8, 1)
                del rec8
        except Exception as e:  # a side measurement must never cost the headline line
            extras["extras_error"] = f"{type(e).__name__}: {e}"
        torch.cuda.synchronize()

    # ---------------- scale_ref: the multi-GPU workload's per-GPU shape on ONE GPU (N = 1 only) ----------------
    # `--gpus N > 1` measures configs[3] (arcface, 1024 faces per GPU, 10 000 IDs); this line's `value` is configs[1].  A
    # scaling curve must divide like by like: value(N) / (N * scale_ref.value).
    scale_ref = None
    if (rank == 0 and world == 1 and args.full and not args.no_extras and args.model is None and args.batch is None and args.gallery is None
            and args.input == "f32"):
        try:
            m4 = frmap_amd.get_model("arcface", 36)
            m4.load_state_dict(synth.calibrated_state_dict("arcface", synth.shapes_of(m4), 1004))
            m4 = m4.to(dev).eval().set_compute_dtype(dtype)
            g4 = frmap_amd.Gallery([f"id{i}" for i in range(10000)], synth.unit_rows(3004, 10000, 512), dev)
            gen4 = torch.Generator(device=dev)
            gen4.manual_seed(2004)
            x4 = torch.randn((1024, 3, 224, 224), device=dev, dtype=torch.float32, generator=gen4)
            rec4, _, _ = make_local_step(m4, x4, bool(args.graph), args.streams, gallery=g4, need_norm=False)
            ms4 = []
            t4 = timed_region(rec4, 30, args.warmup, args.steps, False, ms4)
            scale_ref = {"value": round(1024 * args.steps / t4, 1), "unit": "faces/s", "ms_per_step": round(t4 / args.steps * 1e3, 4),
                         "step_ms": step_stats(ms4),
                         "workload": "BASELINE.json configs[3] per-GPU shape on one GPU: ResNet18-ArcFace embed + top-1 match, 1024 faces, "
                                     "10 000-ID gallery, no collective",
                         "use": "denominator of the scaling curve: efficiency(N) = value(N) / (N * scale_ref.value)"}
            del m4, g4, x4, rec4
        except Exception as e:
            scale_ref = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.synchronize()

    # ---------------- CPU baseline: the oracle on the host cores (bounded sample) -----------------
    cpu_baseline = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        from oracle import face_oracle as fo
        # the GPU box exposes 256 logical CPUs but a 1-GPU job owns a 16-core share; more threads
        # than that only oversubscribe the quota (measured: 256 threads -> 3.8 faces/s)
        try:
            avail = len(os.sched_getaffinity(0))
        except AttributeError:
            avail = os.cpu_count() or 1
        cores = max(1, min(avail, int(os.environ.get("FRMAP_CPU_THREADS", "16"))))
        torch.set_num_threads(cores)
        nb = 64
        xc = x[:nb].cpu()
        if xc.dtype == torch.uint8:   # the reference's ToTensor + Normalize (`src/testing.py:99-104`) on the host
            mean, std = torch.tensor(model.input_mean).view(1, 3, 1, 1), torch.tensor(model.input_std).view(1, 3, 1, 1)
            xc = (xc.permute(0, 3, 1, 2).float() / 255.0 - mean) / std
        gal = gallery.matrix.cpu()
        emb_fn = {"cnn": fo.cnn_embedding, "arcface": fo.arcface_embedding, "baseline": fo.baseline_embedding,
                  "siamese": fo.siamese_forward_one, "hybrid": fo.hybrid_embedding,
                  "attention": fo.attention_embedding}[model_type]
        best = float("inf")
        with torch.no_grad():
            for rep in range(4):
                c0 = time.perf_counter()
                e = emb_fn(sd, xc)
                e = torch.nn.functional.normalize(e, dim=1) if need_norm else e
                fo.match_top1(e, gal)
                c1 = time.perf_counter()
                if rep > 0:
                    best = min(best, c1 - c0)
        cpu_baseline = {"value": round(nb / best, 1), "unit": "faces/s", "cores": cores, "kind": "port",
                        "sample": f"{nb} faces (same synthetic batch), fp32 torch-CPU oracle forward + L2-normalise + "
                                  f"{G}-ID match, best of 3 after 1 warm-up"}

    if rank == 0:
        names = {"cnn": "ResNet18 ('cnn')", "arcface": "ResNet18-ArcFace ('arcface')"}
        line = {
            "metric": "faces/sec (224x224 embed+match)", "value": round(faces_per_s, 1), "unit": "faces/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "settle_steps": max(args.settle_steps, 0),
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "step_ms": step_stats(per_step_ms),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{names.get(model_type, model_type)} embed + L2-normalise + top-1 match, batch {B}/GPU, "
                                   f"{G}-ID gallery, 224x224x3 " + ("fp32 NCHW" if args.input == "f32" else "uint8 HWC") + " inputs resident in HBM, seeded random-init weights "
                                   f"with calibrated BatchNorm statistics (BASELINE.json configs[{3 if model_type == 'arcface' and G >= 10000 else 1}])",
                       "global_batch": total,
                       "parallelism": f"dp{world} (faces sharded, 1 all-gather of 8 B/face" + (", overlapped with the next step" if overlap else "") + ")",
                       "backend": backend if world > 1 else None, "rccl_ranks": rccl_ranks,
                       "execution": (f"HIP graph replay, {args.streams} concurrent micro-batch streams" if is_graphed
                                     else f"eager launches, {args.streams} stream(s)" + graph_note)},
            "roofline": roofline, "cpu_baseline": cpu_baseline,
        }
        if scale_ref is not None:
            line["scale_ref"] = scale_ref
        if shard_check is not None:
            line["shard_check"] = shard_check
        if local_only is not None:
            line["local_only"] = local_only
        line.update(extras)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None) -> int:
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # launcher: spawn the ranks BEFORE anything in this process could touch the GPU (torch is not even imported)
        return launch_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv))
    return worker(args)


if __name__ == "__main__":
    sys.exit(main())
