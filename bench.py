#!/usr/bin/env python
"""bench.py -- benchmark of the SVGP / AnalyticSVI CAVI hot path on MI355X.

Metric (BASELINE.json): CAVI iterations/sec (+ time-to-ELBO-tolerance) for SVGP m = 1024 inducing points on N = 1e6
synthetic points.  Default workload = BASELINE.json configs[1] ("C2"): SqExponential kernel + Logistic likelihood,
AnalyticSVI(1024), m = 1024, N = 1e6, D = 32, fp64, hypers fixed (optimiser=false, as in every reference docs example).

One "step" = one update_parameters!(model::SVGP, ...) (src/training/training.jl:140-144) on one minibatch: kernel
matrix Knm, kappa = Knm K^-1, augmented Cholesky of -2*eta2 with [kappa; eta1'] (W = kappa L^-T), local updates,
natural-gradient step on (eta1, eta2).  Inputs are resident in HBM before the timed region.

--config c2 (default) | c3 | c4 | c5   one of BASELINE.json's configs (c3: Matern52 + StudentT, B = m = 2048, D = 64, fp32;
                                       c4: 8-class LogisticSoftMax, m = B = 1024; c5: multi-output 16 latents / 4 outputs,
                                       m = B = 4096, D = 64, N = 5e6 -- on one GPU the two latents a rank of the 8-GPU run owns)

N GPUs (launched by torch.distributed.run, one rank per GPU).  The collectives of the data path are issued by libagp_hip.so
itself (agp_comm_* -> RCCL over xGMI, include/agp_hip.h); torch.distributed only carries the 128-byte RCCL id and the timing
reduction.  What shards, per config:
  c2  batch-parallel WEAK scaling: global minibatch B = 1024 * N, every rank takes 1024 points, ONE all-reduce per step of the
      packed statistics [kappa'(rho g1) | lower tiles of rho kappa' diag(g2) kappa] (4.46 MB), then the replicated m^3 work.
      `value` counts a step over the global batch as N minibatch-iterations (1024-point minibatches per second, whole job).
  c3  same plan, B = 2048 * N.
  c4  latent-parallel STRONG scaling: the 8 latent GPs of the 8-class model spread over the ranks (one per GPU at N = 8), the
      B-vector sum_k gamma_k all-reduced twice per step; every --hyper-every steps (0 = never) the tied-Z hyper step with its
      all-reduce of the (1 + D + m D)-element gradient.
  c5  latent-parallel STRONG scaling: 16 latents over the ranks, one all-reduce of the (mean_f, var_f) exchange buffer per step.

Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times --steps steps and prints the line: the headline `value` (iter/s), `ms_per_step`, and what the
timed steps themselves measured (the dominant kernel's roofline from HIP events inside the timed region, collective accounting).
--full adds everything that takes runs of its own: the split-overlap A/B (N > 1), isolated launches, the MFMA issue-rate and
sustained-clock runs, the hyper-on iteration and streaming prediction (--no-extras: without them), time to ELBO tolerance
(--no-elbo-tol) and the CPU baseline (--no-cpu-baseline).  --dump-outputs DIR writes the posterior the timed steps left
(dump_outputs); the inputs depend on the arguments alone (fixed seeds), so two builds can be compared output for output.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP64_MFMA_PEAK_TFLOPS = 78.6   # AMD MI355X datasheet FP64 matrix (dense); not in the local guide, see DESIGN.md
FP32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md

CONFIGS = {
    #        kernel     likelihood          m     B     N          D   dtype  latents
    "c2": dict(kernel="sqexp", lik="logistic", m=1024, B=1024, N=1_000_000, D=32, f32=False, K=1,
               name="C2: SVGP SqExponential+Logistic AnalyticSVI({B}) m={m} N={N} D={D} fp64, hypers fixed"),
    "c3": dict(kernel="matern52", lik="studentt", m=2048, B=2048, N=1_000_000, D=64, f32=True, K=1,
               name="C3: SVGP Matern52+StudentT(3) AnalyticSVI({B}) m={m} N={N} D={D} fp32, hypers fixed"),
    "c4": dict(kernel="sqexp", lik="lsm", m=1024, B=1024, N=1_000_000, D=32, f32=False, K=8,
               name="C4: SVGP SqExponential+LogisticSoftMax(8 classes = 8 latent GPs) AnalyticSVI({B}) m={m} N={N} D={D} fp64"),
    "c5": dict(kernel="sqexp", lik="mo", m=4096, B=4096, N=5_000_000, D=64, f32=False, K=16,
               name="C5: multi-output SVGP 16 latents / 4 outputs (2 Gaussian + 2 Logistic) AnalyticSVI({B}) m={m} N={N} "
                    "D={D} fp64"),
}


NO_PREFETCH = os.environ.get("AGP_BENCH_NO_PREFETCH") == "1"  # diagnostic: every step computes its own kappa in-stream


def flush_c_stdio():
    try:
        C.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=30)
    p.add_argument("--config", "--mode", dest="config", default="c2", choices=sorted(CONFIGS))
    p.add_argument("--m", type=int, default=None)
    p.add_argument("--batch", type=int, default=None)
    p.add_argument("--N", type=int, default=None)
    p.add_argument("--D", type=int, default=None)
    p.add_argument("--hyper-every", type=int, default=0, help="c4, N > 1: tied-Z hyper step every k steps inside the timed region")
    p.add_argument("--c5-latents", type=int, default=2, help="c5 on one GPU: how many of the 16 latents this GPU owns")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-elbo-tol", action="store_true")
    p.add_argument("--no-extras", action="store_true")
    p.add_argument("--cpu-seconds", type=float, default=15.0)
    p.add_argument("--cpu-elbo-seconds", type=float, default=200.0,
                   help="budget for running the CPU oracle through the smoothed time-to-ELBO rule (0: only extrapolate)")
    p.add_argument("--collective", default="rccl", choices=["rccl", "torch"],
                   help="N > 1: who issues the all-reduces: libagp_hip.so through its own RCCL communicator (default) or a "
                        "callback into torch.distributed (diagnostic)")
    p.add_argument("--full", action="store_true",
                   help="everything beyond the headline figure: split-overlap A/B, isolated launches, MFMA issue-rate and sustained "
                        "clock runs, hyper-on iteration, streaming prediction, time to ELBO tolerance, CPU baseline (the --no-* "
                        "options switch parts of it off)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the variational posterior they left (mu, Sigma per latent; A of the "
                        "multi-output model) as DIR/<name>.npy")
    return p.parse_args()


DUMP_BYTES = 60 << 20  # data of all --dump-outputs files together: under 64 MB with room for the .npy headers


def dump_outputs(out_dir, model, n_written):
    """--dump-outputs: what a caller of the timed path reads from the model after its last step -- mu and Sigma of every latent
    this rank holds (global latent index in the name; the model's float type) and, for the multi-output model, the mixing weights
    A -- as <out_dir>/<name>.npy.  n_written: latents written by all ranks together.  A Sigma larger than its share of DUMP_BYTES
    is written as `Sigma_latent<k>_sample.npy`: a fixed, seeded sample of its entries (the same flat indices in every run)."""
    os.makedirs(out_dir, exist_ok=True)
    m, es = model.m, np.dtype(model.T).itemsize
    A = model.get_A() if hasattr(model, "get_A") else None
    fixed = n_written * m * es + (A.nbytes if A is not None else 0)
    per_sigma = max(1, (DUMP_BYTES - fixed) // (es * max(n_written, 1)))
    pick = None
    if m * m > per_sigma:
        pick = np.sort(np.random.default_rng(2024).choice(m * m, per_sigma, replace=False))
    for i in range(model.n_latent):
        k = model.latent_offset + i
        mu, Sig, _, _ = model.get_state(i)
        np.save(os.path.join(out_dir, f"mu_latent{k}.npy"), mu)
        if pick is None:
            np.save(os.path.join(out_dir, f"Sigma_latent{k}.npy"), Sig)
        else:
            np.save(os.path.join(out_dir, f"Sigma_latent{k}_sample.npy"), Sig.reshape(-1)[pick])
    if A is not None:
        np.save(os.path.join(out_dir, "A.npy"), A)


def rff_latent(X, D, g, dev, R=256):
    """latent f = sum_j w_j cos(omega_j'x + b_j) sqrt(2/256), omega ~ N(0, l^-2 I), l = sqrt(D)/4."""
    ell = math.sqrt(D) / 4.0
    om = torch.randn(D, R, dtype=torch.float64, device=dev, generator=g) / ell
    b = torch.rand(R, dtype=torch.float64, device=dev, generator=g) * (2 * math.pi)
    w = torch.randn(R, dtype=torch.float64, device=dev, generator=g)
    N = X.shape[0]
    f = torch.zeros(N, dtype=torch.float64, device=dev)
    for s in range(0, N, 131072):
        f[s:s + 131072] = torch.cos(X[s:s + 131072].to(torch.float64) @ om + b) @ w * math.sqrt(2.0 / R)
    return f


def make_data(cfg, seed, dev):
    """X ~ U[0,1]^{N x D} and the labels of the config.  Returns X (model dtype), y (numpy, as a caller of train!
    would pass it: one array, or a list of per-task arrays for the multi-output model), ell."""
    N, D = cfg["N"], cfg["D"]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    X = torch.rand(N, D, dtype=torch.float64, device=dev, generator=g)
    ell = math.sqrt(D) / 4.0
    lik = cfg["lik"]
    if lik == "logistic":
        f = rff_latent(X, D, g, dev)
        u = torch.rand(N, dtype=torch.float64, device=dev, generator=g).clamp_(1e-12, 1 - 1e-12)
        y = torch.sign(f + torch.log(u) - torch.log1p(-u))
        y[y == 0] = 1.0
        yh = y.cpu().numpy()
    elif lik == "studentt":
        f = rff_latent(X, D, g, dev)
        # t_3 noise = normal / sqrt(chi2_3 / 3)
        z = torch.randn(N, dtype=torch.float64, device=dev, generator=g)
        c = (torch.randn(3, N, dtype=torch.float64, device=dev, generator=g) ** 2).sum(0) / 3.0
        yh = (f + 0.1 * z / torch.sqrt(c)).cpu().numpy()
    elif lik == "lsm":
        fs = torch.stack([rff_latent(X, D, g, dev) for _ in range(cfg["K"])])
        yh = (1 + torch.argmax(fs, dim=0)).cpu().numpy()
    elif lik == "mo":
        Q = cfg["K"]
        A = torch.rand(4, Q, dtype=torch.float64, device=dev, generator=g) + 0.1
        A = A / A.norm(dim=1, keepdim=True)
        fs = torch.stack([rff_latent(X, D, g, dev) for _ in range(4)])  # 4 task functions (cheaper than 16 draws then mix)
        yh = [(fs[0] + 0.1 * torch.randn(N, dtype=torch.float64, device=dev, generator=g)).cpu().numpy(),
              (fs[1] + 0.1 * torch.randn(N, dtype=torch.float64, device=dev, generator=g)).cpu().numpy(),
              torch.sign(fs[2]).cpu().numpy(), torch.sign(fs[3]).cpu().numpy()]
        for t in (2, 3):
            yh[t][yh[t] == 0] = 1
        cfg["A"] = A.cpu().numpy()
    else:
        raise ValueError(lik)
    if cfg["f32"]:
        X = X.to(torch.float32)
    return X, yh, ell


def build_model(AGP, cfg, ell, Z, B_local, rank, world, dev_index, mode):
    """the model of this rank: all latents (single GPU, batch-parallel) or a latent slice (latent-parallel)"""
    from agp_amd import parallel as P

    kern = {"sqexp": AGP.SqExponentialKernel, "matern52": AGP.Matern52Kernel}[cfg["kernel"]]()
    k = AGP.with_lengthscale(kern, ell)
    T = np.float32 if cfg["f32"] else np.float64
    lik = cfg["lik"]
    kw = dict(optimiser=False, device=dev_index, T=T)
    if lik == "logistic":
        return AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(B_local), Z, **kw)
    if lik == "studentt":
        return AGP.SVGP(k, AGP.StudentTLikelihood(3.0), AGP.AnalyticSVI(B_local), Z, **kw)
    if lik == "lsm":
        sl = P.latent_slice(cfg["K"], world, rank) if mode == "latent" and world > 1 else None
        if cfg.get("hyper_every"):
            kw.update(optimiser=AGP.ADAM(0.01), Zoptimiser=AGP.ADAM(0.001))
            k = 1.0 * k  # a ScaledKernel: the tied step moves variance, scale and Z
        return AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(cfg["K"]), AGP.AnalyticSVI(B_local), Z, latent_slice=sl, **kw)
    if lik == "mo":
        Q = cfg["K"]
        if world > 1:
            sl = P.latent_slice(Q, world, rank)
        else:
            sl = (0, min(Q, cfg["c5_latents"])) if cfg["c5_latents"] < Q else None
        liks = [AGP.GaussianLikelihood(0.05), AGP.GaussianLikelihood(0.05), AGP.LogisticLikelihood(), AGP.LogisticLikelihood()]
        return AGP.MOSVGP(k, liks, AGP.AnalyticSVI(B_local), [Z] * Q, A=cfg["A"], Aoptimiser=AGP.ADAM(0.01), latent_slice=sl,
                          **kw)
    raise ValueError(lik)


def _pmc_traffic(cfg_name, kernel_name, step_inst):
    """traffic (bytes per launch) of `kernel_name` from profiles/r06_<cfg>_pmc_hbm_bytes.json (older rounds' files as fall-backs):
    -> {"traffic": .., "traffic_source": .., "traffic_kernel": ..} or {} when no file lists the kernel"""
    names = [f"r06_{cfg_name}_pmc_hbm_bytes.json", f"r05_{cfg_name}_pmc_hbm_bytes.json"]
    names += {"c2": ["r04_pmc_hbm_bytes.json", "r03_pmc_hbm_bytes.json"], "c3": ["r04_c3_pmc_hbm_bytes.json", "r03_c3_pmc_hbm_bytes.json"],
              "c5": ["r02_c5_pmc_hbm_bytes.json"]}.get(cfg_name, [])
    # rocprofv3 prints every template argument: match on the kernel's name and its leading arguments
    base = kernel_name.split(" (")[0].split(", ...")[0].rstrip(">")
    stem = base.split("<")[0]
    for pf in names:
        try:
            with open(os.path.join(ROOT, "profiles", pf)) as fh:
                pm = json.load(fh)
        except Exception:
            continue
        keys = [k for k in pm["kernels"] if k.startswith(base)] or ([k for k in pm["kernels"] if k.startswith(stem + "<")] if "blocked" not in base else [])
        if "blocked" in kernel_name:  # the blocked factorisation: its three kernels together, per step launch count unknown here: per kernel
            parts = {k: pm["kernels"][k]["hbm_bytes_per_launch_corrected"] for k in pm["kernels"]
                     if k.startswith(("k_chol_step<", "k_chol_panel<", "k_chol_trail<"))}
            if parts:
                # per launch of the SEQUENCE (what `achieved` is per): the kernels' bytes weighted by their launch counts in that run
                cnt = {k: pm["kernels"][k]["FETCH_SIZE"]["launches"] for k in parts}
                avg = sum(parts[k] * cnt[k] for k in parts) / max(sum(cnt.values()), 1)
                return {"traffic": int(avg), "traffic_per_kernel": parts, "traffic_launches_in_pass": cnt,
                        "traffic_source": f"profiles/{pf} (rocprofv3 --pmc, separate passes; average over the sequence's launches)"}
            continue
        if not keys:
            continue

        def _args(k):
            return k[k.index("<") + 1:k.rindex(">")].split(", ") if "<" in k else []

        if step_inst:  # the CAVI step's own instantiation (template argument STEP = true) when the file has it
            pref = [k for k in keys if len(_args(k)) >= 5 and _args(k)[4] == "true"]
            keys = pref or keys
        # the launch with the most traffic among the candidates is the step's (set-up launches of the same kernel are smaller)
        key = max(keys, key=lambda k: pm["kernels"][k]["hbm_bytes_per_launch_corrected"])
        return {"traffic": pm["kernels"][key]["hbm_bytes_per_launch_corrected"], "traffic_kernel": key,
                "traffic_source": f"profiles/{pf} (rocprofv3 --pmc, separate passes, same command)"}
    return {}


def _hyper_products(m, B):
    """The seven GEMM-shaped launches of one hyper-on iteration: executed vs dense-count flops."""
    rows = [
        ("kappa = Knm K^-1", 2.0 * B * m * m, 2.0 * B * m * m),
        ("W = kappa Xa' (Xa lower triangular: k range of a column tile stops at its last column)", 1.0 * B * m * m * (1 + 64.0 / m),
         2.0 * B * m * m),
        ("Sigma = Xa' Xa (lower tiles, triangular k ranges, balanced units: k_xtx_bal)", m ** 3 / 3.0, 2.0 * m ** 3),
        ("K^-1 Sigma", 2.0 * m ** 3, 2.0 * m ** 3),
        ("kappa (Sigma K^-1)  [H = G_kappa K^-1 from one product]", 2.0 * B * m * m, 2.0 * B * m * m),
        ("C (Sigma K^-1)  [G_K from one product; C = kappa' diag(w) kappa + K^-1/4 comes from the factorisation launch's prologue]",
         2.0 * m ** 3, 2.0 * m ** 3),
        ("K^-1 = X' X after the K_ZZ refresh (k_xtx_bal)", m ** 3 / 3.0, 2.0 * m ** 3),
    ]
    return {"launches": len(rows), "executed_gflop": round(sum(r[1] for r in rows) / 1e9, 3),
            "dense_count_gflop": round(sum(r[2] for r in rows) / 1e9, 3),
            "round3": "nine 2 n^3-shaped launches + the half-flop Apred product (kappa Sigma, (.) K^-1, kappa' H, K^-1 Sigma, Apred "
                      "in addition to kappa, W, Sigma, K^-1)",
            "list": [r[0] for r in rows]}


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher around it (the shape of the driver's N = 1 command): start the N ranks
    ourselves, one process per GPU of this node, with the environment torch.distributed.run would give them (RANK, LOCAL_RANK,
    WORLD_SIZE, MASTER_ADDR = 127.0.0.1, a free MASTER_PORT).  Rank 0's stdout (the ONE JSON line) is ours, the other ranks'
    stdout and every rank's stderr go to our stderr.  Returns the first non-zero exit code (the other ranks are then stopped)."""
    import socket
    import subprocess

    if os.environ.get("AGP_BENCH_SHARE_GPU") != "1":
        have = torch.cuda.device_count()
        if have < n:
            print(f"[bench] --gpus {n} but this node shows {have} GPU(s)", file=sys.stderr)
            return 2
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] starting {n} ranks (MASTER_ADDR=127.0.0.1 MASTER_PORT={port}):", " ".join(cmd), file=sys.stderr, flush=True)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
        env.setdefault("OMP_NUM_THREADS", "1")             # (what torch.distributed.run sets for more than one rank)
        procs.append(subprocess.Popen(cmd, env=env, stdout=None if r == 0 else sys.stderr))
    rc = 0
    alive = set(range(n))
    while alive:
        for r in sorted(alive):
            st = procs[r].poll()
            if st is None:
                continue
            alive.discard(r)
            if st != 0 and rc == 0:
                rc = st
                print(f"[bench] rank {r} exited with code {st}; stopping the other ranks", file=sys.stderr, flush=True)
                for q in alive:
                    procs[q].terminate()
        time.sleep(0.05)
    return rc


def main():
    # c5 on one GPU times the share of ONE rank of the 8-GPU run (a latent slice without its communicator): the library refuses
    # that by default (the mixes are partial), the benchmark asks for it explicitly
    os.environ.setdefault("AGP_ALLOW_PARTIAL_SHARD", "1")
    a = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU) and hand over to them
        raise SystemExit(launch_ranks(a.gpus))
    # Nothing but the ONE JSON line on stdout: gloo ("[Gloo] Rank 0 is connected ..."), RCCL's banner and anything else a library
    # prints through C stdio or fd 1 goes to stderr for the whole run -- fd 1 is pointed at fd 2 here and the saved descriptor is
    # used for the line alone (round 6)
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    if world != a.gpus:
        raise SystemExit(f"[bench] --gpus {a.gpus} but WORLD_SIZE={world}: launch as `python bench.py --gpus N ...` (starts its own "
                         "ranks) or `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 "
                         "--master-port P bench.py --gpus N ...` (script options spelled out in full: the launcher's argument "
                         "parser claims abbreviations such as --m)")
    # test hook: AGP_BENCH_SHARE_GPU=1 maps every rank to GPU 0 and uses gloo + the callback transport, so the N > 1 code path
    # can be exercised on a single-GPU box (never set by the driver; numbers from such a run are meaningless)
    share = os.environ.get("AGP_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_

        dist = dist_
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    import __graft_entry__ as ge

    if rank == 0:
        ge.build()
    if dist is not None:
        dist.barrier()
    import agp_amd as AGP
    from agp_amd import capi
    from agp_amd import parallel as P

    L = capi.lib()
    cfg = dict(CONFIGS[a.config])
    for key, val in (("m", a.m), ("B", a.batch), ("N", a.N), ("D", a.D)):
        if val is not None:
            cfg[key] = val
    cfg["c5_latents"] = a.c5_latents
    cfg["hyper_every"] = a.hyper_every if (a.config == "c4") else 0
    N, D, m, B = cfg["N"], cfg["D"], cfg["m"], cfg["B"]
    steps, warm = a.steps, a.warmup
    # how this config shards
    mode = "batch" if cfg["lik"] in ("logistic", "studentt") else "latent"
    B_global = B * world if mode == "batch" else B
    X, yh, ell = make_data(cfg, 1234, dev)
    rng = np.random.default_rng(4321)  # identical on every rank: Z and the index stream are shared
    Z = X[torch.as_tensor(rng.permutation(N)[:m], device=dev)].cpu().numpy().astype(np.float64)
    total = steps + warm
    idx_np = np.stack([rng.choice(N, B_global, replace=False) for _ in range(total)]).astype(np.int64)
    if mode == "batch" and world > 1:
        idx_all = torch.as_tensor(idx_np[:, rank * B:(rank + 1) * B].copy(), device=dev)  # this rank's share of every minibatch
    else:
        idx_all = torch.as_tensor(idx_np, device=dev)
    rho = N / B_global

    model = build_model(AGP, cfg, ell, Z, B, rank, world, local_rank, mode)
    model.inference.rho = rho
    eng = P.HipEngine(model, B).bind_data(X, yh)
    h = eng.h
    xp, yp, ld = C.c_void_p(eng._X.data_ptr()), C.c_void_p(eng._y.data_ptr()), eng._X.stride(0)
    comm, coll = None, "none"
    if world > 1:
        if a.collective == "rccl" and not share:
            try:
                comm = P.Comm.rccl_from_torch(model)
                coll = "rccl via agp_comm (libagp_hip.so)"
            except Exception as e:  # librccl not loadable by the library: keep the run alive and say so in the JSON line
                if rank == 0:
                    print(f"[bench] agp_comm_init failed ({e}); falling back to the torch.distributed callback", file=sys.stderr)
        if comm is None:
            comm = P.Comm.from_group(model)
            coll = "torch.distributed callback (" + dist.get_backend() + ")"
        if mode == "batch":
            eng.set_batch_shard(rank, world)
        comm.timing(0 if os.environ.get("AGP_BENCH_NO_TIMING") == "1" else 4)  # every 4th collective: two event records cost the stream ~20 us
    elif os.environ.get("AGP_FORCE_SPLIT") == "1" and mode == "batch":
        # diagnostic: the N > 1 step sequence (packed statistics -> all-reduce -> eta step) with a one-rank RCCL communicator
        fake_us = float(os.environ.get("AGP_BENCH_FAKE_ALLREDUCE_US", "0"))
        if fake_us > 0:
            # stand-in for the xGMI all-reduce on a one-GPU box: a kernel that just occupies the stream for about that long
            # (torch.cuda._sleep: ~0.59 ns per count on MI355X; the JSON line carries the measured us per call.)  A call on PART of
            # the statistics (AGP_SPLIT_OVERLAP's column groups) is charged its share of the bytes, but never less than a latency
            # floor (AGP_BENCH_FAKE_ALLREDUCE_LAT_US, default 15: a small xGMI all-reduce is latency-bound)
            lat_us = float(os.environ.get("AGP_BENCH_FAKE_ALLREDUCE_LAT_US", "15"))
            mp_ = (m + 63) // 64 * 64
            full_count = mp_ + (mp_ // 64) * (mp_ // 64 + 1) // 2 * 4096
            exts = {}
            # AGP_BENCH_FAKE_RESIDENT=<workgroups>x<threads> (e.g. 16x512): instead of a sleep kernel, a stand-in that occupies the
            # chip the way RCCL's ring kernel does -- that many workgroups which must ALL be resident to finish (grid barrier, the
            # range moved through their registers, grid barrier; agp_comm_standin_allreduce), lasting at least the same time
            resident = os.environ.get("AGP_BENCH_FAKE_RESIDENT", "")
            res_wg, res_thr = (int(v) for v in resident.split("x")) if resident else (0, 0)
            stuck = torch.zeros(1, dtype=torch.int32, device=dev) if resident else None
            cfg["_standin_stuck"] = stuck

            def _fake(ptr, count, dtype, stream):
                try:
                    us = fake_us if count >= full_count else max(lat_us, fake_us * count / full_count)
                    if resident:
                        st_ = L.agp_comm_standin_allreduce(C.c_void_p(ptr), count, dtype,
                                                           C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream),
                                                           res_wg, res_thr, float(us), C.c_void_p(stuck.data_ptr()))
                        if st_ != 0:
                            raise RuntimeError(f"agp_comm_standin_allreduce -> {st_}")
                        return
                    cyc = int(us * 1700)
                    if stream is None:  # the ctx runs on the default stream, which is torch's current one here
                        torch.cuda._sleep(cyc)
                    else:
                        if stream not in exts:
                            exts[stream] = torch.cuda.ExternalStream(int(stream))
                        with torch.cuda.stream(exts[stream]):
                            torch.cuda._sleep(cyc)
                except BaseException as e:
                    print("[bench] fake all-reduce failed:", repr(e), file=sys.stderr)
                    raise

            comm = P.Comm.from_callback(model, 0, 1, _fake)
            coll = (f"callback: resident stand-in, {res_wg} workgroups x {res_thr} threads, >= {fake_us:.0f} us per whole statistic "
                    "(AGP_BENCH_FAKE_RESIDENT)" if resident else
                    f"callback: ~{fake_us:.0f} us sleep kernel per call (AGP_BENCH_FAKE_ALLREDUCE_US)")
        else:
            comm = P.Comm.rccl(model, 0, 1, P.Comm.unique_id())
            coll = "rccl via agp_comm (one rank, AGP_FORCE_SPLIT)"
        comm.timing(0 if os.environ.get("AGP_BENCH_NO_TIMING") == "1" else 4)  # every 4th collective: two event records cost the stream ~20 us
    flush_c_stdio()  # RCCL's init banner, if any, goes out now
    smode = capi.SHARD_BATCH if mode == "batch" else capi.SHARD_LATENT
    tied = cfg["hyper_every"] > 0
    # a latent slice of the multi-output model goes through the sharded step even on one GPU (its exchange buffer is mixed there)
    use_multi = comm is not None or bool(getattr(model, "sharded", False))

    # The look-ahead (kappa of the next minibatch on the library's second stream) is used in every mode.  In the phase-split
    # batch-parallel step the kappa buffers are released right after the packed statistics, so the look-ahead runs next to the
    # all-reduce.  Measured on one GPU with a stand-in kernel of 27 / 43 / 65 us in the all-reduce's place (AGP_FORCE_SPLIT=1
    # AGP_BENCH_FAKE_ALLREDUCE_US=..): 0.422 / 0.4225 / 0.438 ms per step with the look-ahead, 0.455 / 0.469 / 0.488 without.
    # (With NO kernel between the statistics and the eta step -- a one-rank communicator, whose collective is skipped -- the two
    # streams' event hand-overs collide and the look-ahead costs 0.15 ms; that case does not occur with more than one rank.)
    use_prefetch = not NO_PREFETCH

    def step(i):
        if not use_multi:
            st = L.agp_svgp_cavi_step(h, xp, ld, yp, C.c_void_p(idx_all[i].data_ptr()), B, rho)
        else:
            st = L.agp_svgp_cavi_step_multi(h, comm.h if comm is not None else None, smode, xp, ld, yp,
                                            C.c_void_p(idx_all[i].data_ptr()), B, rho)
        if st != 0:
            capi.check(model._ctx, st)
        if tied and (i + 1) % cfg["hyper_every"] == 0:
            st = L.agp_svgp_hyper_step_multi(h, comm.h if comm is not None else None, 1)
            if st != 0:
                capi.check(model._ctx, st)
        elif i + 1 < total and use_prefetch:  # look-ahead: kappa of the next minibatch on the library's second stream
            L.agp_svgp_prefetch(h, xp, ld, C.c_void_p(idx_all[i + 1].data_ptr()), B)

    for i in range(warm):
        step(i)
    model._chk(L.agp_svgp_check_status(h))  # (also takes the natural-gradient step the last warm-up iteration left pending)
    fb0 = C.c_int64(0)
    model._chk(L.agp_ctx_task_graph_fallbacks(model._ctx, C.byref(fb0)))
    cnt0 = (C.c_int64(), C.c_int64())
    model._chk(L.agp_svgp_step_counters(h, C.byref(cnt0[0]), C.byref(cnt0[1])))
    # HIP events around the dominant kernel sequence of every 4th step (every step at c5): bracketing every step costs the C2
    # step 16 us (0.375 -> 0.391 ms), every 4th 4 us
    t_every = 1 if a.config == "c5" or steps < 12 else 4
    model._chk(L.agp_svgp_timing_enable(h, 0 if os.environ.get("AGP_BENCH_NO_TIMING") == "1" else t_every))
    if comm is not None:
        comm.stats()  # reset the accounting
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, total):
        step(i)
    t_enq = time.perf_counter()  # host side done enqueueing (diagnostic: a host-bound loop shows up as t_enq ~ t1)
    # the natural-gradient step of a single-latent CAVI step rides on the NEXT step's factorisation launch (include/agp_hip.h):
    # the last timed step's is still pending here.  check_status takes it (stand-alone kernel) and synchronises, INSIDE the timed
    # region -- all `steps` natural-gradient steps are paid for between t0 and t1, none is left outside
    model._chk(L.agp_svgp_check_status(h))
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t1 = time.perf_counter()
    dt = t1 - t0
    host_enqueue_ms_per_step = (t_enq - t0) * 1e3 / max(steps, 1)
    # task-graph launches of the timed region that lost a tile dependency and were re-run by the in-stream fallback (0 on a GPU the
    # process has to itself; a non-zero count = steps that took milliseconds, include/agp_hip.h agp_ctx_task_graph_fallbacks)
    fb1 = C.c_int64(0)
    model._chk(L.agp_ctx_task_graph_fallbacks(model._ctx, C.byref(fb1)))
    task_graph_fallbacks = int(fb1.value - fb0.value)
    if dist is not None:
        tfb = torch.tensor([task_graph_fallbacks], dtype=torch.int64, device="cpu" if share else dev)
        dist.all_reduce(tfb, op=dist.ReduceOp.SUM)
        task_graph_fallbacks = int(tfb.item())
    nl, kms = C.c_int64(), C.c_double()
    model._chk(L.agp_svgp_timing_read(h, C.byref(nl), C.byref(kms)))
    model._chk(L.agp_svgp_timing_enable(h, 0))
    cnt1 = (C.c_int64(), C.c_int64())
    model._chk(L.agp_svgp_step_counters(h, C.byref(cnt1[0]), C.byref(cnt1[1])))
    n_pro = cnt1[1].value - cnt0[1].value  # timed steps whose natural-gradient part was the prologue of the next launch
    coll_stats = comm.stats() if comm is not None else (0, 0, 0.0)
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if share else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # the state the timed steps left, before any section below steps the model again (batch-parallel ranks hold the same state:
    # rank 0 writes it; latent-parallel ranks write the latents they own)
    if a.dump_outputs and (rank == 0 or mode == "latent"):
        dump_outputs(a.dump_outputs, model, model.n_latent_total if mode == "latent" and world > 1 else model.n_latent)

    # ---- A/B of the batch-parallel step's collective (outside the timed region above): the same loop once more with
    # AGP_SPLIT_OVERLAP flipped -- the statistics travelling in block-column groups on the communicator's own stream, the next
    # task-graph launch starting on the first group.  The library reads the variable at every step.
    overlap_ab = None
    if a.full and comm is not None and mode == "batch" and os.environ.get("AGP_BENCH_NO_OVERLAP_AB") != "1":
        keep = os.environ.get("AGP_SPLIT_OVERLAP")
        flipped = "0" if keep == "1" else "1"
        os.environ["AGP_SPLIT_OVERLAP"] = flipped
        try:
            for i in range(warm):
                step(i)
            model._chk(L.agp_svgp_check_status(h))
            comm.stats()
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()
            ta = time.perf_counter()
            for i in range(warm, total):
                step(i)
            model._chk(L.agp_svgp_check_status(h))
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            dt_ab = time.perf_counter() - ta
            nc_ab, nb_ab, ms_ab = comm.stats()
            if dist is not None:
                t = torch.tensor([dt_ab], dtype=torch.float64, device="cpu" if share else dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt_ab = float(t.item())
            overlap_ab = {"AGP_SPLIT_OVERLAP": int(flipped), "ms_per_step": round(dt_ab * 1e3 / max(steps, 1), 4),
                          "collective_us_per_call": round(ms_ab * 1e3 / max(nc_ab, 1), 2),
                          "bytes_allreduced_per_step_per_rank": int(nb_ab / max(steps, 1)),
                          "note": "same loop, same index stream, variable flipped; the headline line above ran with AGP_SPLIT_OVERLAP="
                                  + (keep or "0") + "; with the flag on, one call is the train of column groups on the communicator's stream"}
        except Exception as ex:  # the A/B must never cost the headline line (it runs behind the timed region, last GPU work of N > 1)
            overlap_ab = {"AGP_SPLIT_OVERLAP": int(flipped), "error": repr(ex)[:300]}
            print("[bench] split-overlap A/B failed on rank", rank, ":", repr(ex), file=sys.stderr)
        finally:
            if keep is None:
                os.environ.pop("AGP_SPLIT_OVERLAP", None)
            else:
                os.environ["AGP_SPLIT_OVERLAP"] = keep

    # ---- roofline of the dominant kernel: the augmented Cholesky factorisation of -2*eta2 with the [kappa; eta1'] extension
    # rows: ONE launch of the tile task graph k_chol_dag per factorisation up to m = 2048 (several latents of one GPU share
    # interleaved launches), m / 64 launches of k_chol_step beyond ----
    f32 = cfg["f32"]
    peak = FP32_MFMA_PEAK_TFLOPS if f32 else FP64_MFMA_PEAK_TFLOPS
    tname = "float" if f32 else "double"
    mp = (m + 63) // 64 * 64
    Bq = (B + 63) // 64 * 64
    n_lat_local = model.n_latent
    # algorithmic flops of one augmented factorisation: potrf m^3/3 + panel solves of the (B + 64) extension rows m^2 each
    flops_fact = mp ** 3 / 3.0 + (Bq + 64) * mp ** 2
    # with the prologue the same launch also takes the natural-gradient step of the minibatch before (kappa' diag(w) kappa + the
    # eta steps, analyticVI.jl:143-180): credited 2 B m^2 like SURVEY 8d's F_iter credits it (B m^2 executed: one triangle)
    prologue = n_pro >= steps - 1 and steps > 1
    # batch-parallel over a communicator: the prologue only takes the eta step from the all-reduced statistics -- the product is the
    # packed launch in front of the collective, not part of this launch
    pro_product = prologue and comm is None
    flops_pro_credit, flops_pro_exec = 2.0 * Bq * mp ** 2, 1.0 * Bq * mp ** 2
    flops_fact_exec = flops_fact
    if pro_product:
        flops_fact_exec = flops_fact + flops_pro_exec
        flops_fact += flops_pro_credit
    launches_per_step = nl.value / max(-(-steps // t_every), 1)  # launches of the bracketed sequences / number of them
    avg_launch_s = (kms.value * 1e-3) / max(nl.value, 1)
    flops_per_launch = flops_fact * n_lat_local / max(launches_per_step, 1e-9)
    achieved = flops_per_launch / avg_launch_s / 1e12 if nl.value else 0.0
    dag = launches_per_step <= n_lat_local + 0.5
    per_fact = launches_per_step / max(1, -(-n_lat_local // 16))  # latents share launches in chunks of up to 16
    blocked = (not dag) and abs(per_fact - mp // 64) > 0.5
    kernel_name = (f"k_chol_dag<{tname}, true, false, false, true, true>" if dag and prologue else
                   f"k_chol_dag<{tname}, true, {'true' if n_lat_local > 1 else 'false'}>" if dag else
                   f"blocked factorisation: k_chol_step + k_chol_panel + k_chol_trail <{tname}>" if blocked else
                   f"k_chol_step<{tname}>")
    # beyond the task graph the live number above is taken while the next minibatch's kappa GEMM runs on the prefetch stream
    # (the two share the CUs): a few extra steps without the prefetch give the factorisation on its own
    isolated = None
    if a.full and not dag and comm is None:
        model._chk(L.agp_svgp_timing_enable(h, 1))
        for j in range(3):
            if use_multi:
                st = L.agp_svgp_cavi_step_multi(h, None, smode, xp, ld, yp, C.c_void_p(idx_all[j % total].data_ptr()), B, rho)
            else:
                st = L.agp_svgp_cavi_step(h, xp, ld, yp, C.c_void_p(idx_all[j % total].data_ptr()), B, rho)
            if st != 0:
                capi.check(model._ctx, st)
        nl2, kms2 = C.c_int64(), C.c_double()
        model._chk(L.agp_svgp_timing_read(h, C.byref(nl2), C.byref(kms2)))
        model._chk(L.agp_svgp_timing_enable(h, 0))
        if nl2.value:
            a2 = kms2.value * 1e-3 / nl2.value
            isolated = {"avg_launch_us": round(a2 * 1e6, 2), "achieved": round(flops_per_launch / a2 / 1e12, 3),
                        "frac": round(flops_per_launch / a2 / 1e12 / peak, 4),
                        "note": "same sequence with the prefetch stream idle (3 extra steps after the timed region)"}
    roofline = {
        "kernel": kernel_name,
        "bound": "mfma",
        "achieved": round(achieved, 3),
        "peak": peak,
        "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4),
        "traffic": None,
        "traffic_unit": "bytes/launch",
        "avg_launch_us": round(avg_launch_s * 1e6, 2),
        "launches_per_step": round(launches_per_step, 2),
        "timed_steps": f"every {t_every}th step of the timed region ({-(-steps // t_every)} of {steps})" if t_every > 1 else "every step",
        "algorithmic_flops_per_launch": flops_per_launch,
    }
    if prologue and not pro_product:
        roofline["contents"] = ("one launch = the augmented Cholesky of -2 eta2 with the [kappa; eta1'] extension rows (m^3/3 + (B+64) m^2), "
                                "the eta step from the all-reduced statistics of the minibatch before as its prologue and the row "
                                "statistics as its epilogue; the product kappa' diag(w) kappa is the packed launch in front of the "
                                "all-reduce")
    elif prologue:
        roofline["contents"] = ("one launch = the augmented Cholesky of -2 eta2 with the [kappa; eta1'] extension rows (m^3/3 + (B+64) m^2) "
                                "AND, as its prologue, the natural-gradient step of the minibatch before (kappa' diag(w) kappa, credited "
                                "2 B m^2 as in SURVEY 8d; B m^2 executed) -- until round 2 a kernel of its own between two factorisations")
        roofline["executed_frac"] = round(flops_fact_exec * n_lat_local / max(launches_per_step, 1e-9) / avg_launch_s / 1e12 / peak, 4)
        roofline["factorisation_only_frac"] = round((mp ** 3 / 3.0 + (Bq + 64) * mp ** 2) / avg_launch_s / 1e12 / peak, 4)
    # round 4: from 600 tiles per launch the task graph runs as TWO kernels (k_chol_dag<..., ROLE 1> = the chain workgroup(s) on a
    # stream of their own, <..., ROLE 2> = every other tile on the step's stream) -- the HIP events bracket the tile
    # kernel and the join with the chain kernel, i.e. the whole factorisation, as before
    ne_t, nt_t = Bq // 64 + 1, mp // 64
    tiles_per_launch = (nt_t * (nt_t + 1) // 2 + ne_t * nt_t) * (min(n_lat_local, 8) if n_lat_local > 1 else 1)
    if dag and not prologue and tiles_per_launch >= 600 and os.environ.get("AGP_CHAIN_SPLIT", "") != "0":
        roofline["kernel"] = kernel_name[:-1] + ", ..., ROLE 1 + ROLE 2> (chain kernel + tile kernel)"
        roofline["split_launch"] = {"tiles_per_launch": tiles_per_launch,
                                    "note": "chain workgroup(s) as a kernel of their own so that the tile kernel compiles to <= 100 "
                                            "(f64) / 71 (f32) VGPRs and runs 2-3 workgroups per CU (DESIGN.md 5b)"}
    if isolated:
        roofline["isolated"] = isolated
    # whole-iteration algorithmic rate (F_iter = 6 B m^2 + m^3 + B m (3D + 12) per latent)
    f_iter = (6.0 * B * m * m + m ** 3 + B * m * (3 * D + 12)) * n_lat_local
    # executed flops (the step does less than the credited count: the kappa Sigma GEMM is replaced by the panel solves and the
    # symmetric product computes one triangle): kappa GEMM 2Bm^2 + factorisation m^3/3 + panel solves (B+64)m^2 + half SYRK Bm^2
    f_exec = (2.0 * B * m * m + m ** 3 / 3.0 + (B + 64) * m * m + B * m * m + B * m * (3 * D + 12)) * n_lat_local
    if mode == "batch":
        unit_per_step = world          # a step over the global batch = `world` 1024-point minibatch-iterations
        scaling, par = "weak", (f"batch-parallel x{world}: B = {B} x {world}, one all-reduce of the packed statistics per step"
                                if world > 1 else "single GPU")
    else:
        unit_per_step = 1              # the whole model takes one step
        scaling = "strong"
        par = (f"latent-parallel x{world}: {cfg['K']} latent GPs over {world} GPUs ({n_lat_local} on rank 0)"
               if world > 1 else (f"single GPU, {n_lat_local} of {cfg['K']} latents" if n_lat_local < cfg["K"]
                                  else f"single GPU, all {cfg['K']} latents" if cfg["K"] > 1 else "single GPU"))
        if world == 1:
            scaling = "weak"
    out = {
        "metric": "cavi_iters_per_sec",
        "value": round(unit_per_step * steps / dt, 2),
        "unit": "iter/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": warm,
        "ms_per_step": round(dt / steps * 1e3, 4),
        "host_enqueue_ms_per_step": round(host_enqueue_ms_per_step, 4),
        "task_graph_fallbacks": task_graph_fallbacks,
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,
        "dtype": "f32" if f32 else "f64",
        "data": "synthetic",
        "config": {
            "workload": cfg["name"].format(B=B, m=m, N=N, D=D),
            "parallelism": par,
            "global_batch": B_global,
        },
        "iter_algorithmic_tflops": round(f_iter * steps / dt / 1e12, 3),
        "iter_frac_mfma_peak": round(f_iter * steps / dt / 1e12 / peak, 4),
        "iter_executed_tflops": round(f_exec * steps / dt / 1e12, 3),
        "iter_executed_frac_mfma_peak": round(f_exec * steps / dt / 1e12 / peak, 4),
        "roofline": roofline,
    }
    if comm is not None:
        ncalls, nbytes, cms = coll_stats
        out["value_definition"] = ("batch-parallel weak scaling: one step consumes the global minibatch of B x n_gpus points and counts "
                                   "as n_gpus minibatch-iterations; global steps/s = value / n_gpus" if mode == "batch" else
                                   "latent-parallel: one step of the whole model (all latents) counts as one iteration")
        # how many ranks the communicator of the data path really spans: every rank contributes 1.0 to a one-element all-reduce
        # issued through that very communicator (agp_comm_allreduce), outside the timed region
        one = torch.ones(1, dtype=torch.float64, device=dev)
        comm.all_reduce(one)
        torch.cuda.synchronize()
        out["collective"] = {
            "issuer": coll,
            "issued_by": coll,
            "ranks_seen": int(round(float(one.item()))),
            "calls_per_step": round(ncalls / max(steps, 1), 2),
            "bytes_per_step": int(nbytes / max(steps, 1)),
            "bytes_allreduced_per_step_per_rank": int(nbytes / max(steps, 1)),
            "us_per_step": round(cms * 1e3 / max(steps, 1), 2),
            "us_per_call": round(cms * 1e3 / max(ncalls, 1), 2),
            "timing": "HIP events on the ctx stream around every 4th collective (rank 0), scaled to all of them",
        }
        if cfg.get("_standin_stuck") is not None:
            out["collective"]["standin_workgroups_that_gave_up_waiting"] = int(cfg["_standin_stuck"].item())
        if tied:
            out["collective"]["tied_Z_hyper_step_every"] = cfg["hyper_every"]
        if overlap_ab is not None:
            out["collective"]["split_overlap_ab"] = overlap_ab

    # HBM bytes per launch of the dominant kernel from the committed PMC passes (profiles/, FETCH_SIZE x2 + WRITE_SIZE as
    # MI355X_MICROARCH.md prescribes for gfx950); rocprofv3 cannot wrap bench.py from inside, so this is not live.  Counter
    # collection serialises kernels, so those passes run the MERGED task graph (the context's self-test keeps it): where the live
    # launch is the split one (chain kernel + tile kernel) the traffic is that of the merged instantiation of the same task graph.
    if world == 1 and comm is None:
        roofline.update(_pmc_traffic(a.config, roofline["kernel"], step_inst=True))
    if a.full and rank == 0 and world == 1:
        # measured MFMA ceiling (issue-rate microbenchmark inside the library)
        pk = C.c_double()
        if L.agp_mfma_peak(model._ctx, capi.F32 if f32 else capi.F64, C.byref(pk)) == 0:
            # (a sustained issue-rate figure under the chip's power limit, NOT a ceiling: the production GEMMs reach 1.03-1.05 of it
            #  in short launches; every fraction in this line is against the datasheet peak)
            out["roofline"]["mfma_issue_ubench_tflops"] = round(pk.value, 1)

    single_latent = cfg["lik"] in ("logistic", "studentt")
    # ---- extras (rank 0, single GPU, single-latent configs): hyper-parameter step and streaming prediction ----
    if a.full and rank == 0 and world == 1 and single_latent and not a.no_extras:
        cfg_h = dict(cfg)
        kern = {"sqexp": AGP.SqExponentialKernel, "matern52": AGP.Matern52Kernel}[cfg["kernel"]]()
        lik_h = AGP.LogisticLikelihood() if cfg["lik"] == "logistic" else AGP.StudentTLikelihood(3.0)
        mh = AGP.SVGP(1.0 * AGP.with_lengthscale(kern, ell), lik_h, AGP.AnalyticSVI(B), Z, optimiser=AGP.ADAM(0.01),
                      Zoptimiser=AGP.ADAM(0.001), device=local_rank, T=np.float32 if f32 else np.float64)
        mh.inference.rho = rho
        hh = mh._ensure_handle(B)
        mh._chk(L.agp_svgp_refresh_K(hh))
        for i in range(3):
            mh._chk(L.agp_svgp_cavi_step(hh, xp, ld, yp, C.c_void_p(idx_all[i % total].data_ptr()), B, rho))
            mh._chk(L.agp_svgp_hyper_step(hh))
        torch.cuda.synchronize()
        th = time.perf_counter()
        nh = 20
        for i in range(nh):
            mh._chk(L.agp_svgp_cavi_step(hh, xp, ld, yp, C.c_void_p(idx_all[(3 + i) % total].data_ptr()), B, rho))
            mh._chk(L.agp_svgp_hyper_step(hh))
        torch.cuda.synchronize()
        out["ms_per_step_with_hyper_update"] = round((time.perf_counter() - th) / nh * 1e3, 4)
        # the reference's default training mode (SVGP(...; optimiser=ADAM(0.01)), SVGP.jl:39): its dominant kernel is the task-graph
        # factorisation WITH the inverse (twice per iteration: the updated -2 eta2 for Sigma / mu -- with the pending natural-gradient
        # step as its prologue --, and K_ZZ); a few more iterations with HIP events around the first of the two
        mh._chk(L.agp_svgp_timing_enable(hh, 1))
        for i in range(6):
            mh._chk(L.agp_svgp_cavi_step(hh, xp, ld, yp, C.c_void_p(idx_all[(3 + nh + i) % total].data_ptr()), B, rho))
            mh._chk(L.agp_svgp_hyper_step(hh))
        nlh, kmsh = C.c_int64(), C.c_double()
        mh._chk(L.agp_svgp_timing_read(hh, C.byref(nlh), C.byref(kmsh)))
        mh._chk(L.agp_svgp_timing_enable(hh, 0))
        if nlh.value:
            mpad = (m + 63) // 64 * 64
            us = kmsh.value * 1e3 / nlh.value
            pro_h = mpad // 64 <= 16  # the pending natural-gradient step rides on this launch up to 16 block columns (pro_allowed)
            fl = 2.0 * mpad ** 3 / 3.0 + 64 * mpad ** 2  # potrf + inverse (identity block rows) + the eta1 row
            if pro_h:
                fl += 2.0 * ((B + 63) // 64 * 64) * mpad ** 2  # + the product kappa' diag(w) kappa, credited as in SURVEY 8d
            out["hyper_roofline"] = {
                "kernel": f"k_chol_dag<{'float' if f32 else 'double'}, true, false, false, false, {'true' if pro_h else 'false'}>",
                "what": "factorisation of the updated -2 eta2 with L^-1 (identity block rows)"
                        + (" and the natural-gradient step as prologue" if pro_h else "")
                        + "; the iteration runs a second task graph of the same shape (without prologue) for K_ZZ",
                "bound": "mfma", "avg_launch_us": round(us, 2), "launches_per_iteration": 2,
                "algorithmic_flops_per_launch": fl, "achieved": round(fl / us / 1e6, 3), "peak": peak, "unit": "TFLOP/s",
                "frac": round(fl / us / 1e6 / peak, 4),
                "iteration": "no host synchronisation inside the iteration"
                             + (" (17 kernels back to back, profiles/r06_c2_hyper_timeline.txt)" if a.config == "c2" else ""),
                # the GEMM-shaped launches of one iteration (round 4: seven, round 3: nine + the symmetric Apred product) with the
                # flops they execute against what a dense 2 n^3-style count credits them (triangular operands, symmetric results)
                "products": _hyper_products(mpad, (B + 63) // 64 * 64)}
            if a.config == "c2":
                tr = _pmc_traffic("hyper", out["hyper_roofline"]["kernel"], step_inst=False)
                out["hyper_roofline"]["traffic"] = tr.get("traffic")
                out["hyper_roofline"]["traffic_unit"] = "bytes/launch"
                if tr:
                    out["hyper_roofline"]["traffic_source"] = tr["traffic_source"]
                    out["hyper_roofline"]["traffic_kernel"] = tr["traffic_kernel"]
            ngr, ngf = C.c_int64(), C.c_int64()
            if hasattr(L, "agp_svgp_hyper_counters"):
                mh._chk(L.agp_svgp_hyper_counters(hh, C.byref(ngr), C.byref(ngf)))
                out["hyper_roofline"]["gradients_with_one_product_G_K"] = f"{ngf.value} of {ngr.value}"
        del mh, cfg_h
        # streaming predict_f (means) over all N points: K_*m is never materialised
        mu_out = torch.empty(1, N, dtype=model.tdtype, device=dev)
        model._chk(L.agp_svgp_predict_f(h, xp, ld, N, C.c_void_p(mu_out.data_ptr()), None))
        torch.cuda.synchronize()
        tp = time.perf_counter()
        model._chk(L.agp_svgp_predict_f(h, xp, ld, N, C.c_void_p(mu_out.data_ptr()), None))
        torch.cuda.synchronize()
        tp = time.perf_counter() - tp
        es = 4 if f32 else 8
        out["predict_f_mean_all_N"] = {"seconds": round(tp, 4), "points_per_s": round(N / tp, 1),
                                       "hbm_GBps_algorithmic": round((N * D * es + N * es) / tp / 1e9, 2),
                                       "algorithmic_TFLOPs": round(N * m * (3 * D + 14) / tp / 1e12, 2)}
        # round 6: what bounds the streaming predictor (SURVEY 8d called it the HBM-bound measurement; it is not: N D + N elements of
        # traffic against N m kernel values).  1.5 s of back-to-back predictions with the engine clock and socket power sampled.
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from clock_sampler import ClockSampler

            smp = ClockSampler(local_rank, 20.0).start()
            tps, reps = time.perf_counter(), 0
            while time.perf_counter() - tps < 1.5:
                for _ in range(20):
                    model._chk(L.agp_svgp_predict_f(h, xp, ld, N, C.c_void_p(mu_out.data_ptr()), None))
                torch.cuda.synchronize()
                reps += 20
            tpl = (time.perf_counter() - tps) / reps
            clk = smp.stop()
            nval = float(N) * m
            # executed per kernel value: the cross term on the MFMA pipe (2 D flops) + the VALU instructions of the epilogue
            # (fp64 squared-exponential: 22, of which 16 are FMAs -- s2, d2, two clamps, exp_mhalf's 17, the row-dot FMA; the
            # general path ~48: csrc/agp_cavi.h); every fraction against the datasheet peaks
            valu_per_value = 22 if (not f32 and cfg["kernel"] == "sqexp") else 48
            # ... and the kernel's TOTAL VALU instructions per value from the committed counter pass of the same kernel (SQ_INSTS_VALU
            # minus SQ_INSTS_MFMA, profiles/r06_predict_pmc.json: the epilogue + the per-tile copy / address work amortised over a
            # lane's 16 values), which is what the VALU share below is computed from when the file covers this kernel
            valu_total, valu_src = float(valu_per_value), "ISA count of the epilogue only"
            try:
                with open(os.path.join(ROOT, "profiles", "r06_predict_pmc.json")) as fh:
                    pm = json.load(fh)
                if not f32 and cfg["kernel"] == "sqexp" and pm["m"] == m:
                    valu_total = float(pm["derived"]["non_mfma_valu_per_kernel_value_lanes"])
                    valu_src = "profiles/r06_predict_pmc.json (rocprofv3 --pmc SQ_INSTS_VALU / SQ_INSTS_MFMA, tools/pmc_predict.py)"
            except Exception:
                pass
            vpeak = peak  # the VALU's FMA rate equals the MFMA rate in fp64 (78.6 TF); fp32: quoted against the MFMA peak as well
            out["predict_roofline"] = {
                "kernel": f"k_kernelmatrix_mma<{tname}, {'K_SQEXP' if cfg['kernel'] == 'sqexp' else 'K_MATERN52'}, 1> (streaming: K_*m never stored)",
                "seconds_per_pass": round(tpl, 5), "kernel_values_per_s": round(nval / tpl, 1), "exp_per_s": round(nval / tpl, 1),
                "bound": "valu + mfma issue (neither HBM nor a single pipe)",
                "hbm": {"achieved": round((N * D * es + N * es) / tpl / 1e9, 1), "peak": 8000.0,
                        "unit": "GB/s", "frac": round((N * D * es + N * es) / tpl / 1e9 / 8000.0, 4)},
                "mfma": {"achieved": round(2.0 * nval * D / tpl / 1e12, 2), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(2.0 * nval * D / tpl / 1e12 / peak, 4), "what": "cross term x.z of the squared distances"},
                "valu": {"instructions_per_value": valu_per_value, "instructions_per_value_total": valu_total,
                         "instructions_per_value_total_source": valu_src,
                         "achieved": round(2.0 * valu_total * nval / tpl / 1e12, 2),
                         "peak": vpeak, "unit": "TFLOP/s (every VALU instruction counted as an FMA)",
                         "frac": round(2.0 * valu_total * nval / tpl / 1e12 / vpeak, 4)},
                "combined_frac_of_one_pipe": round((2.0 * nval * D + 2.0 * valu_total * nval) / tpl / 1e12 / peak, 4),
                "clock_power_during_the_loop": clk,
                "note": "MFMA and VALU work of different waves overlap; their sum runs at about the rate the register-only MFMA loop "
                        "sustains under the socket power limit (mfma_sustained) -- DESIGN.md section 4",
            }
            try:  # fabric bytes per pass from the same counter file (FETCH_SIZE x 2 + WRITE_SIZE, separate passes)
                if valu_src.startswith("profiles/"):
                    out["predict_roofline"]["hbm"]["traffic"] = pm["derived"]["fabric_bytes_per_launch_corrected"]
                    out["predict_roofline"]["hbm"]["algorithmic_bytes"] = int(N * D * es + N * es)
            except Exception:
                pass
        except Exception as ex:
            out["predict_roofline"] = {"error": repr(ex)}

    # ---- time to ELBO tolerance (build-defined, SURVEY.md 8d: the reference has no stopping rule) ----
    if a.full and not a.no_elbo_tol and rank == 0 and world == 1 and single_latent:
        EVAL = 8192
        eval_idx = torch.as_tensor(np.random.default_rng(77).choice(N, EVAL, replace=False).astype(np.int64), device=dev)
        model2 = build_model(AGP, cfg, ell, Z, B, 0, 1, local_rank, mode)
        model2.inference.rho = rho
        h2 = model2._ensure_handle(EVAL)
        model2._chk(L.agp_svgp_refresh_K(h2))
        rho_e = N / EVAL
        e = C.c_double()
        hist, it = [], 0
        # the contracted rule needs consecutive checks within 1e-4: with RobbinsMonro's (1 + t)^-0.51 step the minibatch noise of
        # the logistic model falls below that only after tens of thousands of iterations (C2: ~3e-4 at t = 6000), so the loop runs
        # up to 60 000 iterations or AGP_BENCH_ELBO_SECONDS (default 40 s), whichever comes first
        max_it = 60000
        t_cap = float(os.environ.get("AGP_BENCH_ELBO_SECONDS", "40"))
        rng2 = np.random.default_rng(99)
        chunk_np = np.stack([rng2.choice(N, B, replace=False) for _ in range(600)]).astype(np.int64)
        chunk = torch.as_tensor(chunk_np, device=dev)  # 600 distinct minibatches, cycled
        hit = {"raw": None, "smoothed": None, "reach": None}
        consec = consec_r = 0
        TOL_R = 1e-3  # the "reachable" consecutive-check rule: 4 x the measured noise floor of consecutive checks at C2 (2.5e-4)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        # round 4: the evaluations are ENQUEUED (agp_svgp_elbo_enqueue: the same kernels in the same place of the stream, the value
        # arrives in mapped host memory behind an event) and read one check later, while the next ten iterations are already in
        # the queue -- the host never waits on the stream inside the loop.  The rule sees exactly the same sequence of ELBO values;
        # its decision comes one check (ten iterations, ~3 ms at C2) after the check that satisfies it, and the reported time is
        # the wall-clock at which the host HAS that value.  AGP_BENCH_ELBO_SYNC=1 restores the synchronous evaluation.
        elbo_sync = os.environ.get("AGP_BENCH_ELBO_SYNC") == "1"
        # round 6: the checks run NEXT TO the training stream (agp_amd.SideObjective: a snapshot of (eta1, eta2) by two device
        # copies on the training stream, the evaluation -- kernel matrices of the 8192 points, local update, factorisation of -2 eta2
        # with its inverse, the ELBO's reductions -- on a side stream with a shadow handle of its own, values equal to a few ulp,
        # tests/test_gpu_round6.py).  In line a check cost the loop 0.87 ms between two 0.31 ms steps, 190 times.
        # AGP_BENCH_ELBO_INLINE=1 restores the in-line enqueued evaluation of rounds 4-5.
        elbo_side = (not elbo_sync) and os.environ.get("AGP_BENCH_ELBO_INLINE") != "1"
        side_prio = os.environ.get("AGP_BENCH_SIDE_PRIORITY")  # (development: -1 = high, 0 = normal; unset = the default stream priority)
        side = AGP.SideObjective(model2, EVAL, ring=4, priority=None if side_prio is None else int(side_prio)) if elbo_side else None
        tk, pending_tk, rdy = C.c_int32(), None, C.c_int32()
        side_q, side_lag = [], max(1, min(3, int(os.environ.get("AGP_BENCH_ELBO_LAG", "1"))))
        while it < max_it and (hit["raw"] is None or hit["smoothed"] is None or hit["reach"] is None) and \
                (time.perf_counter() - ts) < t_cap:
            for _ in range(10):
                st = L.agp_svgp_cavi_step(h2, xp, ld, yp, C.c_void_p(chunk[it % chunk.shape[0]].data_ptr()), B, rho)
                if st != 0:
                    capi.check(model2._ctx, st)
                it += 1
                if use_prefetch:  # the same look-ahead as in the timed loop (the ELBO evaluation in between leaves it valid)
                    L.agp_svgp_prefetch(h2, xp, ld, C.c_void_p(chunk[it % chunk.shape[0]].data_ptr()), B)
            if elbo_sync:
                model2._chk(L.agp_svgp_elbo(h2, xp, ld, yp, C.c_void_p(eval_idx.data_ptr()), EVAL, rho_e, 1, C.byref(e)))
                it_of_value = it
            elif elbo_side:
                # (side_q: tickets in flight, oldest first; a value is read `side_lag` checks after it was enqueued -- with one check
                #  of lag the host can wait for a side stream that shares the chip with ten training steps; SideObjective's ring
                #  holds four snapshots)
                side_q.append((side.enqueue(eng._X, eng._y, eval_idx, EVAL, rho_e), it))
                if len(side_q) <= side_lag:
                    continue
                prev = side_q.pop(0)
                e.value = side.fetch(prev[0])
                it_of_value = prev[1]
            else:
                model2._chk(L.agp_svgp_elbo_enqueue(h2, xp, ld, yp, C.c_void_p(eval_idx.data_ptr()), EVAL, rho_e, 1, C.byref(tk)))
                prev, pending_tk = pending_tk, (tk.value, it)
                if prev is None:
                    continue
                model2._chk(L.agp_svgp_elbo_fetch(h2, prev[0], 1, C.byref(e), C.byref(rdy)))
                it_of_value = prev[1]
            hist.append(e.value)
            now = time.perf_counter() - ts
            if len(hist) >= 2:
                consec = consec + 1 if abs(hist[-1] - hist[-2]) / abs(hist[-1]) < 1e-4 else 0
                if hit["raw"] is None and consec >= 3:
                    hit["raw"] = (now, it_of_value, hist[-1])
                consec_r = consec_r + 1 if abs(hist[-1] - hist[-2]) / abs(hist[-1]) < TOL_R else 0
                if hit["reach"] is None and consec_r >= 3:
                    hit["reach"] = (now, it_of_value, hist[-1])
            if hit["smoothed"] is None and len(hist) >= 20:
                m1, m0 = sum(hist[-10:]) / 10.0, sum(hist[-20:-10]) / 10.0
                if abs(m1 - m0) / abs(m1) < 1e-3:
                    hit["smoothed"] = (now, it_of_value, hist[-1])
        for tq in side_q:  # close the tickets still open
            side.fetch(tq[0])
        if pending_tk is not None:  # close the last ticket
            if elbo_side:
                pass
            else:
                model2._chk(L.agp_svgp_elbo_fetch(h2, pending_tk[0], 1, C.byref(e), C.byref(rdy)))
        torch.cuda.synchronize()
        # contracted rule: |ELBO_t - ELBO_{t-10}| / |ELBO_t| < 1e-4 for 3 consecutive checks
        out["time_to_elbo_tol_s"] = round(hit["raw"][0], 4) if hit["raw"] else None
        out["iters_to_elbo_tol"] = hit["raw"][1] if hit["raw"] else None
        out["elbo_at_tol"] = hit["raw"][2] if hit["raw"] else None
        out["elbo_tol_rule"] = ("SURVEY 8d: ELBO (corrected, fresh local variables) on a fixed 8192-point batch every 10 iterations; stop "
                                "when |ELBO_t - ELBO_{t-10}| / |ELBO_t| < 1e-4 for 3 consecutive checks; wall-clock includes the "
                                f"ELBO evaluations; null = not reached within {it} iterations / {t_cap:.0f} s"
                                + ("" if elbo_sync else "; evaluations " + ("on a side stream from a snapshot of (eta1, eta2) "
                                   "(agp_amd.SideObjective)" if elbo_side else "enqueued in the training stream")
                                   + " and read one check later: reported seconds = when the host has the deciding value, "
                                   "reported iterations = the iteration that value belongs to"))
        out["elbo_checks"] = "side stream (SideObjective)" if elbo_side else ("synchronous" if elbo_sync else "in-line, enqueued")
        if len(hist) > 20:  # what the rule is up against: the spread of consecutive checks at the end of the run
            d = np.abs(np.diff(hist[-101:])) / np.abs(np.asarray(hist[-100:] if len(hist) > 100 else hist[1:]))
            out["elbo_check_noise_floor"] = {"median_rel_change_of_consecutive_checks": float(np.median(d)),
                                             "max": float(np.max(d)), "over_last_checks": int(len(d)), "at_iteration": it}
        # the same three-consecutive-checks rule at a tolerance both sides can meet: 1e-3 = 4 x the noise floor
        out["time_to_elbo_tol_reachable"] = {
            "seconds": round(hit["reach"][0], 4) if hit["reach"] else None,
            "iters": hit["reach"][1] if hit["reach"] else None,
            "elbo": hit["reach"][2] if hit["reach"] else None,
            "rule": f"the contracted rule's three consecutive checks (10 iterations apart, same 8192-point evaluation batch) at "
                    f"|dELBO| / |ELBO| < {TOL_R:g} = 4 x the measured noise floor of consecutive checks (2.5e-4 at C2); device AND "
                    "CPU oracle are RUN through it (cpu_baseline.time_to_elbo_tol_reachable_measured)",
        }
        out["_elbo_ctx"] = {"chunk": chunk_np, "eval_idx": eval_idx.cpu().numpy(), "EVAL": EVAL, "tol_reachable": TOL_R}
        out["time_to_elbo_tol_smoothed"] = {
            "seconds": round(hit["smoothed"][0], 4) if hit["smoothed"] else None,
            "iters": hit["smoothed"][1] if hit["smoothed"] else None,
            "elbo": hit["smoothed"][2] if hit["smoothed"] else None,
            "rule": "mean of the last 10 checks moved < 1e-3 (relative) against the 10 before (the round-1 rule: robust to minibatch noise)",
        }
        if os.environ.get("AGP_BENCH_TRACE"):
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "elbo_trace.json"), "w") as fh:
                json.dump(hist, fh)
        del model2

    # ---- sustained MFMA rate with clock / power samples (rank 0, single GPU) -- LAST of the GPU sections: three seconds at ~0.9 kW
    # leave the chip warm enough to slow whatever is measured right behind them (the time-to-ELBO loop ran 35 % longer there) ----
    # The register-only MFMA issue loop for 3 s with the engine clock and socket power sampled at >= 10 Hz while it runs
    # (tools/clock_sampler.py): what "sustained" means on this box.  The clock the rate itself implies (every SIMD issuing back to
    # back: 256 CUs x 4 SIMDs x 2048 flop per 64-cycle v_mfma_f64_16x16x4, half the cycles in fp32) is printed next to it.
    if a.full and rank == 0 and world == 1 and not a.no_extras:
        pk = C.c_double()
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from clock_sampler import ClockSampler

            idle = ClockSampler(local_rank, 20.0).start()
            time.sleep(0.5)
            idle_s = idle.stop()
            smp = ClockSampler(local_rank, 20.0).start()
            vals, t0s = [], time.perf_counter()
            while time.perf_counter() - t0s < 3.0:
                if L.agp_mfma_peak(model._ctx, capi.F32 if f32 else capi.F64, C.byref(pk)) != 0:
                    break
                vals.append(pk.value)
            sus = smp.stop()
            if vals:
                tf = float(np.median(vals))
                flop_per_cycle = 256 * 4 * 2048 / (32.0 if f32 else 64.0)
                out["mfma_sustained"] = {"tflops": round(tf, 1), "calls": len(vals), "seconds": 3.0,
                                         "implied_clock_mhz": round(tf * 1e12 / flop_per_cycle / 1e6, 0),
                                         "idle": {k: idle_s[k] for k in ("sclk_mhz", "power_w")}, **sus}
            # the same readings while the workload's own steps run (2 s)
            smp = ClockSampler(local_rank, 20.0).start()
            t0s, j = time.perf_counter(), 0
            while time.perf_counter() - t0s < 2.0:
                for _ in range(50):
                    if use_multi:
                        st = L.agp_svgp_cavi_step_multi(h, None, smode, xp, ld, yp, C.c_void_p(idx_all[j % total].data_ptr()), B, rho)
                    else:
                        st = L.agp_svgp_cavi_step(h, xp, ld, yp, C.c_void_p(idx_all[j % total].data_ptr()), B, rho)
                    if st != 0:
                        capi.check(model._ctx, st)
                    j += 1
                    if use_prefetch:
                        L.agp_svgp_prefetch(h, xp, ld, C.c_void_p(idx_all[j % total].data_ptr()), B)
                torch.cuda.synchronize()
            out["step_clock"] = {"steps": j, **smp.stop()}
            model._chk(L.agp_svgp_check_status(h))
        except Exception as ex:  # a missing SMI library must not cost the line
            out["mfma_sustained"] = {"error": repr(ex)}

    # ---- CPU baseline: the oracle (numpy/scipy LAPACK) on the host cores, same workload, bounded sample ----
    if a.full and not a.no_cpu_baseline and rank == 0 and world == 1:
        out["cpu_baseline"] = cpu_baseline(a, cfg, ell, Z, X, yh, idx_np, out)

    # RCCL writes its version banner through C stdio (buffered when stdout is a pipe; it would come out at exit, after the JSON
    # line): flush that buffer first, print the line, and only then tear the communicators down (a teardown that hangs must not
    # cost the result)
    if dist is not None:
        dist.barrier()
    flush_c_stdio()
    out.pop("_elbo_ctx", None)
    if rank == 0:
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if comm is not None:
        comm.destroy()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    flush_c_stdio()


def cpu_baseline(a, cfg, ell, Z, X, yh, idx_np, out):
    """The NumPy/SciPy (OpenBLAS) oracle on the GPU box's host cores: same config, same index stream, a bounded sample."""
    from threadpoolctl import threadpool_info, threadpool_limits

    from oracle import agp_ref as R

    N, D, m, B = cfg["N"], cfg["D"], cfg["m"], cfg["B"]
    avail = len(os.sched_getaffinity(0))
    need = np.unique(idx_np[: max(8, min(len(idx_np), 400))].ravel())  # only the rows the sample touches leave the device
    remap = np.full(N, -1, dtype=np.int64)
    remap[need] = np.arange(len(need))
    Xh = X[torch.as_tensor(need, device=X.device)].cpu().numpy().astype(np.float64)
    lik = cfg["lik"]
    if lik == "mo":
        yt = [np.asarray(t)[need] for t in yh]
    else:
        yt = np.asarray(yh)[need]
    total = min(len(idx_np), 400)

    def fresh_ref():
        kern = R.Kernel("sqexponential" if cfg["kernel"] == "sqexp" else "matern52", 1.0 / ell, 1.0)
        kern.fast = True  # GEMM form of the distances: the favourable-to-CPU variant
        if lik == "logistic":
            r = R.SVGP(kern, R.LogisticLikelihood(), Z, stochastic=True, batchsize=B)
        elif lik == "studentt":
            r = R.SVGP(kern, R.StudentTLikelihood(3.0, 1.0), Z, stochastic=True, batchsize=B)
        elif lik == "lsm":
            r = R.SVGP(kern, R.LogisticSoftMaxLikelihood(cfg["K"]), Z, stochastic=True, batchsize=B)
        else:
            nq = min(cfg["K"], cfg["c5_latents"])
            r = R.MOSVGP(kern, [R.GaussianLikelihood(0.05), R.GaussianLikelihood(0.05), R.LogisticLikelihood(),
                                R.LogisticLikelihood()], [Z] * nq, cfg["A"][:, :nq], stochastic=True, batchsize=B,
                         A_opt=R.Adam(0.01))
        r.rho = N / B
        return r

    if lik == "lsm":
        ytr = R.treat_labels(yt, R.LogisticSoftMaxLikelihood(cfg["K"]))
    elif lik == "mo":
        ytr = None
    else:
        ytr = R.treat_labels(yt, fresh_ref().likelihood)

    def one(r, q):
        ib = remap[idx_np[q % total][:B]]
        if lik == "mo":  # update_parameters!(::MOSVGP) training.jl:153-158, spelled out by the oracle's train loop
            if r.local_vars is None:
                r.local_vars = [R.init_local_vars_single(l, B) for l in r.likelihoods]
            yb = [np.asarray(t, dtype=np.float64)[ib] for t in yt]
            r.compute_kernel_matrices(Xh[ib])
            r.update_A(yb)
            r.variational_updates(yb)
        else:
            r.update_parameters(Xh[ib], ytr[ib])

    # pick the BLAS thread count that is fastest on this host for these LAPACK calls -- at most as many threads as the BLAS pools
    # were started with (OMP_NUM_THREADS / OPENBLAS_NUM_THREADS): OpenBLAS cannot grow its pool past that size, asking it to
    # crashes the process inside LAPACK
    pools = [p["num_threads"] for p in threadpool_info() if p.get("user_api") == "blas"]
    cap = min([avail] + pools)
    best_thr, best_t = 1, float("inf")
    for thr in sorted({t for t in (8, 16, 32, 64, cap) if t <= cap}):
        with threadpool_limits(limits=thr):
            r = fresh_ref()
            one(r, 0)
            tt = time.perf_counter()
            one(r, 1)
            tq = time.perf_counter() - tt
        if tq < best_t:
            best_thr, best_t = thr, tq
        if tq > 8.0:
            break  # large configs: do not spend the whole budget on the thread sweep
    n_cpu, tcpu = 0, 0.0
    with threadpool_limits(limits=best_thr):
        ref = fresh_ref()
        t_start = time.perf_counter()
        while True:
            tt = time.perf_counter()
            one(ref, n_cpu)
            tcpu += time.perf_counter() - tt
            n_cpu += 1
            if (time.perf_counter() - t_start) > a.cpu_seconds and n_cpu >= 2:
                break
    rate = n_cpu / tcpu
    # ... and a single-thread run next to it, a few iterations only
    one_thr = None
    if lik in ("logistic", "studentt"):
        with threadpool_limits(limits=1):
            r1 = fresh_ref()
            one(r1, 0)
            t1, n1 = time.perf_counter(), 0
            while n1 < 3 and (time.perf_counter() - t1) < 10.0:
                one(r1, 1 + n1)
                n1 += 1
            one_thr = round(n1 / (time.perf_counter() - t1), 3)
    res = {
        "value": round(rate, 3),
        "unit": "iter/s",
        "cores": best_thr,
        "single_thread_value": one_thr,
        "kind": "port",
        "sample": f"{n_cpu} iterations of the same workload ({out['config']['workload']}) with the NumPy/SciPy(OpenBLAS) oracle "
                  f"(GEMM-form distances, best of {{8,16,32,64,all}} BLAS threads up to the pool's {cap}; host has {avail} cores), {tcpu:.1f} s of CPU "
                  f"work" + (f"; {min(cfg['K'], cfg['c5_latents'])} of the 16 latents, like the GPU line" if lik == "mo" else ""),
    }
    # the same rule on the same index stream needs the same number of iterations: extrapolated where running it would take many
    # minutes (the contracted rule at C2: tens of thousands of iterations at ~17 it/s) ...
    if out.get("iters_to_elbo_tol"):
        res["time_to_elbo_tol_s_extrapolated"] = round(out["iters_to_elbo_tol"] / rate, 1)
    sm = (out.get("time_to_elbo_tol_smoothed") or {}).get("iters")
    if sm:
        res["time_to_elbo_tol_smoothed_s_extrapolated"] = round(sm / rate, 1)
    # ... and RUN where it is affordable: the smoothed rule with the oracle on the host cores, same minibatch stream, same
    # evaluation batch, same rule, wall-clock including the ELBO evaluations (budget --cpu-elbo-seconds; 0 skips it)
    ctx = out.get("_elbo_ctx")
    budget = float(getattr(a, "cpu_elbo_seconds", 0.0))
    want_r = bool(out.get("iters_to_elbo_tol"))  # the contracted rule was met on the device: run the oracle through it as well
    rc_it = (out.get("time_to_elbo_tol_reachable") or {}).get("iters")
    if rc_it:
        res["time_to_elbo_tol_reachable_s_extrapolated"] = round(rc_it / rate, 1)
    need_it = sm or 0  # the run starts when at least the smoothed rule fits the budget; the other rules are met if the budget lasts
    if ctx is not None and sm and lik in ("logistic", "studentt") and budget > 0 and need_it / rate < budget:
        Xall = X.cpu().numpy().astype(np.float64)
        yall = np.asarray(yh, dtype=np.float64)
        with threadpool_limits(limits=best_thr):
            r = fresh_ref()
            yall_t = R.treat_labels(yall, r.likelihood)
            ev = ctx["eval_idx"]
            Xe, ye = Xall[ev], yall_t[ev]
            hist, it, hit_s, hit_r, consec = [], 0, None, None, 0
            hit_q, consec_q, tol_q = None, 0, ctx.get("tol_reachable", 1e-3)
            ts = time.perf_counter()
            while (time.perf_counter() - ts) < budget and (hit_s is None or (want_r and hit_r is None) or (rc_it and hit_q is None)):
                for _ in range(10):
                    ib = ctx["chunk"][it % len(ctx["chunk"])]
                    r.update_parameters(Xall[ib], yall_t[ib])
                    it += 1
                hist.append(r.elbo_fresh(Xe, ye, N / ctx["EVAL"]))
                now = time.perf_counter() - ts
                if len(hist) >= 2:
                    consec = consec + 1 if abs(hist[-1] - hist[-2]) / abs(hist[-1]) < 1e-4 else 0
                    if hit_r is None and consec >= 3:
                        hit_r = (now, it)
                    consec_q = consec_q + 1 if abs(hist[-1] - hist[-2]) / abs(hist[-1]) < tol_q else 0
                    if hit_q is None and consec_q >= 3:
                        hit_q = (now, it, hist[-1])
                if len(hist) >= 20 and hit_s is None:
                    m1, m0 = sum(hist[-10:]) / 10.0, sum(hist[-20:-10]) / 10.0
                    if abs(m1 - m0) / abs(m1) < 1e-3:
                        hit_s = (now, it, hist[-1])
        res["time_to_elbo_tol_smoothed_measured"] = {
            "seconds": round(hit_s[0], 1) if hit_s else None, "iters": hit_s[1] if hit_s else None,
            "elbo": hit_s[2] if hit_s else None,
            "note": "the oracle RUN through the same rule on the same minibatch stream and evaluation batch (not extrapolated)"}
        res["time_to_elbo_tol_reachable_measured"] = {
            "seconds": round(hit_q[0], 1) if hit_q else None, "iters": hit_q[1] if hit_q else None,
            "elbo": hit_q[2] if hit_q else None,
            "note": f"three consecutive checks within {tol_q:g}: the oracle RUN on the host cores, same minibatch stream and evaluation batch"}
        if hit_r:
            res["time_to_elbo_tol_measured"] = {"seconds": round(hit_r[0], 1), "iters": hit_r[1],
                                                "note": "the contracted rule (SURVEY 8d), oracle RUN on the host cores"}
    return res


if __name__ == "__main__":
    main()
