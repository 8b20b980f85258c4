#!/usr/bin/env python
"""bench.py — graphs/sec of the SignNet+GINE forward (BASELINE.json metric) on N MI355X.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = one eval-mode forward of `SignNetGNN(None, None, 128, 1, 4, 6)` (GINESignNetPyG
defaults, core/config.py:30,53-57) over one synthetic ZINC-like batch of 128 graphs with the
first k=16 eigenvectors (BASELINE.json configs[1]), inputs resident in HBM.  Multi-GPU: the batch
of 128*N graphs is sharded by graph, 128 per rank, no data-path collective (weak scaling).
Rank 0 prints ONE JSON line.

A plain run sets up, warms up (W forwards, then untimed forwards until --clock-ramp-ms of wall time has passed: the GPU reaches its
sustained clock), times the K steps and prints the headline line (`metric`, `value`, `unit`, `ms_per_step`, ...).  `--full` adds every
extra measurement and check of the forward bench to the same line (cold pass, roofline and per-kernel figures, the module's other
modes, the CPU baseline, ...).  `--dump-outputs DIR` writes the predictions of the last timed step as DIR/y.npy (float32); the inputs
and weights are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_F32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: fp32 MFMA (f32 in / f32 acc) dense peak
VALU_F32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: "Peak FP32 (vector) 157.3 TFLOPS (spec)" (packed v_pk_fma_f32; scalar-width FMAs issue at half of it)

DOMINANT = "sn_phi_fused_f32"     # the kernel the roofline block is quoted on (largest share of the step)
# what bounds a kernel whose MFMA fraction alone would mislead (kernels.* block of the line)
KERNEL_BOUND_NOTES = {
    "sn_gnn_fused_f32": {"bound": "latency chain",
                         "bound_note": "one workgroup per graph walks ~22 dependent stages (encoders, 6 x [aggregate, Linear, Linear], pooling, head) "
                                       "with a workgroup barrier between them; its duration is the largest graph's chain and does not depend on the "
                                       "batch size (128 of 256 CUs busy at 128 graphs), so `frac` (MFMA) is not what limits it"},
    "sn_batch_plan": {"bound": "latency chain",
                      "bound_note": "three workgroups (CSR, phi columns, rho bins): dependent scans / a packing chain, no throughput bound applies"},
}
# BASELINE.json `configs`: [1] is the configuration the metric is quoted on (the default and the driver's bench line);
# [0] and [2] can be selected with --config for extra measurements (they are parity-test cases, not the headline).
WORKLOADS = {
    1: dict(name="ZINC SignNet k=16 hidden=128 batch=128 (GINESignNetPyG SignNetGNN(None,None,128,1,4,6))",
            variant="gine", node_feat=None, edge_feat=None, features="zinc", n_lo=9, n_hi=37,
            B=128, k=16, hidden=128, nl_signnet=4, nl_rho=1, nl_gnn=6, n_out=1),
    0: dict(name="ZINC-subset SignNet k=8 hidden=64 batch=32 (GINESignNetPyG SignNetGNN(None,None,64,1,4,6))",
            variant="gine", node_feat=None, edge_feat=None, features="zinc", n_lo=9, n_hi=37,
            B=32, k=8, hidden=64, nl_signnet=4, nl_rho=1, nl_gnn=6, n_out=1),
    2: dict(name="Alchemy SignNet batch=256 (main_alchemy.py:35 SignNetGNN(6,4,108,12,8,16), all eigenvectors)",
            variant="alchemy", node_feat=6, edge_feat=4, features="alchemy", n_lo=6, n_hi=14,
            B=256, k=None, hidden=108, nl_signnet=8, nl_rho=4, nl_gnn=16, n_out=12),
}
WORKLOAD = WORKLOADS[1]


def build_model(dev, k="workload"):
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    m = SignNetGNN(WORKLOAD["node_feat"], WORKLOAD["edge_feat"], WORKLOAD["hidden"], WORKLOAD["n_out"], WORKLOAD["nl_signnet"],
                   WORKLOAD["nl_gnn"], variant=WORKLOAD["variant"], max_k=WORKLOAD["k"] if k == "workload" else k)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():          # eval-BN must not be the identity
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m.to(dev).eval()


def algorithmic_flops(data, k, d, L_phi, L_rho, L_g):
    """Dense-contraction flops of one forward on this batch (SURVEY.md §8(d) formulas, valid rows only)."""
    n = torch.tensor(data.sizes, dtype=torch.float64)
    kk = torch.clamp(n, max=k) if k else n                # slots per node: min(n_graph, k), or all eigenvectors
    M = float((n * kk).sum())                             # valid (node, slot) rows
    N = float(n.sum())
    phi = 2 * (L_phi - 1) * 2 * 2 * M * d * d + 2 * 2 * M * d           # hidden layers, both signs (+ tiny first layer)
    rho = L_rho * (6 * 2 * M * d * d + 4 * float((n * kk ** 2).sum()) * d) + 2 * N * d * d
    if WORKLOAD["variant"] == "alchemy":                  # first phi layer is 1 -> d -> d; eigenvalue encoder 1 -> d -> d
        phi += 2 * 2 * M * d * d
        rho += 2 * M * d * d
    gnn = 2 * N * 2 * d * d + L_g * 2 * 2 * N * d * d + 2 * len(data.sizes) * d * d
    return dict(phi=phi, rho=rho, gnn=gnn, total=phi + rho + gnn, M=M, N=N)


def cpu_model_string():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n)
    except Exception:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def cpu_baseline(data, model_cpu_sd, budget_s=8.0):
    """The oracle (CPU restatement of the reference) timed on this host's cores over the SAME batch.  SURVEY.md section 8(d)'s protocol:
    `torch.set_num_threads(P)` with P = all PHYSICAL cores of the host and P = 1, 3 warm-up + 10 timed forwards each, median, CPU
    model stated (`protocol_8d` entries of the sweep).  Kept as extras: P = 8 and P = 32 (1 warm-up + up to 5 forwards inside a
    time budget).  `value` is the BEST of the sweep (a CPU baseline de-tuned by oversubscription would flatter the ratio: on the
    128-thread hosts of this pool a few threads beat all of them on these small matrices), `cores` the P it was reached with."""
    from oracle import pyg_signnet as O
    cfg = O.make_cfg(WORKLOAD["variant"], WORKLOAD["node_feat"], WORKLOAD["edge_feat"], WORKLOAD["hidden"], WORKLOAD["n_out"],
                     WORKLOAD["nl_signnet"], WORKLOAD["nl_gnn"])
    cores = torch.get_num_threads()
    phys = min(physical_cores(), cores) if cores > 1 else 1

    def fwd(batch):
        t0 = time.perf_counter()
        O.signnet_gnn(model_cpu_sd, cfg, batch, training=False, max_k=WORKLOAD["k"])
        return time.perf_counter() - t0

    def run(batch, warm, timed, budget=None):
        with torch.no_grad():
            first = [fwd(batch) for _ in range(warm)][-1]
            if budget is not None:
                timed = max(1, min(timed, int(budget / max(first, 1e-3))))
            ts = [fwd(batch) for _ in range(timed)]
        return sorted(ts)[len(ts) // 2], timed

    sweep = []
    try:
        for p_ in sorted({1, phys}):
            torch.set_num_threads(p_)
            med, iters = run(data, 3, 10)
            sweep.append(dict(cores=p_, value=len(data.sizes) / med, warmup=3, forwards=iters, protocol_8d=True))
        extra = sorted({p for p in (8, 32) if p <= cores} - {1, phys})
        for p_ in extra:
            torch.set_num_threads(p_)
            med, iters = run(data, 1, 5, budget_s / max(1, len(extra)))
            sweep.append(dict(cores=p_, value=len(data.sizes) / med, warmup=1, forwards=iters, protocol_8d=False))
    finally:
        torch.set_num_threads(cores)
    sweep.sort(key=lambda r: r["cores"])
    best = max(sweep, key=lambda r: r["value"])
    out = dict(value=best["value"], unit="graphs/s", cores=best["cores"], kind="port", cpu_model=cpu_model_string(),
               logical_cpus=os.cpu_count(), physical_cores=phys, sweep=sweep,
               sample=f"best of torch.set_num_threads(P) over the sweep: median of {best['forwards']} forward(s) of the same "
                      f"{len(data.sizes)}-graph batch after {best['warmup']} warm-up(s); P = 1 and P = {phys} (physical cores) follow "
                      f"SURVEY 8(d) (3 warm-up + 10 timed, median); oracle/pyg_signnet.py (torch CPU fp32)")
    one = [r for r in sweep if r["cores"] == 1]
    if one:
        out["single_thread"] = dict(value=one[0]["value"], unit="graphs/s", cores=1)
    allp = [r for r in sweep if r["cores"] == phys]
    if allp:
        out["all_physical_cores"] = dict(value=allp[0]["value"], unit="graphs/s", cores=phys)
    return out


def evd_bench(args, dev):
    """Secondary workload (not the headline metric): `--workload evd` times the batched Laplacian
    eigendecomposition (sn_laplacian_evd_f32) that produces the forward's eigen-data, on the same 128-graph batch
    and on a large batch for the throughput limit.  Prints its own JSON line."""
    import numpy as np
    from oracle import evd as OE
    from signnet_basisnet_amd import ops, synth
    out = {"metric": "graphs/sec batched Laplacian eigendecomposition ('sym'), ZINC-like graphs", "unit": "graphs/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "dtype": "f32", "data": "synthetic",
           "vs_baseline": None, "roofline": None,
           "roofline_note": "one-sided Jacobi in registers, four waves per graph (rows dealt round-robin, the partial dot products "
                            "meet in LDS once per rotation step): bound by the step's DEPENDENT chain — partner rows through "
                            "ds_bpermute -> dot products -> LDS meeting + barrier -> rotation parameters -> update — of which a sweep "
                            "has n - 1 and a graph ~9 sweeps; neither HBM nor MFMA.  `roofline` prices the arithmetic of those steps "
                            "against the fp32 VECTOR peak (the pipe it runs on): the fraction is the VALU-issue share of the chain"}
    for tag, B in (("batch128", WORKLOAD["B"]), ("batch8192", 8192)):
        base = synth.make_batch(min(B, 1024), seed=1236)
        reps = max(1, B // 1024)
        ei = torch.cat([base.edge_index + r * base.num_nodes for r in range(reps)], 1)
        sizes = list(base.sizes) * reps
        gp = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
        eid, N, total = ei.to(dev), sum(sizes), sum(v * v for v in sizes)
        for _ in range(args.warmup):
            ops.laplacian_evd(eid, gp, N, total, "sym")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            st = ops.laplacian_evd(eid, gp, N, total, "sym")[-1]
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        out[tag] = {"graphs": len(sizes), "nodes": N, "ms_per_step": 1e3 * dt, "value": len(sizes) / dt,
                    "status": st.tolist()}
        # arithmetic of the Jacobi steps: per sweep m - 1 steps (m = n rounded to even), per step and column n rows x (2 FMA of the two
        # dot products + 4 FMA of the G and V updates) = 12 flop; sweeps = the measured maximum (status[1] - 1 rotating sweeps + the
        # confirming one), an upper bound for the smaller graphs
        sweeps = max(1, int(st[1].item()))
        flops = sum(sweeps * ((v + 1) // 2 * 2 - 1) * v * v * 12.0 for v in sizes)
        out[tag]["jacobi_gflop"] = flops / 1e9
        if tag == "batch128":
            ach = flops / dt / 1e12
            out["roofline"] = {"bound": "valu (latency chain)", "achieved": ach, "peak": VALU_F32_PEAK_TF, "unit": "TFLOP/s", "frac": ach / VALU_F32_PEAK_TF,
                               "traffic": None, "sweeps": sweeps,
                               "note": "achieved = 12 flop x rows x columns x steps of every graph / wall time of the whole call (memset, class "
                                       "lists, adjacency scatter and the Jacobi launch); peak = the fp32 vector peak of MI355X_MICROARCH.md (157.3 TFLOP/s, packed "
                                       "FMA)"}
            out["value"], out["ms_per_step"] = len(sizes) / dt, 1e3 * dt
            out["config"] = {"workload": f"EVDTransform('sym') of one collated batch of {len(sizes)} ZINC-like graphs (n 9..37)"}
            t0 = time.perf_counter()
            n_rep = 0
            while time.perf_counter() - t0 < 10.0:
                OE.evd_batch(ei.numpy(), sizes, "sym")
                n_rep += 1
            out["cpu_baseline"] = {"value": n_rep * len(sizes) / (time.perf_counter() - t0), "unit": "graphs/s", "cores": 1,
                                   "kind": "port", "sample": f"{n_rep} passes over the same batch, oracle/evd.py "
                                   "(numpy LAPACK ssyevd per graph, one thread, as a DataLoader worker runs the reference's transform)"}
    out["device"] = device_block(dev)
    print(json.dumps(out))


def device_block(dev):
    """Which device ran this line and at what clock: name, CU count, the driver's nominal clock and the clock MEASURED under load
    (sn_clock_probe: a wave counts 40 M shader cycles between two events, right behind ~50 ms of spinning that lets the part ramp) —
    the boxes of a pool differ by up to 10 % on the same kernels; with this block a box effect is distinguishable from a kernel edit."""
    import ctypes as C
    from signnet_basisnet_amd._lib import check, lib, stream
    cu, lds, khz = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().sn_device_info(C.byref(cu), C.byref(lds), C.byref(khz)), "sn_device_info")
    out = {"name": torch.cuda.get_device_name(dev), "cu_count": cu.value, "lds_bytes_per_cu": lds.value, "nominal_clock_mhz": khz.value / 1e3}
    try:
        buf = torch.zeros(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            check(lib().sn_clock_probe(120_000_000, buf.data_ptr(), stream()), "sn_clock_probe")       # ramp (~50 ms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib().sn_clock_probe(40_000_000, buf.data_ptr(), stream()), "sn_clock_probe")
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        out["measured_clock_mhz"] = int(buf.item()) / ms / 1e3
        out["probe"] = {"cycles": int(buf.item()), "ms": ms}
    except Exception as e:            # (the probe is evidence, not part of the measurement)
        out["measured_clock_mhz"] = None
        out["probe_error"] = str(e)[:200]
    return out


def train_roofline(fwd_flops, dt):
    """Whole training step against the pipes it actually runs on: the forward links and the backward links' dX product evaluate
    their fp32 Linears as six bf16 partial products (csrc/train.hip, split-bf16: 2500 / 6 = 416.7 TFLOP/s fp32-equivalent), the dW
    product (K = rows) stays on the fp32-input MFMA (157.3).  `peak` is the flop-weighted (harmonic) peak of the mix, `frac` =
    achieved / peak = (time of the step's flops at their pipes' peaks) / (measured time)."""
    split_peak = 2500.0 / 6.0
    pipes = [{"what": "forward links + backward dX (split-bf16, 6 partial products per fp32 product)", "flops": 2 * fwd_flops, "peak": split_peak},
             {"what": "backward dW (fp32-input MFMA)", "flops": fwd_flops, "peak": MFMA_F32_PEAK_TF}]
    t_peak = sum(p_["flops"] / (p_["peak"] * 1e12) for p_ in pipes)
    total = sum(p_["flops"] for p_ in pipes)
    ach = total / dt / 1e12
    peak = total / t_peak / 1e12
    return {"bound": "mfma", "unit": "TFLOP/s", "achieved": ach, "peak": peak, "frac": ach / peak, "pipes": pipes,
            "frac_vs_f32_mfma": ach / MFMA_F32_PEAK_TF, "traffic": None,
            "note": "whole step, ~3x the forward's dense flops (forward + dX + dW); one peak per pipe actually used and a flop-weighted "
                    "fraction (round 4 divided everything by the fp32-input MFMA peak, 157.3); the step is bound by ~100 launches of a "
                    "few us on 2 950-row tensors, not by either pipe"}


def train_bench(args, dev, dist=None, rank=0, world=1):
    """Secondary workload (not the headline metric): `--workload train` times full training steps
    (differentiable train-mode forward on the layer kernels, L1 loss, backward through the hand-written adjoints, one
    gradient all-reduce over RCCL when --gpus N > 1, one FlatAdam launch) of the headline model; every rank trains on its
    own 128-graph shard (weak scaling, BASELINE config 4's data-parallel pattern).  Rank 0 prints its own JSON line."""
    from signnet_basisnet_amd import dist as D
    from signnet_basisnet_amd import ops, optim, synth
    host = synth.make_batch(WORKLOAD["B"], seed=1236 + 1000 * rank)
    data = synth.batch_to(host, dev)
    model = build_model(dev).train()
    opt = optim.FlatAdam(model.parameters(), lr=1e-3, dist=dist)
    target = torch.randn(WORKLOAD["B"], WORKLOAD["n_out"], generator=torch.Generator().manual_seed(0)).to(dev)

    def step():
        opt.zero_grad()
        loss = (model(data) - target).abs().mean()
        loss.backward()
        opt.step()
        return loss
    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync_all()
    dt = D.max_over_ranks(time.perf_counter() - t0, dist, dev) / args.steps
    rec = ops.KernelTimer()
    with rec:                       # untimed per-kernel pass; every rank takes part (the step contains the all-reduce)
        for _ in range(3):
            step()
    kt = rec.summary()
    # the same step (fixed shape: this bench trains on one synthetic batch) captured once as a HIP graph and replayed: one graph launch
    # + the Adam launch per step instead of ~350 launches issued from Python (train_graph.GraphedStep).
    final_loss = float(loss.detach())
    del loss            # (a live loss keeps the eager step's autograd graph — and its default-stream AccumulateGrad nodes — alive: the
                        #  capture below would then have to synchronise with the default stream, which a capturing stream must not)
    graphed = None
    if not args.no_graph:
        # (with a process group: the replay per rank, then the flat gradient's all-reduce — all buckets, issued by step() — and Adam)
        from signnet_basisnet_amd.train_graph import GraphedStep
        gs = GraphedStep(model, opt, data, target)
        for _ in range(max(2, args.warmup // 2)):
            gs.step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            gloss = gs.step()
        sync_all()
        dtg = D.max_over_ranks(time.perf_counter() - t0, dist, dev) / args.steps
        model.check_train()
        graphed = {"value": WORKLOAD["B"] * world / dtg, "unit": "graphs/s", "ms_per_step": 1e3 * dtg, "final_loss": float(gloss),
                   "note": "forward + loss + backward replayed as one captured HIP graph" +
                           (" + one Adam launch (fixed batch shape)" if dist is None else
                            ", then the flat gradient's all-reduce (after the replay) + one Adam launch (fixed batch shape)")}
    rccl = rccl_allreduce_probe(dist, dev, opt.flat_g.numel()) if dist is not None else None     # collective: every rank
    if rank != 0:
        return
    per = {k: {"launches_per_step": v[0] / 3, "mean_us": 1e3 * v[1], "us_per_step": 1e3 * v[1] * v[0] / 3} for k, v in kt.items()}
    fl = algorithmic_flops(host, WORKLOAD["k"], WORKLOAD["hidden"], WORKLOAD["nl_signnet"], WORKLOAD["nl_rho"], WORKLOAD["nl_gnn"])
    out = {"device": device_block(dev) if rank == 0 else None,
           "metric": "graphs/sec SignNet+GINE training step (forward + backward + Adam), ZINC batch=128 k=16", "unit": "graphs/s",
           "value": WORKLOAD["B"] * world / dt, "ms_per_step": 1e3 * dt, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "higher_is_better": True, "scaling": "weak", "dtype": "f32", "data": "synthetic", "vs_baseline": None, "final_loss": final_loss,
           "config": {"workload": WORKLOAD["name"] + ", train step", "gflop_per_step": 3 * fl["total"] / 1e9},
           "roofline": train_roofline(fl["total"], dt),
           "distributed": {"world_size": world, "backend": dist.get_backend() if dist is not None else None,
                           "gradient_allreduce": rccl,
                           "note": "one SUM all-reduce of the flat gradient per step (optim.FlatAdam), 1/world folded into the Adam kernel"},
           "launches_per_step": sum(v["launches_per_step"] for v in per.values()),
           "kernels": dict(sorted(per.items(), key=lambda kv: -kv[1]["us_per_step"]))}
    if graphed is not None:
        out["eager"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "note": "the same step issued launch by launch from Python"}
        out["graphed"] = graphed
        out["value"], out["ms_per_step"] = graphed["value"], graphed["ms_per_step"]
        out["roofline"] = train_roofline(fl["total"], graphed["ms_per_step"] * 1e-3)
    if world == 1 and not args.no_cpu_baseline:
        # the float32 CPU oracle under torch.autograd + torch.optim.Adam: what the reference's training loop does on the host
        from oracle import pyg_signnet as O
        cfg = O.make_cfg("gine", None, None, WORKLOAD["hidden"], WORKLOAD["n_out"], WORKLOAD["nl_signnet"], WORKLOAD["nl_gnn"])
        sd = {k: (torch.nn.Parameter(v.detach().cpu().clone()) if v.is_floating_point() and "running" not in k else v.detach().cpu().clone())
              for k, v in model.state_dict().items()}
        oopt = torch.optim.Adam([v for v in sd.values() if isinstance(v, torch.nn.Parameter)], lr=1e-3)
        tcpu = target.cpu()
        ts = []
        t_end = time.perf_counter() + 20.0
        while len(ts) < 2 or (time.perf_counter() < t_end and len(ts) < 6):
            t0 = time.perf_counter()
            oopt.zero_grad()
            (O.signnet_gnn(sd, cfg, host, training=True, max_k=WORKLOAD["k"]) - tcpu).abs().mean().backward()
            oopt.step()
            ts.append(time.perf_counter() - t0)
        med = sorted(ts[1:])[len(ts[1:]) // 2]
        out["cpu_baseline"] = {"value": WORKLOAD["B"] / med, "unit": "graphs/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"{len(ts) - 1} training step(s) of the same batch after one warm-up, median; oracle/pyg_signnet.py "
                                         "under torch.autograd + torch.optim.Adam (CPU fp32)"}
    print(json.dumps(out))


def basisnet_bench(args, dev):
    """BASELINE configs[4] (extra measurement, `--config 4`): BasisNet on one 32x32 2-D grid graph (LearningFilters/training.py:
    47-73,119-126,205-222): the eigenspaces of the normalised Laplacian grouped by multiplicity, IGNBasisInv(hidden 32) over the
    stacked projectors, EqDeepSetsEncoder(2N -> 10 -> 10 -> 32).  A step = one forward of phi for every multiplicity + rho.
    The contraction kernel streams every projector element exactly once: its roofline is HBM."""
    import numpy as np
    from oracle import basisnet as OB
    from signnet_basisnet_amd import basisnet as BN
    from signnet_basisnet_amd import ops
    side = 32
    N = side * side
    idx = np.arange(N).reshape(side, side)
    A = np.zeros((N, N))
    for a, b in ((idx[:-1, :], idx[1:, :]), (idx[:, :-1], idx[:, 1:])):
        A[a.ravel(), b.ravel()] = 1
        A[b.ravel(), a.ravel()] = 1
    dis = 1.0 / np.sqrt(A.sum(1))
    L = np.eye(N) - dis[:, None] * A * dis[None, :]                       # utils.py:72-78 (fp64 eigh, then .float())
    w, V = np.linalg.eigh(L)
    eigvals, eigvecs = torch.from_numpy(w).float(), torch.from_numpy(V).float()
    ev_dev, val_dev = eigvecs.to(dev), eigvals.to(dev)
    # training.py:47-73 on the device, once per graph (not timed in the step): sn_eigenspace_group + sn_eigenspace_projectors_f32
    BN.group_eigenspaces(val_dev, ev_dev)                                  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    groups_dev, eplan = BN.group_eigenspaces(val_dev, ev_dev, return_plan=True)
    torch.cuda.synchronize()
    t_group = time.perf_counter() - t0
    mults = sorted(groups_dev)
    torch.manual_seed(0)
    phi = BN.IGNBasisInv(mults, 1, hidden_channels=32).to(dev).eval()
    rho = BN.EqDeepSetsEncoder(2 * N, hidden_channels=10, num_layers=3, out_channels=32, use_bn=True).to(dev).eval()
    evm = eigvals.to(dev).unsqueeze(0).repeat(N, 1)

    def step():
        outs = [phi(groups_dev[m], m) for m in mults]
        feats = torch.cat([o.reshape(N, -1) for o in outs] + [evm], dim=-1)       # training.py:119-123 (the caller's concat)
        return rho(feats)

    def step_from_eigvecs():      # extension: the 2->1 contractions from V alone (no 2.15 GB read), everything else identical
        outs = phi.forward_eigvecs(ev_dev, eplan)
        feats = torch.cat([outs[m].reshape(N, -1) for m in mults] + [evm], dim=-1)
        return rho(feats)
    with torch.no_grad():
        for _ in range(args.warmup):
            step_from_eigvecs()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y2 = step_from_eigvecs()
        torch.cuda.synchronize()
        dt_fast = (time.perf_counter() - t0) / args.steps
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        rec = ops.KernelTimer()
        with rec:
            for _ in range(min(args.steps, 5)):
                step()
        kt = rec.summary()
        # the same forward replayed as ONE captured HIP graph: this workload's graph (one 2-D grid) never changes shape
        dt_graph = None
        try:
            from signnet_basisnet_amd.train_graph import GraphedForward
            gf = GraphedForward(step)
            for _ in range(args.warmup):
                gf.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                yg = gf.replay()
            torch.cuda.synchronize()
            dt_graph = (time.perf_counter() - t0) / args.steps
            if not torch.equal(yg, y):
                raise RuntimeError("graph replay differs from the eager forward")
        except Exception as e:      # (reported, never silently: the eager numbers stand)
            dt_graph = None
            graph_error = repr(e)
    nrep = min(args.steps, 5)
    proj_bytes = 4.0 * sum(int(g.shape[0]) for g in groups_dev.values()) * N * N
    launches, mean_ms = kt["sn_ign_contract_2to1_f32"]
    per_step_ms = mean_ms * launches / nrep
    out = {"metric": "forwards/sec BasisNet (IGNBasisInv + DeepSets rho) on one 32x32 grid graph, BASELINE configs[4] (extra measurement)",
           "value": 1.0 / dt, "unit": "graphs/s", "ms_per_step": 1e3 * dt, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "higher_is_better": True, "dtype": "f32", "data": "synthetic", "vs_baseline": None,
           "graphed": ({"value": 1.0 / dt_graph, "ms_per_step": 1e3 * dt_graph,
                        "note": "the same forward (projector path) replayed as one captured HIP graph; bit-identical output"}
                       if dt_graph else {"error": graph_error}),
           "config": {"workload": "LearningFilters BasisNet, 2-D grid 32x32 (N = 1024), eigenspace multiplicities "
                                  + str({m: int(g.shape[0]) for m, g in groups_dev.items()}),
                      "projector_bytes": proj_bytes},
           "roofline": {"kernel": "sn_ign_contract_2to1_f32 (k_ign_rowcol + k_ign_finish, all multiplicities of a step)",
                        "bound": "hbm", "achieved": proj_bytes / (per_step_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": proj_bytes / (per_step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                        "bytes_per_step": proj_bytes, "ms_per_step": per_step_ms,
                        "note": "algorithmic bytes = every projector element read once (4*b*n*n)"},
           "kernels": {k: {"launches_per_step": v[0] / nrep, "mean_us": 1e3 * v[1]} for k, v in kt.items()}}
    out["preprocessing"] = {"what": "eigenspace grouping + projector stack on the device (training.py:47-73; once per graph, not in the step)",
                            "ms": 1e3 * t_group, "bytes_written": proj_bytes, "write_gbs": proj_bytes / t_group / 1e9}
    out["from_eigenvectors"] = {"value": 1.0 / dt_fast, "unit": "graphs/s", "ms_per_step": 1e3 * dt_fast,
                                "max_abs_diff_vs_projector_path": float((y2 - y).abs().max()), "output_scale": float(y.abs().max()),
                                "note": "IGNBasisInv.forward_eigvecs: contractions of P = V V^T computed from V (4*N*sum(mult) = "
                                        f"{4 * N * N} bytes instead of {int(proj_bytes)}); an extension, the reference API takes projectors"}
    # the training workload the reference runs on this graph (scripts/sign_basis_inv.sh): epochs of
    # training.py:132-150 — get_lap_feat (basis_inv) -> base net -> masked square loss -> backward -> Adam
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd.optim import Adam
    out["training"] = {"what": "one epoch = training.py:132-150 (forward of every IGN2to1 + rho + base net, loss, backward, Adam) on "
                               "the 32x32 grid; contractions of the constant projectors computed once (GridEigen)", "configs": {}}
    gen = torch.Generator().manual_seed(5)
    xs, ys = torch.randn(N, 1, generator=gen).to(dev), torch.randn(N, 1, generator=gen).to(dev)
    ms = torch.ones(N, 1, device=dev)
    for label, fa in (("DS h16 + basis_inv IGN", LF.FilterArgs(net="DS", hidden_channels=16, use_eig=True, lap_method="basis_inv")),
                      ("Transformer h12 + basis_inv IGN", LF.FilterArgs(net="Transformer", hidden_channels=12, use_eig=True,
                                                                         lap_method="basis_inv")),
                      ("DS h32 L3 + sign_inv DS", LF.FilterArgs(net="DS", hidden_channels=32, num_layers=3, use_eig=True,
                                                                 lap_method="sign_inv", sign_inv_net="DS"))):
        geig = LF.GridEigen(val_dev, ev_dev, fa)
        torch.manual_seed(0)
        fmodel = LF.gen_model(fa, geig, dev)
        fopt = Adam(fmodel.parameters(), lr=fa.lr)
        for _ in range(max(3, args.warmup // 4)):
            LF.train_step(fmodel, fopt, fa, geig, xs, ys, ms)
        torch.cuda.synchronize()
        nst = max(5, args.steps // 4)
        t0 = time.perf_counter()
        for _ in range(nst):
            floss, _ = LF.train_step(fmodel, fopt, fa, geig, xs, ys, ms)
        torch.cuda.synchronize()
        dte = (time.perf_counter() - t0) / nst
        # the same epoch captured once as a HIP graph and replayed (learning_filters.GraphedEpoch: fixed graph, fixed shapes, 2 000
        # epochs per image — one graph launch + one Adam launch per epoch; bit-identical losses, tests/test_learning_filters_gpu.py)
        from signnet_basisnet_amd.optim import FlatAdam
        torch.manual_seed(0)
        gmodel = LF.gen_model(fa, geig, dev)
        gepoch = LF.GraphedEpoch(gmodel, FlatAdam(gmodel.parameters(), lr=fa.lr), fa, geig, xs, ys, ms)
        for _ in range(5):
            gepoch.step()
        torch.cuda.synchronize()
        ng = max(20, args.steps)
        t0 = time.perf_counter()
        for _ in range(ng):
            gloss, _ = gepoch.step()
        torch.cuda.synchronize()
        dtg = (time.perf_counter() - t0) / ng
        out["training"]["configs"][label] = {"ms_per_epoch": 1e3 * dte, "epochs_per_s": 1.0 / dte, "loss_after": float(floss),
                                             "parameters": sum(p.numel() for p in fmodel.parameters()),
                                             "hip_graph": {"ms_per_epoch": 1e3 * dtg, "epochs_per_s": 1.0 / dtg, "loss_after": float(gloss)}}
    if not args.no_cpu_baseline:
        sdphi = [{k: v.detach().cpu() for k, v in phi.encs[phi.mult_to_idx[m]].state_dict().items()} for m in mults]
        eqs = [[(e.coeffs.detach().cpu(), e.bias.detach().cpu()) for e in phi.encs[phi.mult_to_idx[m]].equi_layers] for m in mults]
        small = {m: groups_dev[m][:min(4, groups_dev[m].shape[0])].cpu() for m in mults}        # bounded sample: <= 4 projectors per class
        nproj = sum(int(g.shape[0]) for g in small.values())
        t0 = time.perf_counter()
        with torch.no_grad():
            for m, sd_, eq in zip(mults, sdphi, eqs):
                OB.ign2to1(sd_, eq, small[m], training=False)
        tcpu = time.perf_counter() - t0
        total = sum(int(g.shape[0]) for g in groups_dev.values())
        out["cpu_baseline"] = {"value": 1.0 / (tcpu * total / nproj), "unit": "graphs/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"oracle/basisnet.py IGN2to1 on {nproj} of the {total} projectors (<= 4 per multiplicity), "
                                         "time scaled to all of them; rho not included"}
    print(json.dumps(out))


def dgl_bench(args, dev):
    """`--workload dgl` (extra measurement): the GraphPrediction tree's shipped GatedGCN_ZINC_LapPE_signinv_GIN.json model
    (GINDeepSigns sign_inv_net with 8 layers, k = 8, phi_out 4; GatedGCNNet L = 16, hidden 68, concat PE) in eval mode on a
    128-graph ZINC-like batch, driven as train_ZINC_graph_regression.py:20-25,77-80 does; plus the edge-gated aggregation
    kernel alone on an 8192-graph batch, where it is HBM-bound (gathers of Bh / Dh rows per edge)."""
    import numpy as np
    from oracle import dgl_deepsigns as OD
    from oracle import dgl_nets as ON
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import dgl_nets, ops, synth
    k, hidden, L = 8, 68, 16
    params = dict(num_atom_type=28, num_bond_type=4, hidden_dim=hidden, out_dim=hidden, in_feat_dropout=0.0, dropout=0.0, L=L,
                  readout="mean", batch_norm=True, residual=True, edge_feat=True, device=str(dev), pe_init="lap_pe",
                  lap_method="sign_inv", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, pos_enc_dim=k,
                  sign_inv_net="gin", sign_inv_layers=8, sign_inv_activation="relu", pe_aggregate="concat", phi_out_dim=4)
    torch.manual_seed(0)
    net = dgl_nets.GatedGCNNet(params)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)
    sd_cpu = {kk: v.detach().clone() for kk, v in net.state_dict().items()}
    net = net.to(dev).eval()
    host = synth.make_batch(128, seed=1236)
    pe = synth.dgl_pos_enc(host, k)
    ei = host.edge_index
    src_d, dst_d, bnn = ei[0].to(dev), ei[1].to(dev), torch.tensor(host.sizes)
    g = DS.Graph(src_d, dst_d, bnn)
    hx, ex, ped = host.x.squeeze(-1).to(dev), host.edge_attr.to(dev), pe.unsqueeze(-1).to(dev)

    def step():
        # a NEW graph object every step, as a data loader hands over: the per-graph plan (sn_batch_plan) and size limits that the
        # modules keep on the graph object are rebuilt inside the timed region
        g = DS.Graph(src_d, dst_d, bnn)
        p = net.sign_inv_net(g, ped).squeeze(-1)
        return net(g, hx, p, ex, None)[0]
    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = step()
        torch.cuda.synchronize()
        dt_seq = (time.perf_counter() - t0) / args.steps
        rec = ops.KernelTimer()
        with rec:
            for _ in range(3):
                step()
        kt = rec.summary()
        # `value`: the same loop with the sign-invariant net's overlap mode (dgl_deepsigns: plan + its two stage launches on a side stream
        # of the module, handed to the base network with an event kept on the graph object) — the next batch's positional encoding is
        # computed under this batch's GatedGCN stack.  Same call site, outputs bit-identical.
        net.sign_inv_net.overlap = True
        for _ in range(max(3, args.warmup)):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = step()
        if hasattr(net, "check_last"):
            net.check_last()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        net.sign_inv_net.overlap = False
        # the gather kernel alone, large batch
        reps = 8
        base = synth.make_batch(1024, seed=7)
        big_ei = torch.cat([base.edge_index + r * base.num_nodes for r in range(reps)], 1).to(dev)
        sizes = list(base.sizes) * reps
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
        plan = ops.build_plan(batch, big_ei, len(sizes), 0)
        Nn, E = plan.N, plan.E
        A_, B_, D_, E_ = (torch.randn(Nn, hidden, device=dev) for _ in range(4))
        Ce = torch.randn(E, hidden, device=dev)
        for _ in range(3):
            ops.gated_aggregate(A_, B_, D_, E_, Ce, plan)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.gated_aggregate(A_, B_, D_, E_, Ce, plan)
        e1.record()
        torch.cuda.synchronize()
        gms = e0.elapsed_time(e1) / 10
    gbytes = 4.0 * hidden * (3 * E + 4 * Nn)
    out = {"metric": "graphs/sec GINDeepSigns + GatedGCN eval forward (GatedGCN_ZINC_LapPE_signinv_GIN.json), ZINC batch=128 (extra measurement)",
           "value": 128 / dt, "unit": "graphs/s", "ms_per_step": 1e3 * dt, "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "higher_is_better": True, "dtype": "f32", "data": "synthetic", "vs_baseline": None,
           "config": {"workload": "DGL tree: sign_inv_net gin (8 layers, k=8) + GatedGCNNet (L=16, hidden 68, concat), batch 128",
                      "module_mode": "sign_inv_net.overlap = True (its launches on a side stream, event on the graph object)"},
           "sequential": {"value": 128 / dt_seq, "unit": "graphs/s", "ms_per_step": 1e3 * dt_seq,
                          "note": "overlap off: every launch of a step on one stream (rounds 1-2's `value`)"},
           "roofline": {"kernel": "sn_gated_aggregate_f32 (k_gated_fwd_v4) on an 8192-graph batch", "bound": "hbm",
                        "achieved": gbytes / (gms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": gbytes / (gms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None, "bytes_per_launch": gbytes,
                        "mean_launch_us": 1e3 * gms, "nodes": Nn, "edges": E,
                        "note": "algorithmic bytes 4*d*(3E + 4N): Ce in, e out, Bh and Dh gathered per edge; Ah, Eh in, h out (+den)"},
           "kernels": {kk: {"launches_per_step": v[0] / 3, "mean_us": 1e3 * v[1]} for kk, v in kt.items()}}
    # The other four shipped base networks run their eval forward layer by layer (50-130 launches: host-bound); for a fixed batch shape
    # the whole step is one HIP-graph launch (serving.GraphedDGLForward).  Extra blocks, not `value`: ms per 128-graph forward, eager
    # (a fresh graph object per step) and replayed.
    from signnet_basisnet_amd import dgl_configs
    from signnet_basisnet_amd.serving import GraphedDGLForward
    out["nets"] = {}
    sn = torch.cat([torch.full((n, 1), 1.0 / n) for n in host.sizes]).sqrt().to(dev)
    bne = torch.bincount(torch.bucketize(ei[1], torch.cumsum(torch.tensor(host.sizes), 0), right=True), minlength=len(host.sizes))
    for name in ("gin", "gat", "pna", "transformer", "gatedgcn"):
        cls, prm = dgl_configs.net_params(name, dev)
        torch.manual_seed(0)
        nt = getattr(dgl_nets, cls)(prm).to(dev).eval()
        kk_ = prm["pos_enc_dim"]
        pe_n = synth.dgl_pos_enc(host, kk_).unsqueeze(-1).to(dev)
        snn = sn if name == "pna" else None

        def step_n():
            gg = DS.Graph(src_d, dst_d, bnn, bne)
            pp = nt.sign_inv_net(gg, pe_n).squeeze(-1)
            return nt(gg, hx, pp, ex, snn)[0]
        with torch.no_grad():
            for _ in range(max(3, args.warmup)):
                step_n()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step_n()
            torch.cuda.synchronize()
            t_eager = (time.perf_counter() - t0) / args.steps
            rec_n = ops.KernelTimer()
            with rec_n:
                step_n()
            launches = sum(v[0] for v in rec_n.summary().values())
            gf = GraphedDGLForward(nt, DS.Graph(src_d, dst_d, bnn, bne), hx, pe_n, ex, snn)
            for _ in range(3):
                gf()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                gf()
            torch.cuda.synchronize()
            t_graph = (time.perf_counter() - t0) / args.steps
        out["nets"][name] = {"config": f"{cls} hidden {prm['hidden_dim']}, L = {prm['L']}, k = {kk_}, sign_inv_net gin (8 layers)",
                             "eager_ms": 1e3 * t_eager, "graphed_ms": 1e3 * t_graph, "c_abi_launches": int(launches),
                             "graphs_per_s_graphed": 128 / t_graph}
    if not args.no_cpu_baseline:
        ssd = {kk[len("sign_inv_net."):]: v for kk, v in sd_cpu.items() if kk.startswith("sign_inv_net.")}
        ts = []
        with torch.no_grad():
            for _ in range(4):
                t0 = time.perf_counter()
                po = OD.gin_deepsigns(ssd, ei[0], ei[1], pe.unsqueeze(-1), 8, k).squeeze(-1)
                ON.gatedgcn_net(sd_cpu, ei[0], ei[1], host.sizes, host.x.squeeze(-1), po, host.edge_attr, L, "concat")
                ts.append(time.perf_counter() - t0)
        med = sorted(ts[1:])[1]
        out["cpu_baseline"] = {"value": 128 / med, "unit": "graphs/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": "3 forwards of the same batch after a warm-up, median; oracle/dgl_deepsigns.py + oracle/dgl_nets.py (torch CPU fp32)"}
    print(json.dumps(out))


def scatter_measure(dev, graphs, feat, kind, steps=20, warmup=5, base=None):
    """One standalone aggregation launch (layer-at-a-time entry point) on `graphs` synthetic ZINC-like graphs, timed with HIP
    events on the launch stream.  kind 'gin': sn_gin_aggregate_f32 over the [N, feat] slot tensor (the reference's eigvec scatter:
    PyG GINConv over [K, N, d], masked_layers.py:75) — algorithmic bytes 8*feat*N + 4*(E+N+1): every feature row read once and
    written once, int32 CSR.  kind 'gine': sn_gine_aggregate_f32 over [N, feat] nodes and [E, feat] edge embeddings
    (pyg_gnn_wrapper.py:28) — 4*feat*(2N+E)."""
    from signnet_basisnet_amd import ops, synth
    if base is None:
        base = synth.make_batch(min(graphs, 1024), seed=5)
    reps = max(1, graphs // base.num_graphs)
    ei = torch.cat([base.edge_index + r * base.num_nodes for r in range(reps)], 1).to(dev)
    batch = torch.cat([base.batch + r * base.num_graphs for r in range(reps)]).to(dev)
    plan = ops.build_plan(batch, ei, base.num_graphs * reps, 16)
    N, E = plan.N, plan.E
    eps = torch.zeros(1, device=dev)
    if kind == "gin":
        x = torch.randn(N, feat, device=dev)
        f = lambda: ops.gin_aggregate(x, plan, eps)
        byt = 8 * feat * N + 4 * (E + N + 1)
        name = f"sn_gin_aggregate_f32 [N, K*d = {feat}]"
    else:
        x, ea = torch.randn(N, feat, device=dev), torch.randn(E, feat, device=dev)
        f = lambda: ops.gine_aggregate(x, ea, plan, eps)
        byt = 4 * feat * (2 * N + E)
        name = f"sn_gine_aggregate_f32 [N, d = {feat}]"
    for _ in range(warmup):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        f()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    traffic = None          # HBM bytes of this very launch from the committed PMC passes (profiles/hbm_traffic.json), if it is one of them
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "hbm_traffic.json")) as fh:
            traffic = json.load(fh)["scatter"]["launches"][str(byt)]["bytes"]
    except (OSError, KeyError, ValueError):
        pass
    return {"kernel": name, "graphs": base.num_graphs * reps, "nodes": N, "edges": E, "mean_launch_us": 1e3 * ms, "traffic": traffic,
            "algorithmic_bytes": byt, "working_set_mib": byt / 2 ** 20, "bound": "hbm", "achieved": byt / ms / 1e6, "unit": "GB/s",
            "peak": HBM_PEAK_GBS, "frac": byt / ms / 1e6 / HBM_PEAK_GBS}


def scatter_roofline(dev):
    """The north_star's second figure — HBM bandwidth of the eigenvector scatter against the chip peak (target >= 40 %) — measured
    in the same run as the headline, on working sets beyond the 256 MiB Infinity Cache: GIN over [N, K*d = 2048] on 1024 graphs
    (~390 MB) and GINE over [N, 128] + [E, 128] on 6144 graphs (~300 MB).  In the eval forward this aggregation happens inside LDS
    (fused phi / GINE stages) and has no HBM figure; these are the standalone entry points of the layer-at-a-time / training path."""
    from signnet_basisnet_amd import synth
    base = synth.make_batch(1024, seed=5)
    gin = scatter_measure(dev, 1024, 2048, "gin", base=base)
    gine = scatter_measure(dev, 6144, 128, "gine", base=base)
    return {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "achieved": gin["achieved"], "frac": gin["frac"],
            "traffic": gin["traffic"], "kernel": gin["kernel"], "target_frac": 0.40, "gin": gin, "gine": gine,
            "note": "achieved = algorithmic bytes / mean launch time (HIP events on the launch stream); working sets > 256 MiB so that "
                    "the Infinity Cache cannot serve them.  The headline forward does NOT launch this kernel: its eigenvector (GIN) aggregation "
                    "runs inside sn_phi_fused_f32 on an LDS image of the bin (no HBM traffic at all: the [rows, d] activations never leave the "
                    "CU between layers) and the GINE aggregation inside sn_gnn_fused_f32 likewise; this block times the standalone layer-path / "
                    "training kernels (sn_gin_aggregate_f32, sn_gine_aggregate_f32) that the north_star's HBM figure can be quoted on"}


def scatter_bench(args, dev):
    """`--workload scatter` (extra measurement): the standalone GIN / GINE aggregation entry points at several sizes."""
    res = {}
    for B in (128, 1024, 2048, 6144):
        for kind, feat in (("gin", 2048), ("gine", 128)):
            r = scatter_measure(dev, B, feat, kind, args.steps, args.warmup)
            res[f"{r['kernel']}, {r['graphs']} graphs"] = r
    best = res["sn_gin_aggregate_f32 [N, K*d = 2048], 2048 graphs"]
    print(json.dumps({"metric": "HBM roofline fraction of the standalone GIN / GINE aggregation (extra measurement)", "value": best["frac"],
                      "unit": "fraction of 8 TB/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
                      "dtype": "f32", "data": "synthetic", "vs_baseline": None,
                      "roofline": {"kernel": "sn_gin_aggregate_f32 (k_gin_gather), 2048 graphs", "bound": "hbm", "achieved": best["achieved"],
                                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": best["frac"], "traffic": None,
                                   "note": "algorithmic bytes 8*F*N + 4*(E+N+1): every feature row read once and written once, int32 CSR"},
                      "kernels": res}))


def rccl_allreduce_probe(dist, dev, numel, iters=20):
    """What the training variant's gradient exchange costs on this node: ONE fp32 SUM all-reduce of the model's flat gradient
    (optim.FlatAdam) over RCCL, device buffers, timed with HIP events after a warm-up (not part of the timed forward region)."""
    buf = torch.ones(numel, dtype=torch.float32, device=dev)
    for _ in range(3):
        dist.all_reduce(buf)
    torch.cuda.synchronize()
    dist.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        dist.all_reduce(buf)
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / iters
    w = dist.get_world_size()
    return {"world_size": w, "backend": dist.get_backend(), "allreduce_bytes": 4 * numel, "allreduce_us": us,
            "busbw_gbs": 4 * numel * 2 * (w - 1) / w / us / 1e3,
            "note": "one SUM all-reduce of the flat fp32 gradient buffer (all parameters of the model), ring bus bandwidth"}


def all_eigenvectors_block(dev, host, data, steps, warmup):
    """Extra pass (not `value`): the SAME batch and weights with `max_k=None` — every eigenvector of every graph (K = the largest
    graph of the batch), which is what the reference's own ZINC entry point computes (GINESignNetPyG/core/sign_net.py:99-120,
    core/transform.py:29-66) and what the drop-in binding runs (dropin/gine_pyg/core/sign_net.py).  One-stream loop, module in its
    throughput mode (strict=False), flags checked inside the timed region."""
    from signnet_basisnet_amd import ops
    wl = dict(WORKLOAD, k=None)
    model = build_model(dev, k=None)
    model.strict = False
    fl = algorithmic_flops(host, None, wl["hidden"], wl["nl_signnet"], wl["nl_rho"], wl["nl_gnn"])
    with torch.no_grad():
        for _ in range(max(warmup, 10)):
            model(data)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model(data)
        model.check_last()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec = ops.KernelTimer()
        n_ev = min(steps, 10)
        with rec:
            for _ in range(n_ev):
                model(data)
        torch.cuda.synchronize()
    kern = {}
    for name, (launches, mean_ms) in rec.summary().items():
        kern[name] = {"launches_per_step": launches / n_ev, "mean_us": 1e3 * mean_ms}
        f = ops.KERNEL_ROOFLINE.get(name)
        if f is not None and name != "sn_masked_linear_f32":
            r = f(fl, wl, host, mean_ms, launches / n_ev)
            kern[name].update(achieved_tflops=r["achieved"], frac=r["frac"])
    return {"value": steps * host.num_graphs / dt, "unit": "graphs/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
            "K": int(max(host.sizes)), "valid_rows": int(fl["M"]), "gflop_per_step": fl["total"] / 1e9, "kernels": kern,
            "note": "extra pass, not `value`: max_k=None (all eigenvectors, K = the batch's largest graph) on the headline batch and "
                    "weights; the reference's ZINC default (GINESignNetPyG/core/sign_net.py:99-120) and the drop-in binding's mode"}


def protocol_8d_block(model, data, num_graphs, warmup=20, timed=200):
    """SURVEY.md section 8(d) literally: 20 warm-up forwards, then 200 timed ones, the median of the per-step times.  A step is timed
    from the host: clock, forward, device synchronize, clock (what a caller who needs the result sees; the host wait per step is
    part of it, so this is slower than `value`, whose K steps are queued back to back).  The same loop with one HIP-event pair per
    step on the launch stream is reported beside it (`event_median_ms`: the device-side duration of the forward's four kernels)."""
    import statistics
    with torch.no_grad():
        for _ in range(warmup):
            model(data)
        torch.cuda.synchronize()
        ts = []
        for _ in range(timed):
            t0 = time.perf_counter()
            model(data)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        model.check_last()
        evs = []
        for _ in range(timed):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(data)
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        model.check_last()
    med = statistics.median(ts)
    emed = statistics.median(e0.elapsed_time(e1) for e0, e1 in evs)
    return {"warmup": warmup, "timed": timed, "median_ms": 1e3 * med, "value": num_graphs / med, "unit": "graphs/s",
            "event_median_ms": emed, "event_value": num_graphs / (emed * 1e-3),
            "note": "SURVEY 8(d): 20 warm-up + 200 timed forwards, median of per-step times; median_ms = host clock around forward + "
                    "synchronize (one step in flight at a time), event_median_ms = HIP events around each forward on the launch stream"}



def recorded_traffic(kernel):
    """HBM bytes per launch from the committed PMC pass of this same command (profiles/hbm_traffic.json; FETCH_SIZE and
    WRITE_SIZE need their own rocprofv3 passes, so they cannot be collected in the timed run).  None for another workload."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "hbm_traffic.json")
    try:
        with open(path) as f:
            rec = json.load(f)
        if rec["workload"] != WORKLOAD["name"]:
            return {"traffic": None}
        return {"traffic": rec["kernels"][kernel]["bytes"], "traffic_unit": "bytes/launch", "traffic_kind": "recorded",
                "traffic_source": rec["source"] + " (separate rocprofv3 --pmc passes; 2 x FETCH_SIZE + WRITE_SIZE; RECORDED at commit "
                                  + str(rec.get("commit")) + " on " + str(rec.get("date")) + ", not measured in this run)"}
    except (OSError, KeyError, ValueError):
        return {"traffic": None}


def relaunch_under_torchrun(n):
    """`python bench.py --gpus N` without a launcher: run this command line again as a child process
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py ...`
    (one rank per GPU over RCCL, the launch the driver uses) and exit with its status; does not return.  A fresh child rather than
    an exec: this process has already opened the GPU (device_count)."""
    import socket
    have = torch.cuda.device_count()
    if have < n and os.environ.get("SN_BENCH_SHARE_DEVICE", "0") != "1":
        raise SystemExit(f"--gpus {n}: this node has {have} visible GPU(s)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    sys.stderr.flush()
    import subprocess
    raise SystemExit(subprocess.call(cmd))


def dump_outputs(outdir, arrays, limit_bytes=64 << 20):
    """--dump-outputs DIR: every array as DIR/<name>.npy in float32 (float64 stays float64), at most `limit_bytes` in all; a larger
    array is replaced by a fixed sample (seeded, the same entries from run to run) and its shape is recorded in DIR/<name>.shape.json."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        a = t.detach().cpu()
        a = (a.double() if a.dtype == torch.float64 else a.float()).contiguous().numpy()
        budget = max(0, limit_bytes - total) // a.itemsize
        if a.size > budget:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=budget, replace=False))
            with open(os.path.join(outdir, name + ".shape.json"), "w") as f:
                json.dump({"shape": list(a.shape), "sampled_flat_indices_seed": 0, "sampled": int(budget)}, f)
            a = a.reshape(-1)[idx]
        np.save(os.path.join(outdir, name + ".npy"), a)
        total += a.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="forward bench: also run every extra measurement and check (cold pass, HIP-event roofline, per-kernel table, overlap / "
                         "strict / layer-path / sustained / pipelined passes, SURVEY 8(d) protocol, all-eigenvector block, device clock probe, "
                         "CPU baseline, scatter roofline, all-reduce probe).  Off: set up, warm up, time the K steps, print the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="forward bench: after the timed steps write what the last timed step computed (the predictions y a caller of "
                         "model(data) receives) as DIR/y.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--config", type=int, default=1, choices=[0, 1, 2, 4],
                    help="BASELINE.json configs index: 1 = the headline (default); 0 / 2 / 4 = extra measurements of the other "
                         "single-GPU configs (4 = BasisNet on the 2-D grid)")
    ap.add_argument("--workload", default="forward", choices=["forward", "evd", "train", "dgl", "scatter"],
                    help="forward = the headline metric (default); evd = the eigendecomposition pre-transform, train = a full training step (secondary)")
    ap.add_argument("--streams", type=int, default=3, help="streams of the extra pipelined pass (1 = skip it)")
    ap.add_argument("--no-graph", action="store_true", help="--workload train: skip the captured-HIP-graph replay of the step")
    ap.add_argument("--no-overlap", action="store_true", help="forward bench: skip the extra pass in the module's overlap mode (`overlap_mode` block)")
    ap.add_argument("--no-kernel-events", action="store_true", help="skip the per-kernel HIP events (no roofline block)")
    ap.add_argument("--all-eigenvectors", action="store_true",
                    help="forward bench, extra measurement (not the headline): the main loop itself with max_k=None — every eigenvector, K = the "
                         "batch's largest graph (what the `all_eigenvectors` block of the default line times; this flag is for profiler passes)")
    ap.add_argument("--no-extras", action="store_true", help="forward bench: skip the `all_eigenvectors` and `protocol_8d` extra passes")
    ap.add_argument("--no-scatter", action="store_true", help="skip the scatter_roofline block (standalone GIN / GINE aggregation on > 256 MiB)")
    ap.add_argument("--clock-ramp-ms", type=float, default=60.0,
                    help="forward bench: after the W warm-up steps keep issuing untimed forwards until this much wall time has passed since "
                         "the first one (the GPU reaches its sustained clock; 0 = off).  Reported as `clock_ramp` in the JSON line")
    ap.add_argument("--sustained-ms", type=float, default=None,
                    help="forward bench, one GPU: extra pass — the `value` loop kept running for this much wall time (`sustained` block; 0 = off; "
                         "default 1500, or 0 with --no-cpu-baseline: the profiling / A-B command lines stay short)")
    ap.add_argument("--overlap-warmup", type=int, default=32,
                    help="forward bench: untimed forwards in the module's overlap mode before the K timed steps of the `overlap_mode` extra pass "
                         "(the caching allocator needs a pipeline depth of forwards before it stops asking the driver for memory)")
    ap.add_argument("--event-stride", type=int, default=0,
                    help="inside the timed region, bracket every n-th launch of the dominant kernel with HIP events (1 = all; 0 = "
                         "automatic: max(4, steps // 12), i.e. about a dozen brackets over the timed steps and never more than one launch in four — a bracket is two marker packets that idle the stream "
                         "for ~5 us, i.e. 10-15 us per step at stride 1: 0.277-0.284 ms instead of 0.266-0.267 ms without any)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.dump_outputs and (args.workload != "forward" or args.config == 4):
        raise SystemExit("--dump-outputs: only the forward bench (--workload forward, --config 0 / 1 / 2) writes its outputs")

    global WORKLOAD
    if args.config == 4:
        if int(os.environ.get("RANK", "0")) == 0:
            torch.cuda.set_device(0)
            basisnet_bench(args, torch.device("cuda", 0))
        return
    WORKLOAD = WORKLOADS[args.config]
    if args.all_eigenvectors:
        WORKLOAD = dict(WORKLOAD, k=None, name=WORKLOAD["name"] + " with max_k=None (all eigenvectors; extra measurement)")
        args.no_extras = True
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args.gpus)       # plain `python bench.py --gpus N`: one rank per GPU, never returns
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}")
    from signnet_basisnet_amd import dist as D
    from signnet_basisnet_amd import ops, synth
    # (test hooks, never set by the driver: SN_BENCH_BACKEND=gloo + SN_BENCH_SHARE_DEVICE=1 run the N > 1 code path — barriers, the
    #  max-over-ranks time, the all-reduce probe, rank 0's JSON line — with every rank on cuda:0 of a one-GPU box, where RCCL refuses
    #  two ranks on one device: tests/test_bench_multirank_gpu.py)
    backend = os.environ.get("SN_BENCH_BACKEND", "nccl")
    if os.environ.get("SN_BENCH_SHARE_DEVICE", "0") == "1":
        local = 0
        os.environ["LOCAL_RANK"] = "0"
    dist = D.init_process_group(backend) if world > 1 else None      # "nccl" is RCCL on ROCm
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    if args.workload == "train":
        train_bench(args, dev, dist, rank, world)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.workload in ("evd", "dgl", "scatter"):
        if rank == 0:
            {"evd": evd_bench, "dgl": dgl_bench, "scatter": scatter_bench}[args.workload](args, dev)
        if dist is not None:
            dist.destroy_process_group()
        return

    # ONE global batch of B x world graphs (BASELINE configs[3]: 1024 graphs over 8 GPUs), the same on every rank (same seed), cut into
    # contiguous graph ranges by signnet_basisnet_amd.dist.shard_batch: by graph count when the slot count is fixed (every graph costs
    # about the same), by (node, slot) rows in the all-eigenvector mode (max_k=None: a graph's work grows with n^2).  No data-path
    # collective: a rank never sees another rank's graphs.
    if world > 1:
        glob = synth.make_batch(WORKLOAD["B"] * world, seed=1234 + 2, n_lo=WORKLOAD["n_lo"], n_hi=WORKLOAD["n_hi"], features=WORKLOAD["features"])
        host = D.shard_batch(glob, rank, world, balance="count" if WORKLOAD["k"] else "rows", max_k=WORKLOAD["k"])
    else:
        host = synth.make_batch(WORKLOAD["B"], seed=1234 + 2, n_lo=WORKLOAD["n_lo"], n_hi=WORKLOAD["n_hi"], features=WORKLOAD["features"])
    # which device every rank runs on (an N-rank line is then self-evidently N ranks on N devices)
    dev_names = None
    if dist is not None:
        props = torch.cuda.get_device_properties(dev)
        mine = f"rank {rank}: cuda:{local} {props.name} [{getattr(props, 'uuid', '')}]"
        dev_names = [None] * world
        dist.all_gather_object(dev_names, mine)
    data = synth.batch_to(host, dev)
    model = build_model(dev)
    # the throughput / serving mode of the module: no host wait per forward.  The device flags of EVERY forward are still posted
    # and are checked before the clock stops (model.check_last() inside the timed region); the module's default (strict: one host
    # wait per forward, oversize batches re-run layer by layer) is measured as an extra pass below (`strict_mode`)
    model.strict = False
    fl = algorithmic_flops(host, WORKLOAD["k"], WORKLOAD["hidden"], WORKLOAD["nl_signnet"], WORKLOAD["nl_rho"], WORKLOAD["nl_gnn"])

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    ramp_steps = 0
    dt_cold = dt_ovl = dt_strict = dt_layer = dt_pipe = None
    rec = None
    with torch.no_grad():
        t_ramp = time.perf_counter()
        for i in range(args.warmup):
            model(data)
            if i == 0:                       # (the first forward packs the weights and loads the code objects: not GPU work)
                torch.cuda.synchronize()
                t_ramp = time.perf_counter()
        if args.full:
            # (0) COLD pass (reported as `cold`, not `value`): exactly the K steps a `--warmup W --steps K` command line describes, right
            #     behind the W warm-up forwards and nothing else — the number a reader gets who takes the two flags at their word.  An idle
            #     MI355X needs tens of milliseconds of continuous work to reach its sustained clock and W = 5 forwards are 1.4 ms of it.
            sync_all()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                model(data)
            model.check_last()
            sync_all()
            dt_cold = time.perf_counter() - t0
        # clock ramp (untimed, reported in the line as `clock_ramp`): measured on one box, same command: phi 137-141 us and 0.290 ms per
        # sequential step behind --warmup 5, 120-126 us and 0.266 ms behind --warmup 200 (= a loop that has been running for 50 ms,
        # which is what a training / evaluation epoch is).  So more untimed forwards follow until --clock-ramp-ms of wall time have passed
        # since the end of the first forward (with --full the cold pass counts); the timed region is exactly K steps.
        if args.clock_ramp_ms > 0:
            torch.cuda.synchronize()
            while (time.perf_counter() - t_ramp) * 1e3 < args.clock_ramp_ms:
                for _ in range(8):
                    model(data)
                ramp_steps += 8
                torch.cuda.synchronize()
        # timed region, --full only: HIP events around the dominant kernel, on the launch stream, every --event-stride-th step (the
        # `roofline` block; a bracket = two marker packets, each idling the stream for ~5 us: measured 0.277-0.284 / 0.270 / 0.266-0.267
        # ms per step at stride 1 / 4 / no events on the same box.  Default: about a dozen brackets over the timed steps, at least one in
        # eight).  A plain run takes no events.
        if args.full:
            if args.event_stride <= 0:
                args.event_stride = max(4, args.steps // 12)        # never every launch by default: a 20-step driver run is not taxed
            rec = ops.KernelTimer(only=["__none__"] if args.no_kernel_events else [DOMINANT], stride=args.event_stride)
        # (1) `value`: a plain `for: model(data)` loop at one call site, every kernel of a forward on the caller's stream, one after
        #     the other — the definition of rounds 1-2 (round 3 reported the module's opt-in overlap mode here; it is the `overlap_mode`
        #     block now).  With --full the dominant kernel's HIP events are taken here: alone on the chip its duration is attributable.
        sync_all()
        t0 = time.perf_counter()
        with rec if rec is not None else contextlib.nullcontext():
            for _ in range(args.steps):
                y = model(data)
            model.check_last()               # every forward's status flags read and clean before the clock stops
        sync_all()
        dt = time.perf_counter() - t0
        y_last = y.float().cpu() if args.dump_outputs else None     # (before any extra pass of --full runs the model again)
        if args.full:
            # (2) extra pass (`overlap_mode`, not `value`): the same loop with the module's opt-in overlap mode (pyg.SignNetGNN.overlap_front):
            #     a forward is a three-stage pipeline — batch plan + phi on side stream A, rho on side stream B, the GINE stage on the caller's
            #     stream, chained by events — so the stages of consecutive steps share the GPU.  Outputs are bit-identical and ordered on the
            #     caller's stream; the batch is resident (the mode's precondition).
            # (small batches — configs[0], 32 graphs — are bound by the host's ~0.1 ms of stream / event calls per overlapped forward: the
            #  mode is measured from 64 graphs per GPU on)
            overlap = not args.no_overlap and WORKLOAD["B"] >= 64
            dt_ovl = None
            if overlap:
                model.overlap_front = True
                for _ in range(args.overlap_warmup):        # untimed: the mode's side streams, events and per-forward buffers reach their steady state
                    model(data)
                sync_all()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    model(data)
                model.check_last()
                sync_all()
                dt_ovl = time.perf_counter() - t0
                model.overlap_front = False
            # extra pass (not `value`): the module's DEFAULT mode, strict = True (the flags are waited for after every forward)
            model.strict = True
            for _ in range(3):
                model(data)
            sync_all()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                model(data)
            sync_all()
            dt_strict = time.perf_counter() - t0
            model.strict = False
            # extra pass (not `value`): the LAYER-AT-A-TIME path (model.use_fused = False) — what serves a batch beyond the stage kernels'
            # limits (a graph of > 64 nodes or > 192 in-edges, d > 128, ...: the reference has no such limits, Alchemy/sign_net/sign_net.py:
            # 96-118), one launch per op on the same batch
            dt_layer = None
            if not args.no_extras:
                model.use_fused, model._prep = False, None
                for _ in range(3):
                    model(data)
                sync_all()
                n_layer = max(3, min(args.steps, 10))
                t0 = time.perf_counter()
                for _ in range(n_layer):
                    model(data)
                sync_all()
                dt_layer = (time.perf_counter() - t0) / n_layer
                model.use_fused, model._prep = True, None
                for _ in range(3):
                    model(data)
                sync_all()
            # extra pass (not `value`): the one-stream loop kept running for --sustained-ms of wall clock, in chunks of 200 forwards with one
            # host wait each — the rate the part settles at (clocks, temperature) rather than that of a 25 ms window, and seconds of GPU
            # activity for an outside utilisation sampler to see
            sustained = None
            if args.sustained_ms is None:
                # >= 6 s: an outside utilisation sampler with 5 s spacing lands in it at least once (`gpu_busy` of the driver's record read 0
                # for three rounds: the longest busy window of a run was 1.5 s)
                args.sustained_ms = 0.0 if args.no_cpu_baseline else 6500.0
            if args.sustained_ms > 0 and world == 1:
                chunk, rates, n_fw = 200, [], 0
                sync_all()
                t_s = time.perf_counter()
                while (time.perf_counter() - t_s) * 1e3 < args.sustained_ms:
                    t_c = time.perf_counter()
                    for _ in range(chunk):
                        model(data)
                    torch.cuda.synchronize()
                    rates.append(chunk * host.num_graphs / (time.perf_counter() - t_c))
                    n_fw += chunk
                dt_s = time.perf_counter() - t_s
                sustained = {"value": n_fw * host.num_graphs / dt_s, "unit": "graphs/s", "ms_per_step": 1e3 * dt_s / n_fw, "forwards": n_fw,
                             "wall_ms": 1e3 * dt_s, "chunk_forwards": chunk, "chunk_min": min(rates), "chunk_max": max(rates),
                             "note": "the `value` loop kept running for --sustained-ms (one host wait per 200 forwards); not `value`"}
            # extra pass (not `value`): the same K steps issued round-robin on S HIP streams, so that independent batches
            # overlap on the device the way a serving loop would run them (fills the tails of one step's kernels with the
            # next step's work).  Same barrier + synchronize bracket, max over ranks.
            dt_pipe = None
            if args.streams > 1:
                streams = [torch.cuda.Stream(device=dev) for _ in range(args.streams)]
                for i in range(2 * args.streams):
                    with torch.cuda.stream(streams[i % args.streams]):
                        model(data)
                sync_all()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    with torch.cuda.stream(streams[i % args.streams]):
                        model(data)
                sync_all()
                dt_pipe = time.perf_counter() - t0
            # extra pass (not `value`): SURVEY 8(d)'s literal protocol (20 warm-up + 200 timed, median), one GPU
            proto = protocol_8d_block(model, data, host.num_graphs) if (world == 1 and args.config == 1 and not args.no_extras) else None
            # untimed extra pass: events around every launch, for the per-kernel table
            rec_all = ops.KernelTimer()
            with rec_all:
                for _ in range(min(args.steps, 20)):
                    model(data)
            torch.cuda.synchronize()
    dt_ranks = D.all_ranks(dt, dist, dev)          # every rank's own clock over the K timed steps (the line's time is their maximum)
    graphs_ranks = [int(v) for v in D.all_ranks(float(host.num_graphs), dist, dev)]
    dt = D.max_over_ranks(dt, dist, dev)
    if args.dump_outputs:
        # what the timed path computed in its last step: the [graphs, n_out] predictions a caller of model(data) receives, every rank's
        # shard in rank order (= graph order of the global batch)
        ys = [y_last]
        if dist is not None:
            ys = [None] * world
            dist.all_gather_object(ys, y_last)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"y": torch.cat(ys, 0)})
    if args.full:
        dt_cold = D.max_over_ranks(dt_cold, dist, dev)
        if dt_ovl is not None:
            dt_ovl = D.max_over_ranks(dt_ovl, dist, dev)
        dt_strict = D.max_over_ranks(dt_strict, dist, dev)
        if dt_pipe is not None:
            dt_pipe = D.max_over_ranks(dt_pipe, dist, dev)

    if rank == 0:
        total_graphs = sum(graphs_ranks) * args.steps
        out = {
            "metric": "graphs/sec SignNet+GINE forward, ZINC batch=128 k=16" if (args.config == 1 and not args.all_eigenvectors) else
                      "graphs/sec SignNet+GINE forward, ZINC batch=128, all eigenvectors (extra measurement, not the headline)" if args.all_eigenvectors else
                      f"graphs/sec SignNet+GINE forward, BASELINE configs[{args.config}] (extra measurement, not the headline)",
            "value": total_graphs / dt, "unit": "graphs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "arithmetic": "fp32 in / fp32 out / fp32 accumulate; every [d,d] Linear of phi, rho and GINE: operands split exactly into "
                          "3 bf16 pieces, 6 partial products on the bf16 matrix pipe (error <= 2^-23 |x||w| per product); "
                          "attention scores and P.V: fp32-input MFMA",
            "config": {"workload": WORKLOAD["name"], "graphs_per_gpu": WORKLOAD["B"], "global_batch": WORKLOAD["B"] * world,
                       "nodes": int(fl["N"]), "valid_rows": int(fl["M"]), "parallelism": f"graph-sharded dp{world}, no collective",
                       "gflop_per_step": fl["total"] / 1e9,
                       "module_mode": "strict=False (no host wait per forward; every forward's device flags checked inside the timed region); "
                                      "overlap_front=False: a forward's kernels one after the other on the caller's stream"},
            "value_definition": "K forwards of a plain `for: model(data)` loop at one call site, one stream, between barrier + synchronize "
                                "(rounds 1-2's definition; round 3's `value` was the opt-in overlap mode, now the `overlap_mode` block of --full)",
            "warmup_effective": args.warmup + (args.steps if args.full else 0) + ramp_steps,
            "clock_ramp": {"ms": args.clock_ramp_ms, "extra_untimed_steps": ramp_steps,
                           "note": "untimed forwards issued after the warm-up (and, with --full, the cold pass) until `ms` of wall time had passed "
                                   "since the first forward, so that the timed K steps of `value` run at the sustained clock (an idle GPU needs "
                                   "tens of ms of work to reach it; --clock-ramp-ms 0 switches this off)"},
            "full": args.full,
        }
        if args.full:
            dom_times = rec.summary()                    # {kernel: (launches, mean_ms)} — measured inside the timed region
            roof = None
            if DOMINANT in dom_times:
                launches, mean_ms = dom_times[DOMINANT]
                roof = ops.KERNEL_ROOFLINE[DOMINANT](fl, WORKLOAD, host, mean_ms, 1.0)      # one launch per step
                roof.update({"timed_launches": launches, "event_stride": args.event_stride, "timed_pass": "sequential"})
                roof["frac_vs_f32_mfma"] = roof["achieved"] / MFMA_F32_PEAK_TF      # the same rate against the fp32-input MFMA peak (157.3)
                roof.update(recorded_traffic(DOMINANT))
            ktimes = rec_all.summary()
            nall = min(args.steps, 20)
            all_roofs = {}
            for name, (launches, mean_ms) in ktimes.items():
                f = ops.KERNEL_ROOFLINE.get(name)
                if f is not None:
                    r = f(fl, WORKLOAD, host, mean_ms, launches / nall)
                    all_roofs[name] = {"achieved_tflops": r["achieved"], "frac": r["frac"]}
            out.update({
                "cold": {"value": total_graphs / dt_cold, "unit": "graphs/s", "ms_per_step": 1e3 * dt_cold / args.steps, "untimed_forwards_before": args.warmup,
                         "note": "the same K-step loop timed right behind the W warm-up forwards and nothing else (no clock ramp): what `--warmup W "
                                 "--steps K` says literally; `value` is measured after this pass and the clock ramp (`warmup_effective` untimed forwards)"},
                "sequential": {"value": total_graphs / dt, "unit": "graphs/s", "ms_per_step": 1e3 * dt / args.steps,
                               "note": "identical to `value` since round 4 (kept so that the block rounds 1-3 printed stays comparable)"},
                "overlap_mode": None if dt_ovl is None else {
                    "value": total_graphs / dt_ovl, "unit": "graphs/s", "ms_per_step": 1e3 * dt_ovl / args.steps, "untimed_forwards_before": args.overlap_warmup,
                    "note": "extra pass, not `value`: model.overlap_front = True (opt-in): a forward = plan + phi on side stream A -> rho on side "
                            "stream B -> GINE on the caller's stream, chained by events; consecutive forwards of the one call site overlap; "
                            "bit-identical outputs (round 3's `value`)"},
                "sustained": sustained,
                "device": device_block(dev),
                "strict_mode": {"value": total_graphs / dt_strict, "unit": "graphs/s", "ms_per_step": 1e3 * dt_strict / args.steps,
                                "note": "the module's default: flags waited for after every forward (one host round trip per step); extra pass, not `value`"},
                "layer_path": None if dt_layer is None else {
                    "value": sum(graphs_ranks) / dt_layer, "unit": "graphs/s", "ms_per_step": 1e3 * dt_layer,
                    "note": "extra pass, not `value`: model.use_fused = False — every op its own launch (sn_masked_linear_f32, sn_gin_aggregate_f32, "
                            "sn_set_attention_f32, ...): the path a batch takes that the whole-stage kernels cannot hold (a graph of > 64 nodes or "
                            "> 192 in-edges, hidden width > 128); the default mode routes such a batch here by itself"},
                "protocol_8d": proto,
                "roofline": roof,
                "kernels": {k: {"launches_per_step": v[0] / nall, "mean_us": 1e3 * v[1], **all_roofs.get(k, {}), **KERNEL_BOUND_NOTES.get(k, {})}
                            for k, v in ktimes.items()},
            })
            if world == 1 and args.config == 1 and not args.no_extras:
                out["all_eigenvectors"] = all_eigenvectors_block(dev, host, data, args.steps, args.warmup)
            if dt_pipe is not None:
                out["pipelined"] = {"streams": args.streams, "value": total_graphs / dt_pipe, "unit": "graphs/s",
                                    "ms_per_step": 1e3 * dt_pipe / args.steps,
                                    "note": "same K steps round-robin on S streams (independent batches overlap); not the headline value"}
            if world == 1 and not args.no_cpu_baseline:
                sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
                out["cpu_baseline"] = cpu_baseline(host, sd)
                out["vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    # (outside the timed region, --full) every rank takes part in the RCCL probe; rank 0 measures the scatter roofline
    rccl = None
    if dist is not None and args.full:
        rccl = rccl_allreduce_probe(dist, dev, sum(p.numel() for p in model.parameters()))
    if rank == 0:
        out["distributed"] = {"world_size": world, "backend": (f"{backend} (RCCL)" if backend == "nccl" else backend) if dist is not None else None,
                              "ranks_seen_by_backend": dist.get_world_size() if dist is not None else 1,
                              "devices": sorted(set(dev_names)) if dev_names else None,
                              "per_rank_ms_per_step": [1e3 * t / args.steps for t in dt_ranks],
                              "graphs_per_rank": graphs_ranks,
                              "data_path_collectives": 0, "gradient_allreduce": rccl,
                              "allreduce_us": None if rccl is None else rccl["allreduce_us"]}
        if args.full and args.config == 1 and not args.no_scatter:
            out["scatter_roofline"] = scatter_roofline(dev)
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
