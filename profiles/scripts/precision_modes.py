"""Time and accuracy of the three matmul-precision modes of the fused eval forward -> profiles/precision_modes.json.

    python profiles/scripts/precision_modes.py [--rounds 5] [--forwards 200] [--out profiles/precision_modes.json]
    python profiles/scripts/precision_modes.py --trace-config headline      # the program of a `rocprofv3 --kernel-trace --stats` run
    python profiles/scripts/precision_modes.py --merge-stats headline=<kernel_stats.csv> ...   # the profiler's per-kernel table -> the JSON

One process, every shape warmed up, the three modes ALTERNATING in rounds (a round = `--forwards` forwards per mode between two device
events), a device synchronise at the end; median and min-max of the per-round means per mode.  Configurations (bench.py's WORKLOADS):
the headline (128 ZINC-like graphs, k = 16, hidden 128), the same with all eigenvectors, BASELINE configs[2] (Alchemy, batch 256).
Accuracy: max|y - f64| / max|f64| against the float64 oracle on a 32-graph sub-batch, per mode.  Per-kernel phi / rho times are NOT
taken here: they come from a separate profiler run of `--trace-config` (which only replays forwards, mode by mode, untimed).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = ("highest", "high", "medium")
CONFIGS = {
    "headline": dict(variant="gine", ctor=(None, None, 128, 1, 4, 6), max_k=16, batch=dict(num_graphs=128, seed=1236)),
    "headline_all_eigenvectors": dict(variant="gine", ctor=(None, None, 128, 1, 4, 6), max_k=None, batch=dict(num_graphs=128, seed=1236)),
    "alchemy_b256": dict(variant="alchemy", ctor=(6, 4, 108, 12, 8, 16), max_k=None,
                         batch=dict(num_graphs=256, seed=1236, n_lo=6, n_hi=14, features="alchemy")),
}


def build(cfg, dev):
    import parity_util as PU
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    model = SignNetGNN(*cfg["ctor"], variant=cfg["variant"], max_k=cfg["max_k"])
    PU.bn_randomize(model, 1)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    host = synth.make_batch(**cfg["batch"])
    model = model.to(dev).eval()
    model.strict = False            # the serving mode bench.py measures: no host wait per forward
    return model, sd, host, synth.batch_to(host, dev)


def accuracy(cfg, model, sd, host, dev):
    """e_gpu per mode on the first 32 graphs of the batch, against the float64 oracle (and the fp32 oracle's own distance)."""
    import parity_util as PU
    from oracle import pyg_signnet as O
    from signnet_basisnet_amd import dist as D
    from signnet_basisnet_amd import synth
    sub = D.slice_graphs(host, 0, 32)
    ocfg = O.make_cfg(cfg["variant"], *cfg["ctor"])
    with torch.no_grad():
        y64 = O.signnet_gnn(PU.to_f64(sd), ocfg, PU.data_f64(sub), training=False, max_k=cfg["max_k"])
        y32 = O.signnet_gnn(sd, ocfg, sub, training=False, max_k=cfg["max_k"])
    out = {"fp32_oracle": PU.relerr(y32, y64)}
    dd = synth.batch_to(sub, dev)
    for mode in MODES:
        model.matmul_precision = mode
        with torch.no_grad():
            out[mode] = PU.relerr(model(dd), y64)
        model.check_last()
    model.matmul_precision = "highest"
    return out


def timed(model, dd, rounds, forwards):
    per = {m: [] for m in MODES}
    with torch.no_grad():
        for mode in MODES:              # warm-up: every mode, this shape
            model.matmul_precision = mode
            for _ in range(20):
                model(dd)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for mode in MODES:
                model.matmul_precision = mode
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(forwards):
                    model(dd)
                b.record()
                b.synchronize()
                per[mode].append(1e3 * a.elapsed_time(b) / forwards)       # us per forward
        torch.cuda.synchronize()
    model.check_last()
    model.matmul_precision = "highest"
    return {m: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), rounds_us=v) for m, v in per.items()}


def merge_stats(out, pairs):
    """Per-mode phi / rho kernel times of a profiler run (rocprofv3 --kernel-trace --stats --output-format csv) into the JSON."""
    import csv
    import re
    with open(out) as f:
        res = json.load(f)
    for pair in pairs:
        cfg, path = pair.split("=", 1)
        kern = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                m = re.match(r"void sn::(k_phi_fused|k_rho_fused|k_rho_wide)<(.*), (\d)>\(", r["Name"])
                if m:
                    kern.setdefault(MODES[int(m.group(3))], {})["phi" if m.group(1) == "k_phi_fused" else "rho"] = dict(
                        kernel=f"{m.group(1)}<{m.group(2)}>", calls=int(r["Calls"]), mean_us=float(r["AverageNs"]) / 1e3,
                        min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
        res["configs"][cfg]["kernel_trace"] = kern
    res["kernel_trace_note"] = ("separate rocprofv3 --kernel-trace --stats runs of `precision_modes.py --trace-config <config>` (50 forwards "
                                "per mode, highest first: its mean includes the process's first launches, see min_us)")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forwards", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precision_modes.json"))
    ap.add_argument("--trace-config", choices=list(CONFIGS), help="only replay 50 forwards per mode of this configuration (profiler run)")
    ap.add_argument("--skip-accuracy", action="store_true")
    ap.add_argument("--commit", help="commit id to record (default: git rev-parse HEAD of this tree)")
    ap.add_argument("--merge-stats", nargs="+", metavar="CONFIG=CSV", help="add per-kernel times of profiler runs to --out (no GPU needed)")
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.out, args.merge_stats)
        return
    if args.rounds < 5 or args.forwards < 200:
        ap.error("at least 5 rounds of at least 200 forwards per mode")
    dev = torch.device("cuda:0")
    if args.trace_config:
        model, _, _, dd = build(CONFIGS[args.trace_config], dev)
        with torch.no_grad():
            for mode in MODES:
                model.matmul_precision = mode
                for _ in range(50):
                    model(dd)
                torch.cuda.synchronize()
        model.check_last()
        return
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "forwards_per_round": args.forwards,
           "unit": "us per eval forward (whole model: plan + phi + rho + GINE stage), device events around each window",
           "configs": {}}
    for name, cfg in CONFIGS.items():
        model, sd, host, dd = build(cfg, dev)
        t = timed(model, dd, args.rounds, args.forwards)
        hi = t["highest"]
        entry = {"graphs": cfg["batch"]["num_graphs"], "max_k": cfg["max_k"], "time": t,
                 "highest_spread_us": hi["max_us"] - hi["min_us"],
                 "speedup_vs_highest": {m: hi["median_us"] / t[m]["median_us"] for m in MODES}}
        if not args.skip_accuracy:
            entry["e_gpu_vs_float64_32_graphs"] = accuracy(cfg, model, sd, host, dev)
        res["configs"][name] = entry
        print(name, json.dumps({m: round(t[m]["median_us"], 1) for m in MODES}), "spread(highest)", round(entry["highest_spread_us"], 2),
              entry.get("e_gpu_vs_float64_32_graphs"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
