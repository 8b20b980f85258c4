"""rho alone on a batch with more bins than two workgroups per CU hold: launch time of fused.RhoPlan.run (one layer, register attention).

    SN_RHO_RESIDENT=2 python profiles/scripts/rho_resident.py --hidden 64 --nodes 4101     # two workgroups per CU (the earlier launch)
    python profiles/scripts/rho_resident.py --hidden 64 --nodes 4101                        # three where the batch has the bins

The switch is read once per process, so the two forms are alternated from the shell (one process each) on one box.  Prints one JSON
line: the per-launch time of `--launches` back-to-back launches between two device events (median / min / max over `--rounds`), and
the SHA-256 of out_sum — the two forms must print the same digest.  Rows are x ~ N(0, 1) on graphs of 9..37 nodes, max_k 16.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=4101)
    ap.add_argument("--max-k", type=int, default=16)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from signnet_basisnet_amd import fused, ops, pyg
    dev = torch.device("cuda", 0)
    sizes, n, rem = [], 9, args.nodes
    while rem >= n + 9:
        sizes.append(n)
        rem -= n
        n = 9 + (n - 9 + 11) % 29
    sizes += [rem] if rem <= 37 else [rem // 2, rem - rem // 2]
    N, B, K, d = sum(sizes), len(sizes), args.max_k, args.hidden
    torch.manual_seed(0)
    rho = pyg.SetTransformer(d, 1, "gine").to(dev).eval()
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(dev)
    plan = ops.build_plan(batch, torch.empty(2, 0, dtype=torch.int64, device=dev), B, K, bins=True)
    nv = torch.repeat_interleave(torch.tensor([min(s, K) for s in sizes]), torch.tensor(sizes))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(N, K, d, generator=g) * (torch.arange(K)[None, :] < nv[:, None]).unsqueeze(-1)).to(dev).view(N * K, d).contiguous()
    rp = fused.RhoPlan(rho, None, pyg.N_HEAD, pyg.LN_EPS)
    out = torch.empty(N, d, device=dev)
    per = []
    with torch.no_grad():
        for _ in range(50):
            rp.run(plan, x, None, K, out=out)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                rp.run(plan, x, None, K, out=out)
            e1.record()
            torch.cuda.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / args.launches)
    plan.check()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    print(json.dumps({"resident_env": os.environ.get("SN_RHO_RESIDENT"), "hidden": d, "nodes": N, "graphs": B, "max_k": K, "bins": (N + 3) // 4,
                      "cus": cus, "launches": args.launches, "us_per_launch_median": statistics.median(per), "us_per_launch_min": min(per),
                      "us_per_launch_max": max(per), "out_sum_sha256": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}))


if __name__ == "__main__":
    main()
