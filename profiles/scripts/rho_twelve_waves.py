"""rho alone (one layer, register attention, d = 128): launch time of fused.RhoPlan.run per workgroup form, alternating in ONE process.

    python profiles/scripts/rho_twelve_waves.py --nodes 2950 4101 --waves 4 12

For every node count and every form (`waves` of RhoPlan.run: 4 = four-wave workgroups, two or three resident per CU; 12 = one
twelve-wave workgroup per CU; 0 = the library's choice) `--rounds` rounds of `--launches` back-to-back launches between two device
events, the forms alternating inside a round.  Prints one JSON line per node count: per form the per-launch time (median / min / max
over the rounds) and the SHA-256 of out_sum — the forms must print the same digest.  Rows are x ~ N(0, 1) on graphs of 9..37 nodes,
max_k 16 (the batch of profiles/scripts/rho_resident.py).
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
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--nodes", type=int, nargs="+", default=[2950, 4101])
    ap.add_argument("--waves", type=int, nargs="+", default=[4, 12])
    ap.add_argument("--max-k", type=int, default=16)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from signnet_basisnet_amd import fused, ops, pyg
    dev = torch.device("cuda", 0)
    K, d = args.max_k, args.hidden
    torch.manual_seed(0)
    rho = pyg.SetTransformer(d, 1, "gine").to(dev).eval()
    rp = fused.RhoPlan(rho, None, pyg.N_HEAD, pyg.LN_EPS)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for nodes in args.nodes:
        sizes, n, rem = [], 9, nodes
        while rem >= n + 9:
            sizes.append(n)
            rem -= n
            n = 9 + (n - 9 + 11) % 29
        sizes += [rem] if rem <= 37 else [rem // 2, rem - rem // 2]
        N, B = sum(sizes), len(sizes)
        batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(dev)
        plan = ops.build_plan(batch, torch.empty(2, 0, dtype=torch.int64, device=dev), B, K, bins=True)
        nv = torch.repeat_interleave(torch.tensor([min(s, K) for s in sizes]), torch.tensor(sizes))
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(N, K, d, generator=g) * (torch.arange(K)[None, :] < nv[:, None]).unsqueeze(-1)).to(dev).view(N * K, d).contiguous()
        out = {w: torch.empty(N, d, device=dev) for w in args.waves}
        per = {w: [] for w in args.waves}
        with torch.no_grad():
            for w in args.waves:
                for _ in range(50):
                    rp.run(plan, x, None, K, out=out[w], waves=w)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for w in args.waves:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        rp.run(plan, x, None, K, out=out[w], waves=w)
                    e1.record()
                    torch.cuda.synchronize()
                    per[w].append(1e3 * e0.elapsed_time(e1) / args.launches)
        plan.check()
        print(json.dumps({"hidden": d, "nodes": N, "graphs": B, "max_k": K, "bins4": (N + 3) // 4, "bins12": (N + 11) // 12, "cus": cus,
                          "launches": args.launches,
                          "forms": {str(w): {"us_per_launch_median": round(statistics.median(per[w]), 2), "us_per_launch_min": round(min(per[w]), 2),
                                             "us_per_launch_max": round(max(per[w]), 2),
                                             "out_sum_sha256": hashlib.sha256(out[w].cpu().numpy().tobytes()).hexdigest()} for w in args.waves}}),
              flush=True)


if __name__ == "__main__":
    main()
