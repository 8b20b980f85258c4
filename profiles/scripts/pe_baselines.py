"""What SignNet costs per training step next to the baseline PE rows of the same table: GatedGCN at pe_init 'no_pe', behind the
sign-flip and the canonical LapPE (configs/gatedgcn/GatedGCN_ZINC_{NoPE,LapPE,LapPE_can}.json: hidden 77, 16 layers) and with the
sign-invariant net (GatedGCN_ZINC_LapPE_signinv_GIN.json: hidden 68 + GINDeepSigns), all through the same loops.

The protocol of profiles/scripts/dgl_bucketed_train.py: 16 shuffled batches of 128 ZINC-like molecules, the eager loop of
train_ZINC_graph_regression.py:60-82 and train_graph.DGLBucketedStep alternating pass by pass, median and range over five passes.
Also the transform kernel alone (sn_lap_pe_transform_f32, HIP events over 200 launches per mode) on the first batch.

    python profiles/scripts/pe_baselines.py [out.json]        (default: profiles/pe_baselines.json)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import bench  # noqa: E402
import dgl_bucketed_train as base  # noqa: E402
from signnet_basisnet_amd import dgl_nets, ops  # noqa: E402
from signnet_basisnet_amd.train_graph import DGLBucketedStep  # noqa: E402

DEV = base.DEV
ROWS = [("gatedgcn_nope", "NoPE"), ("gatedgcn_lappe", "sign_flip"), ("gatedgcn_lappe_can", "canonical"), ("gatedgcn", "sign_inv")]


def run(name, label):
    net2, o2 = base._net(name)
    batches = base._batches(net2.pos_enc_dim)
    res = dict(config=name, row=label, hidden=net2.embedding_h.weight.shape[1], k=net2.pos_enc_dim, batches=len(batches), graphs=base.GRAPHS)
    step = DGLBucketedStep(net2, o2, max_graphs=base.GRAPHS, granule=base.GRANULE, max_captures=4)
    lap = net2.pe_init == "lap_pe"
    bucketed = lambda b: step.step(b["g"], b["h"], b["p"] if lap else None, b["e"], None, b["t"])
    res["first_pass_ms_per_step"] = base._pass(bucketed, batches)
    net, o = base._net(name)

    def eager(b):          # train_ZINC_graph_regression.py:66-81 (the per-step loss.item() of :82 left out)
        o.zero_grad()
        p = dgl_nets.handle_lap(net, b["p"], b["g"], DEV) if lap else None
        y, _ = net(b["g"], b["h"], p, b["e"], None)
        net.loss(y, b["t"]).backward()
        o.step()

    base._pass(eager, batches)
    eager_ms, bucketed_ms = [], []
    for _ in range(base.PASSES):
        eager_ms.append(base._pass(eager, batches))
        bucketed_ms.append(base._pass(bucketed, batches))
    step.check()
    res["eager_ms_per_step"], res["eager_passes_ms"] = statistics.median(eager_ms), eager_ms
    res["bucketed_ms_per_step"], res["bucketed_passes_ms"] = statistics.median(bucketed_ms), bucketed_ms
    res["speedup"] = res["eager_ms_per_step"] / res["bucketed_ms_per_step"]
    res["captures"], res["hits"] = step.captures, step.hits
    step.release()
    del step, net, o, net2, o2
    torch.cuda.empty_cache()
    return res


def transform_alone(reps=200):
    b = base._batches(8)[0]
    p = b["p"]
    gp = dgl_nets.cached_plan(b["g"], p.shape[0]).graph_ptr
    u = torch.rand(8, device=DEV)
    out = dict(nodes=int(p.shape[0]), k=8, graphs=base.GRAPHS, launches=reps, us_per_launch={})
    for mode, kw in (("none", {}), ("sign_flip", dict(u=u)), ("abs_val", {}), ("canonical", dict(graph_ptr=gp))):
        dst = torch.empty_like(p)
        for _ in range(10):
            ops.lap_pe_transform(p, mode, out=dst, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.lap_pe_transform(p, mode, out=dst, **kw)
        e1.record()
        torch.cuda.synchronize()
        out["us_per_launch"][mode] = e0.elapsed_time(e1) * 1e3 / reps      # (back-to-back launches: launch-bound, includes the host's issue rate)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pe_baselines.json")
    res = dict(device=bench.device_block(DEV), transform=transform_alone(), runs=[run(n, l) for n, l in ROWS])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("transform us/launch", {k: round(v, 2) for k, v in res["transform"]["us_per_launch"].items()})
    for r in res["runs"]:
        print(f"{r['row']} ({r['config']}, hidden {r['hidden']}): eager {r['eager_ms_per_step']:.2f} ms/step "
              f"{[round(v, 2) for v in r['eager_passes_ms']]}, bucketed {r['bucketed_ms_per_step']:.2f} ms/step "
              f"{[round(v, 2) for v in r['bucketed_passes_ms']]}, captures {r['captures']}, hits {r['hits']}")


if __name__ == "__main__":
    main()
