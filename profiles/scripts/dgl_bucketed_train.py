"""The DGL tree's training step on SHUFFLED batch shapes: the eager loop of train_ZINC_graph_regression.py:60-82 vs
train_graph.DGLBucketedStep (one capture per capacity bucket).

16 batches of 128 ZINC-like molecules (synth.make_batch, seeds 1-16: every batch has its own N and E), for the shipped `gatedgcn`
(k = 8, GINDeepSigns) and `gatedgcn_mask` (k = 37, MaskedGINDeepSigns) configs at their shipped widths.  For each: eager ms/step over
the sequence and bucketed ms/step (after the first pass, which captures), PASSES passes each, alternating; captures, hits, padding
fraction of the rows, memory_reserved per capture, and the device block of bench.py (measured clock).

    python profiles/scripts/dgl_bucketed_train.py [out.json]        (default: profiles/dgl_bucketed_train.json)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from signnet_basisnet_amd import dgl_configs, dgl_nets, optim, synth  # noqa: E402
from signnet_basisnet_amd.dgl_deepsigns import Graph  # noqa: E402
from signnet_basisnet_amd.train_graph import DGLBucketedStep  # noqa: E402

DEV = "cuda:0"
SEEDS = range(1, 17)
GRAPHS = 128
PASSES = 5
GRANULE = dict(N=256, E=512)


def _batches(k):
    out = []
    g = torch.Generator().manual_seed(0)
    for s in SEEDS:
        d = synth.make_batch(GRAPHS, seed=s)
        src, dst = d.edge_index
        out.append(dict(g=Graph(src.to(DEV), dst.to(DEV), torch.tensor(d.sizes).to(DEV)), h=d.x.squeeze(-1).to(DEV),
                        p=synth.dgl_pos_enc(d, k).to(DEV), e=d.edge_attr.to(DEV), t=torch.randn(GRAPHS, 1, generator=g).to(DEV),
                        N=d.batch.numel(), E=d.edge_index.shape[1]))
    return out


def _net(name):
    cls, p = dgl_configs.net_params(name, DEV)
    torch.manual_seed(0)
    net = getattr(dgl_nets, cls)(p).to(DEV).train()
    return net, optim.FlatAdam(net.parameters(), lr=1e-4)


def _pass(fn, batches):
    """ms per step over one whole pass of the sequence."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        fn(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def run(name):
    k = dgl_configs.SHIPPED[name]["pos_enc_dim"]
    batches = _batches(k)
    res = dict(config=name, k=k, batches=len(batches), graphs=GRAPHS, nodes=[b["N"] for b in batches], edges=[b["E"] for b in batches])
    net2, o2 = _net(name)
    step = DGLBucketedStep(net2, o2, max_graphs=GRAPHS, granule=GRANULE, max_captures=4)
    bucketed = lambda b: step.step(b["g"], b["h"], b["p"], b["e"], None, b["t"])
    # first pass: captures every bucket (before the eager net exists: the memory reserved per capture is that capture's alone)
    res["first_pass_ms_per_step"] = _pass(bucketed, batches)
    net, o = _net(name)

    def eager(b):          # train_ZINC_graph_regression.py:66-81 (the per-step loss.item() of :82 left out)
        o.zero_grad()
        p = net.sign_inv_net(b["g"], b["p"].unsqueeze(-1)).squeeze(-1)
        y, _ = net(b["g"], b["h"], p, b["e"], None)
        net.loss(y, b["t"]).backward()
        o.step()

    _pass(eager, batches)                     # warm-up pass (lazy setup, allocator)
    # the two loops alternate pass by pass on the same box: a drift of the clock or of the host load hits both
    eager_ms, bucketed_ms = [], []
    for _ in range(PASSES):
        eager_ms.append(_pass(eager, batches))
        bucketed_ms.append(_pass(bucketed, batches))
    res["eager_ms_per_step"], res["eager_passes_ms"] = statistics.median(eager_ms), eager_ms
    res["bucketed_ms_per_step"], res["bucketed_passes_ms"] = statistics.median(bucketed_ms), bucketed_ms
    step.check()
    res["speedup"] = res["eager_ms_per_step"] / res["bucketed_ms_per_step"]
    res["captures"], res["hits"] = step.captures, step.hits
    res["granule"] = dict(step.granule)
    res["buckets"] = [dict(N=bk.N, E=bk.E) for bk in step.buckets]
    rows = dict(nodes=[0, 0], edges=[0, 0])
    for b in batches:
        bk = step.bucket_of(b["g"], b["h"])
        for key, n, cap in (("nodes", b["N"], bk.N), ("edges", b["E"], bk.E)):
            rows[key][0] += cap - n
            rows[key][1] += cap
    res["padding_fraction"] = {key: v[0] / v[1] for key, v in rows.items()}
    res["memory_reserved_per_capture_MB"] = [round(c.memory_reserved / 2**20, 1) for c in step._lru.values()]
    res["memory_reserved_total_MB"] = round(torch.cuda.memory_reserved(DEV) / 2**20, 1)
    step.release()
    del step, net, o, net2, o2
    torch.cuda.empty_cache()
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dgl_bucketed_train.json")
    res = dict(device=bench.device_block(DEV), runs=[run("gatedgcn"), run("gatedgcn_mask")])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["runs"]:
        print(f"{r['config']} (k={r['k']}): eager {r['eager_ms_per_step']:.2f} ms/step {[round(v, 2) for v in r['eager_passes_ms']]}, "
              f"bucketed {r['bucketed_ms_per_step']:.2f} ms/step {[round(v, 2) for v in r['bucketed_passes_ms']]}, "
              f"captures {r['captures']}, hits {r['hits']}, padding {r['padding_fraction']}, MB/capture {r['memory_reserved_per_capture_MB']}")


if __name__ == "__main__":
    main()
