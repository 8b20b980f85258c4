"""Training step on SHUFFLED batch shapes: the eager step vs train_graph.BucketedStep (one capture per capacity bucket).

16 batches of 128 graphs at the bench workload's sizes (bench.WORKLOAD, seeds 1-16: every batch has its own N, E and eigenvector
block), at k = 16 and with all eigenvectors (max_k=None).  For each: eager ms/step over the sequence, bucketed ms/step (after the
first pass, which captures), captures, padding fraction of the rows, memory_reserved per capture.

    python profiles/scripts/bucketed_train.py [out.json]        (default: profiles/r07_bucketed_train.json)
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
from signnet_basisnet_amd import optim, synth  # noqa: E402
from signnet_basisnet_amd.train_graph import BucketedStep  # noqa: E402

DEV = "cuda:0"
W = bench.WORKLOAD
SEEDS = range(1, 17)
PASSES = 3
GRANULE = dict(N=256, E=512, S=16384, K=8)


def _batches():
    hosts = [synth.make_batch(W["B"], seed=s, n_lo=W["n_lo"], n_hi=W["n_hi"], features=W["features"]) for s in SEEDS]
    g = torch.Generator().manual_seed(0)
    targets = [torch.randn(h.num_graphs, W["n_out"], generator=g).to(DEV) for h in hosts]
    return hosts, [synth.batch_to(h, DEV) for h in hosts], targets


def _timed(fn, batches, targets):
    """ms per step over whole passes of the sequence (median of PASSES passes)."""
    out = []
    for _ in range(PASSES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d, t in zip(batches, targets):
            fn(d, t)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / len(batches))
    return statistics.median(out), out


def run(k):
    hosts, batches, targets = _batches()
    res = dict(k="all" if k is None else k, batches=len(batches), graphs=W["B"],
               nodes=[h.batch.numel() for h in hosts], edges=[h.edge_index.shape[1] for h in hosts])
    m = bench.build_model(DEV, k=k).train()
    o = optim.FlatAdam(m.parameters(), lr=1e-4)

    def eager(d, t):
        o.zero_grad()
        loss = (m(d) - t).abs().mean()
        loss.backward()
        o.step()

    for d, t in zip(batches, targets):        # warm-up pass (lazy setup, allocator)
        eager(d, t)
    res["eager_ms_per_step"], res["eager_passes_ms"] = _timed(eager, batches, targets)
    del m, o
    torch.cuda.empty_cache()

    m = bench.build_model(DEV, k=k).train()
    o = optim.FlatAdam(m.parameters(), lr=1e-4)
    step = BucketedStep(m, o, max_graphs=W["B"], granule=GRANULE, max_captures=4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for d, t in zip(batches, targets):        # first pass: captures every bucket
        step.step(d, t)
    torch.cuda.synchronize()
    res["first_pass_ms_per_step"] = (time.perf_counter() - t0) * 1e3 / len(batches)
    res["bucketed_ms_per_step"], res["bucketed_passes_ms"] = _timed(lambda d, t: step.step(d, t), batches, targets)
    step.check()
    res["captures"], res["hits"] = step.captures, step.hits
    res["granule"] = dict(step.granule)
    res["buckets"] = [dict(N=b.N, E=b.E, S=b.S, K=b.K) for b in step.buckets]
    rows = dict(nodes=[0, 0], edges=[0, 0], eigvec_entries=[0, 0])
    for h in hosts:
        b = step.bucket_of(h)
        for key, n, cap in (("nodes", h.batch.numel(), b.N), ("edges", h.edge_index.shape[1], b.E),
                            ("eigvec_entries", h.eigen_vectors.numel(), b.S)):
            rows[key][0] += cap - n
            rows[key][1] += cap
    res["padding_fraction"] = {key: v[0] / v[1] for key, v in rows.items()}
    res["memory_reserved_per_capture_MB"] = [round(c.memory_reserved / 2**20, 1) for c in step._lru.values()]
    res["memory_reserved_total_MB"] = round(torch.cuda.memory_reserved(DEV) / 2**20, 1)
    del step, m, o
    torch.cuda.empty_cache()
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_bucketed_train.json")
    res = dict(workload=W["name"], device=torch.cuda.get_device_name(0), target_ms_k16=3.3,
               runs=[run(W["k"]), run(None)])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["runs"]:
        print(f"k={r['k']}: eager {r['eager_ms_per_step']:.2f} ms/step, bucketed {r['bucketed_ms_per_step']:.2f} ms/step, "
              f"captures {r['captures']}, padding {r['padding_fraction']}, MB/capture {r['memory_reserved_per_capture_MB']}")


if __name__ == "__main__":
    main()
