"""What delivering the batch costs a training step: host collate vs resident batches vs the device-resident store.

Pool: 4 096 synthetic molecules (synth.make_batch, 9-37 nodes), ONE seeded shuffle cut into 32 batches of 128 graphs.  Three ways
to hand the same batches to the same captured step (one covering bucket: one capture per path), alternating pass by pass in one
process, the first pass of each discarded:
  (a) host     per-sample CPU tensors -> the torch.cat collate of the reference's DataLoader (edge ids re-based, eigenvector blocks
               laid end to end) -> pinned copies -> BucketedStep.step
  (b) resident the same batches collated and copied to the device beforehand -> BucketedStep.step (nothing but the pack launch)
  (c) store    data.GraphStore + data.IndexLoader -> BucketedStep.step_from (one sn_store_gather launch, no copy)
for the headline training model SignNetGNN(None, None, 128, 1, 4, 6) at max_k = 16, and the same three for GatedGCNNet (k = 8) with
DGLBucketedStep.  Per path: ms/step (median over the passes), every pass, captures and hits; the bytes a gather moves, from shapes.

    python profiles/scripts/device_loader.py [out.json]                 (default: profiles/device_loader.json)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/scripts/device_loader.py --gather-only
    python profiles/scripts/device_loader.py --merge-stats DIR [out.json]    (the gather's kernel time and bytes/s into the json)
"""
import csv
import glob
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from signnet_basisnet_amd import dgl_configs, dgl_nets, optim, synth  # noqa: E402
from signnet_basisnet_amd.data import DGLGraphStore, GraphSizes, GraphStore, IndexLoader  # noqa: E402
from signnet_basisnet_amd.dgl_deepsigns import Graph  # noqa: E402
from signnet_basisnet_amd.train_graph import BucketedStep, DGLBucketedStep  # noqa: E402

DEV = "cuda:0"
POOL, GRAPHS, SEED = 4096, 128, 0
PASSES = 6                      # per path, the first discarded
K_PYG, K_DGL = 16, 8
OUT = os.path.join(ROOT, "profiles", "device_loader.json")


def _pool():
    """-> (collated pool on the host, per-graph samples as views of it with local edge ids, targets [POOL, 1])."""
    whole = synth.make_batch(POOL, seed=SEED, n_lo=9, n_hi=37)
    sz = GraphSizes.from_batch(whole)
    samples = []
    for g in range(POOL):
        n0, n1, e0, e1, s0, s1 = sz.node_ptr[g], sz.node_ptr[g + 1], sz.edge_ptr[g], sz.edge_ptr[g + 1], sz.eig_ptr[g], sz.eig_ptr[g + 1]
        samples.append(types.SimpleNamespace(
            x=whole.x[n0:n1], edge_index=whole.edge_index[:, e0:e1] - n0, edge_attr=whole.edge_attr[e0:e1],
            eigen_values=whole.eigen_values[n0:n1], eigen_vectors=whole.eigen_vectors[s0:s1], num_nodes=int(n1 - n0)))
    y = torch.randn(POOL, 1, generator=torch.Generator().manual_seed(1))
    return whole, samples, y


def _collate(samples, idx, y):
    """The reference loader's collate: seven tensors concatenated per batch, edge ids re-based (a Python loop over the samples)."""
    sel = [samples[i] for i in idx]
    off, eis, batch = 0, [], []
    for b, s in enumerate(sel):
        eis.append(s.edge_index + off)
        batch.append(torch.full((s.num_nodes,), b, dtype=torch.long))
        off += s.num_nodes
    d = types.SimpleNamespace(
        x=torch.cat([s.x for s in sel]), edge_index=torch.cat(eis, 1), edge_attr=torch.cat([s.edge_attr for s in sel]),
        batch=torch.cat(batch), eigen_values=torch.cat([s.eigen_values for s in sel]),
        eigen_vectors=torch.cat([s.eigen_vectors for s in sel]), num_graphs=len(sel), num_nodes=off)
    d.sizes = [s.num_nodes for s in sel]
    return d, y[torch.from_numpy(idx)]


def _pinned_to(d, t):
    """Seven pinned host-to-device copies + the target's."""
    out = types.SimpleNamespace(**vars(d))
    for k, v in vars(d).items():
        if torch.is_tensor(v):
            setattr(out, k, v.pin_memory().to(DEV, non_blocking=True))
    return out, t.pin_memory().to(DEV, non_blocking=True)


def _dgl_sample(s, k):
    s.sizes = [s.num_nodes]
    return (Graph(s.edge_index[0], s.edge_index[1], [s.num_nodes]), s.x.reshape(-1), synth.dgl_pos_enc(s, k), s.edge_attr.reshape(-1))


def _dgl_collate(dsamples, idx, y):
    sel = [dsamples[i] for i in idx]
    off, src, dst = 0, [], []
    for g, h, _, _ in sel:
        src.append(g.src + off)
        dst.append(g.dst + off)
        off += h.shape[0]
    return (torch.cat(src), torch.cat(dst), [int(s[1].shape[0]) for s in sel], torch.cat([s[1] for s in sel]),
            torch.cat([s[2] for s in sel]), torch.cat([s[3] for s in sel]), y[torch.from_numpy(idx)])


def _dgl_to(c, pinned):
    mv = (lambda v: v.pin_memory().to(DEV, non_blocking=True)) if pinned else (lambda v: v.to(DEV))
    src, dst, sizes, h, p, e, t = c
    return Graph(mv(src), mv(dst), sizes), mv(h), mv(p), mv(e), None, mv(t)


def _pass(fn, items):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in items:
        fn(it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(items)


def _alternate(paths, items):
    """PASSES passes of every path, alternating; the first of each discarded.  -> {name: record}."""
    passes = {name: [] for name in paths}
    for _ in range(PASSES):
        for name, (fn, step) in paths.items():
            passes[name].append(_pass(fn, items[name]))
    out = {}
    for name, (fn, step) in paths.items():
        step.check()
        kept = passes[name][1:]
        out[name] = dict(ms_per_step=statistics.median(kept), passes_ms=kept, spread_ms=max(kept) - min(kept),
                         first_pass_ms=passes[name][0], captures=step.captures, hits=step.hits)
    return out


def _gather_bytes(store, pad, batches):
    """Bytes one gather moves, from shapes: the selected graphs' source rows + index and table entries read, every capacity buffer
    written (mean over the batches)."""
    written = sum(t.numel() * t.element_size() for _, t, _, _, _ in store.segments(pad)) + 4 * 4 + pad.counts.numel() * 4
    read = []
    for idx in batches:
        N, E, S, _ = store.totals(idx)
        B = len(idx)
        rows = {0: N, 1: E, 2: S, 3: B}
        r = sum(rows[kind] * src.element_size() * (src[0].numel() if src.dim() > 1 else 1)
                for src, _, kind, _, _ in store.segments(pad) if src is not None)
        read.append(r + B * 8 + B * 2 * 8 * (2 if store.dgl else 3))
    return dict(read=statistics.mean(read), written=written, total=statistics.mean(read) + written)


def _models_pyg():
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    m = SignNetGNN(None, None, 128, 1, 4, 6, variant="gine", max_k=K_PYG).to(DEV).train()
    return m, optim.FlatAdam(m.parameters(), lr=1e-4)


def _models_dgl():
    cls, p = dgl_configs.net_params("gatedgcn", DEV)
    torch.manual_seed(0)
    net = getattr(dgl_nets, cls)(p).to(DEV).train()
    return net, optim.FlatAdam(net.parameters(), lr=1e-4)


def setup():
    whole, samples, y = _pool()
    loader = IndexLoader(POOL, GRAPHS, shuffle=True, seed=SEED, device=DEV)
    loader.epoch(0)
    pairs = list(loader)                                        # (host indices, device view) of the ONE shuffle
    return whole, samples, y, pairs


def run_pyg(whole, samples, y, pairs):
    store = GraphStore.from_batch(whole, y, DEV)
    host_idx = [h for h, _ in pairs]
    gran = dict(BucketedStep(*_models_pyg(), max_graphs=GRAPHS).granule)
    bucket = store.covering_bucket(host_idx, gran, K_PYG)
    distinct = len({store.bucket_of(h, gran, K_PYG) for h in host_idx})
    steps = {n: BucketedStep(*_models_pyg(), max_graphs=GRAPHS) for n in "abc"}
    resident = [_pinned_to(*_collate(samples, h, y)) for h in host_idx]
    torch.cuda.synchronize()

    def host(h):
        d, t = _pinned_to(*_collate(samples, h, y))
        steps["a"].step(d, t, bucket=bucket)
    paths = {"a_host_collate": (host, steps["a"]),
             "b_resident": (lambda dt: steps["b"].step(dt[0], dt[1], bucket=bucket), steps["b"]),
             "c_store": (lambda pair: steps["c"].step_from(store, pair, bucket=bucket), steps["c"])}
    items = {"a_host_collate": host_idx, "b_resident": resident, "c_store": pairs}
    res = dict(model="SignNetGNN(None, None, 128, 1, 4, 6), max_k = %d" % K_PYG, bucket=list(bucket), default_granule_buckets=distinct,
               paths=_alternate(paths, items))
    # the host half of path (a) alone: collate + pinned copies, no step
    res["host_collate_alone_ms"] = _pass(lambda h: _pinned_to(*_collate(samples, h, y)), host_idx)
    res["gather_bytes_per_step"] = _gather_bytes(store, steps["c"]._lru[bucket].pad, host_idx)
    return res


def run_dgl(whole, samples, y, pairs):
    ds = [_dgl_sample(s, K_DGL) for s in samples]
    host_idx = [h for h, _ in pairs]
    g = Graph(whole.edge_index[0], whole.edge_index[1], whole.sizes)
    store = DGLGraphStore.from_batch((g, whole.x.reshape(-1), torch.cat([s[2] for s in ds]), whole.edge_attr.reshape(-1), None), y, DEV)
    bucket = store.covering_bucket(host_idx)
    distinct = len({store.bucket_of(h) for h in host_idx})
    steps = {n: DGLBucketedStep(*_models_dgl(), max_graphs=GRAPHS) for n in "abc"}
    resident = [_dgl_to(_dgl_collate(ds, h, y), False) for h in host_idx]
    torch.cuda.synchronize()
    paths = {"a_host_collate": (lambda h: steps["a"].step(*_dgl_to(_dgl_collate(ds, h, y), True), bucket=bucket), steps["a"]),
             "b_resident": (lambda b: steps["b"].step(*b, bucket=bucket), steps["b"]),
             "c_store": (lambda pair: steps["c"].step_from(store, pair, bucket=bucket), steps["c"])}
    items = {"a_host_collate": host_idx, "b_resident": resident, "c_store": pairs}
    res = dict(model="GatedGCNNet (shipped gatedgcn config), pos_enc_dim = %d" % K_DGL, bucket=list(bucket),
               default_granule_buckets=distinct, paths=_alternate(paths, items))
    res["host_collate_alone_ms"] = _pass(lambda h: _dgl_to(_dgl_collate(ds, h, y), True), host_idx)
    res["gather_bytes_per_step"] = _gather_bytes(store, steps["c"]._lru[bucket].pad, host_idx)
    return res


def gather_only():
    """What the rocprofv3 run traces: gathers alone, into the capacity buffers of the covering buckets (no model)."""
    from signnet_basisnet_amd.train_graph import DGLPaddedBatch, PaddedBatch
    whole, samples, y, pairs = setup()
    store = GraphStore.from_batch(whole, y, DEV)
    host_idx = [h for h, _ in pairs]
    bucket = store.covering_bucket(host_idx, None, K_PYG)
    pad = PaddedBatch(bucket, GRAPHS + 1, *store.proto(), DEV)
    g = Graph(whole.edge_index[0], whole.edge_index[1], whole.sizes)
    p = torch.cat([synth.dgl_pos_enc(types.SimpleNamespace(sizes=[s.num_nodes], eigen_vectors=s.eigen_vectors), K_DGL) for s in samples])
    dstore = DGLGraphStore.from_batch((g, whole.x.reshape(-1), p, whole.edge_attr.reshape(-1), None), y, DEV)
    dpad = DGLPaddedBatch(dstore.covering_bucket(host_idx), GRAPHS + 1, K_DGL, True, False, DEV)
    for _ in range(8):
        for pair in pairs:
            store.gather_into(pair, pad)
    torch.cuda.synchronize()
    for _ in range(8):
        for pair in pairs:
            dstore.gather_into(pair, dpad)
    torch.cuda.synchronize()
    print("gathers: %d PyG then %d DGL" % (8 * len(pairs), 8 * len(pairs)))


def merge_stats(directory, out):
    """The k_store_gather row(s) of a rocprofv3 --kernel-trace --stats run of --gather-only -> the json (the PyG gathers run first)."""
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_store_gather" in r.get("Kernel_Name", ""):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    res = json.load(open(out))
    half = len(rows) // 2
    for key, part in (("pyg", rows[:half]), ("dgl", rows[half:])):
        ns = [d for _, d in part][len(part) // 8:]              # (the first of the eight rounds: warm-up)
        if not ns:
            continue
        us = statistics.median(ns) / 1e3
        b = res[key]["gather_bytes_per_step"]["total"]
        res[key]["gather_kernel"] = dict(calls=len(ns), median_us=us, min_us=min(ns) / 1e3, max_us=max(ns) / 1e3,
                                         achieved_GB_per_s=b / (us * 1e-6) / 1e9)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k].get("gather_kernel") for k in ("pyg", "dgl")}))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--gather-only" in sys.argv:
        return gather_only()
    if "--merge-stats" in sys.argv:
        return merge_stats(args[0], args[1] if len(args) > 1 else OUT)
    out = args[0] if args else OUT
    whole, samples, y, pairs = setup()
    res = dict(device=torch.cuda.get_device_name(0), pool=POOL, graphs_per_step=GRAPHS, steps_per_pass=len(pairs), passes_kept=PASSES - 1,
               shuffle_seed=SEED, pyg=run_pyg(whole, samples, y, pairs))
    torch.cuda.empty_cache()
    res["dgl"] = run_dgl(whole, samples, y, pairs)
    for key in ("pyg", "dgl"):
        p = res[key]["paths"]
        b, c, a = p["b_resident"], p["c_store"], p["a_host_collate"]
        res[key]["store_minus_resident_ms"] = c["ms_per_step"] - b["ms_per_step"]
        res[key]["store_not_slower_than_resident"] = bool(c["ms_per_step"] <= b["ms_per_step"] + b["spread_ms"])
        res[key]["host_within_resident_spread"] = bool(abs(a["ms_per_step"] - b["ms_per_step"]) <= b["spread_ms"])
        print(f"{key}: host collate {a['ms_per_step']:.3f}  resident {b['ms_per_step']:.3f} (spread {b['spread_ms']:.3f})  "
              f"store {c['ms_per_step']:.3f} ms/step; captures {a['captures']}/{b['captures']}/{c['captures']}; "
              f"gather moves {res[key]['gather_bytes_per_step']['total'] / 1e6:.2f} MB")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
