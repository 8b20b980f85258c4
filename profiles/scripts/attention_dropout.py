"""The two sources of the attention-dropout mask (SignNetGNN.attn_dropout_source: "generator" | "counter") in the captured training step,
and the attention launches alone.

  train     profiles/r07_bucketed_train.json's protocol — 16 shuffled batches of 128 ZINC-like graphs through train_graph.BucketedStep,
            k = 16 and all eigenvectors — plus the Alchemy model (bench.WORKLOADS[2]) on batches of its own; the two sources alternate
            pass by pass in one process, five passes each: median and range of ms/step, memory_reserved per capture, and the launches
            step() issues outside the graph (counted from its code path: pack + graph + Adam, plus draw, threshold and copy per rho
            layer for the generator source).
  launches  forward and backward of the set attention at [2950, 4, 16, 32] and [3072, 4, 40, 32] for an explicit mask and for the
            counter source, and the draw / threshold / copy launches the counter source removes: device events, back to back.
  default   the default source alone on the k = 16 row, with nothing this tree adds: the same function runs in the parent commit's
            tree for the regression check (alternating processes; see `parent_ab_same_box` in the output).

    python profiles/scripts/attention_dropout.py [out.json]             (default: profiles/attention_dropout.json)
    python profiles/scripts/attention_dropout.py --default-only out.json
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
from signnet_basisnet_amd import ops, optim, synth  # noqa: E402
from signnet_basisnet_amd.train_graph import BucketedStep  # noqa: E402

DEV = "cuda:0"
PASSES = 5
GRANULE = dict(N=256, E=512, S=16384, K=8)


def _batches(W, seeds):
    hosts = [synth.make_batch(W["B"], seed=s, n_lo=W["n_lo"], n_hi=W["n_hi"], features=W["features"]) for s in seeds]
    g = torch.Generator().manual_seed(0)
    targets = [torch.randn(h.num_graphs, W["n_out"], generator=g).to(DEV) for h in hosts]
    return hosts, [synth.batch_to(h, DEV) for h in hosts], targets


def _model(W, k):
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    m = SignNetGNN(W["node_feat"], W["edge_feat"], W["hidden"], W["n_out"], W["nl_signnet"], W["nl_gnn"], variant=W["variant"], max_k=k)
    return m.to(DEV).train()


def _pass(step, batches, targets):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for d, t in zip(batches, targets):
        step.step(d, t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def _summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), passes_ms=ms)


def train_row(W, k, seeds, sources=("generator", "counter")):
    hosts, batches, targets = _batches(W, seeds)
    row = dict(workload=W["name"], k="all" if k is None else k, batches=len(batches), graphs=W["B"])
    steps = {}
    for src in sources:
        m = _model(W, k)
        if src != "default":                      # ("default": nothing this tree adds is touched)
            m.attn_dropout_source = src
        o = optim.FlatAdam(m.parameters(), lr=1e-4)
        torch.cuda.empty_cache()                  # (memory_reserved per capture: no cached block of the other source to reuse)
        steps[src] = BucketedStep(m, o, max_graphs=W["B"], granule=GRANULE, max_captures=4)
        _pass(steps[src], batches, targets)       # first pass: captures every bucket
    ms = {src: [] for src in sources}
    for _ in range(PASSES):                       # the sources alternate pass by pass
        for src in sources:
            ms[src].append(_pass(steps[src], batches, targets))
    n_rho = len(steps[sources[0]].model.sign_net.rho.transformer_layers)
    for src in sources:
        s = steps[src]
        s.check()
        caps = list(s._lru.values())
        row[src] = dict(**_summary(ms[src]), captures=s.captures,
                        buckets=[dict(N=b.N, E=b.E, S=b.S, K=b.K) for b in s.buckets],
                        memory_reserved_per_capture_MB=[round(c.memory_reserved / 2**20, 1) for c in caps],
                        mask_buffer_MB_per_capture=[round(sum(x.numel() * 4 for x in (c._masks or [])) / 2**20, 1) for c in caps],
                        launches_outside_graph=3 + (0 if caps[0]._masks is None else 3 * n_rho))
    for s in steps.values():
        s.release()
    del steps
    torch.cuda.empty_cache()
    return row


def _events(fn, iters=200, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(5):
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out))


def launches(N, H, K, dk, p=0.1):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    g = torch.Generator(device=DEV).manual_seed(1)
    q, k, v, go = (torch.randn(N * K, H * dk, device=DEV, generator=g) for _ in range(4))
    out, dq, dk_, dv = (torch.empty_like(q) for _ in range(4))
    nv = torch.randint(max(K // 2, 1), K + 1, (N,), device=DEV, generator=g, dtype=torch.int32)
    pm = ops.attention_dropout_mask(N, K, H, p, DEV)
    static = torch.empty_like(pm)
    snap = ops.DropoutState(1, DEV, 1).snapshot()
    thr, scale = ops.dropout_threshold(p)
    L = lib()
    res = dict(shape=[N, H, K, dk], p=p, mask_MB=round(pm.numel() * 4 / 2**20, 2))
    res["fwd_explicit_mask"] = _events(lambda: check(L.sn_set_attention_f32(ptr(q), ptr(k), ptr(v), N, K, H, dk, ptr(nv), ptr(pm), ptr(out), stream()), "fwd"))
    res["fwd_counter"] = _events(lambda: check(L.sn_set_attention_drop_f32(ptr(q), ptr(k), ptr(v), N, K, H, dk, ptr(nv), thr, scale, ptr(snap),
                                                                           ops.ATTN_DROP_SITE, ptr(out), stream()), "fwd drop"))
    res["bwd_explicit_mask"] = _events(lambda: check(L.sn_set_attention_bwd_f32(ptr(q), ptr(k), ptr(v), ptr(go), N, K, H, dk, ptr(nv), ptr(pm), ptr(dq),
                                                                                ptr(dk_), ptr(dv), stream()), "bwd"))
    res["bwd_counter"] = _events(lambda: check(L.sn_set_attention_drop_bwd_f32(ptr(q), ptr(k), ptr(v), ptr(go), N, K, H, dk, ptr(nv), thr, scale,
                                                                               ptr(snap), ops.ATTN_DROP_SITE, ptr(dq), ptr(dk_), ptr(dv), stream()),
                                               "bwd drop"))
    res["draw_and_threshold"] = _events(lambda: ops.attention_dropout_mask(N, K, H, p, DEV))
    res["copy_to_static_buffer"] = _events(lambda: static.copy_(pm))
    return res


def main():
    args = sys.argv[1:]
    W1, W2 = bench.WORKLOADS[1], bench.WORKLOADS[2]
    if args and args[0] == "--default-only":
        res = train_row(W1, W1["k"], range(1, 17), sources=("default",))
        with open(args[1], "w") as f:
            json.dump(res, f, indent=1)
        print(f"default source, k=16: {res['default']['median_ms']:.3f} ms/step {res['default']['passes_ms']}")
        return
    out = args[0] if args else os.path.join(ROOT, "profiles", "attention_dropout.json")
    res = dict(device=torch.cuda.get_device_name(0), passes=PASSES,
               train=[train_row(W1, W1["k"], range(1, 17)), train_row(W1, None, range(1, 17)), train_row(W2, W2["k"], range(1, 5))],
               launches=[launches(2950, 4, 16, 32), launches(3072, 4, 40, 32)])
    if os.path.exists(out):                        # (the regression check is merged in by the session that ran both trees)
        with open(out) as f:
            old = json.load(f)
        if "parent_ab_same_box" in old:
            res["parent_ab_same_box"] = old["parent_ab_same_box"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["train"]:
        print(f"{r['workload'][:24]} k={r['k']}: " + ", ".join(
            f"{s} {r[s]['median_ms']:.3f} ms/step [{r[s]['min_ms']:.3f}, {r[s]['max_ms']:.3f}] {r[s]['memory_reserved_per_capture_MB']} MB "
            f"{r[s]['launches_outside_graph']} launches" for s in ("generator", "counter")))
    for r in res["launches"]:
        print(r["shape"], {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict)})


if __name__ == "__main__":
    main()
