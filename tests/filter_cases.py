"""Shared by tests/test_filter_baselines_cpu.py and tests/test_filter_baselines_gpu.py: the graphs of the polynomial-filter kernel tests
and float64 restatements, on DENSE operators built from the definitions, of everything the filter baselines compute —

  dense_lap_adj   A = D^-1/2 A D^-1/2 of get_laplacian(..., 'sym'): self loops removed, degree over the source index, 1/0 -> 0, multi-edges add
  dense_gcn       gcn_norm: input self loops replaced by one unit loop per node, degree over the target index
  basis_ref / combine_ref   P_k(S) x and sum_k c_k P_k(S) a_k from the matrix polynomials themselves (no Horner / Clenshaw)
  bern_conv_ref   BernConv.forward in its ORIGINAL form (models.py:326-340): K propagations by 2I - L, then for every i the i + 1
                  propagations by L — K + K (K + 1) / 2 = 65 for K = 10 — so the two-launch rewrite is checked against it
  net_ref         BernNet / GPRNet / ChebNet / GcnNet forward from a reference-keyed state_dict (differentiable, any dtype)

Messages go from edge_index[0] to edge_index[1]: (S x)_i sums over the edges whose TARGET is i.
"""
import math

import numpy as np
import torch

from signnet_basisnet_amd import synth

REL = 1e-5            # the project's bound: 1e-5 of the output's scale against float64


def bound(recorded=0.0):
    """REL, or 4 x the reference's own recorded fp32-vs-float64 error where that is larger than REL."""
    return REL if recorded <= REL else 4.0 * recorded


def ring(n):
    i = np.arange(n)
    return np.stack([np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i])]), n


def _graphs():
    g = {}
    g["single"] = (np.zeros((2, 0), dtype=np.int64), 1)                                         # N = 1, no edges
    p = np.array([[0, 1, 1, 2, 2, 3, 3, 4], [1, 0, 2, 1, 3, 2, 4, 3]])
    g["path5_isolated"] = (p, 6)                                                                # a 5-path and an isolated node 5
    g["directed_cycle_chord"] = (np.array([[0, 1, 2, 0], [1, 2, 0, 2]]), 3)                     # non-symmetric: S^T != S
    e = np.array([[0, 1, 1, 2, 2, 0, 0, 3, 3, 1, 2, 2], [1, 0, 2, 1, 0, 2, 1, 2, 3, 3, 3, 2]])  # 0->1 twice, self loops 3->3 and 2->2
    g["dup_selfloop_shuffled"] = (e[:, np.random.RandomState(5).permutation(e.shape[1])], 4)
    ei, n = synth.grid_graph(6)
    g["grid6"] = (np.asarray(ei), n)
    g["ring1030"] = ring(1030)                                                                  # more nodes than threads in a workgroup
    return g


GRAPHS = _graphs()
SMALL = ("single", "path5_isolated", "directed_cycle_chord", "dup_selfloop_shuffled", "grid6")


def dense_lap_adj(ei, N, dtype=torch.float64):
    ei = torch.as_tensor(np.asarray(ei)).long()
    A = torch.zeros(N, N, dtype=dtype)
    for s, t in ei.t().tolist():
        if s != t:
            A[t, s] += 1.0                           # row = target, column = source
    deg = A.sum(0)                                   # over the source index: out-degree
    dis = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    return dis[:, None] * A * dis[None, :]


def dense_gcn(ei, N, dtype=torch.float64):
    ei = torch.as_tensor(np.asarray(ei)).long()
    A = torch.eye(N, dtype=dtype)
    for s, t in ei.t().tolist():
        if s != t:
            A[t, s] += 1.0
    deg = A.sum(1)                                   # over the target index: in-degree (self loop included)
    dis = deg.pow(-0.5)
    return dis[:, None] * A * dis[None, :]


def operator_dense(op, dtype=torch.float64):
    """An ops.SparseOperator (CSR by destination) as a dense [N, N] matrix."""
    W = torch.zeros(op.N, op.N, dtype=dtype)
    rp, col, w = op.rowptr.cpu().tolist(), op.col.cpu().tolist(), op.w.cpu().to(dtype)
    for i in range(op.N):
        for e in range(rp[i], rp[i + 1]):
            W[i, col[e]] += w[e]
    return W


def poly_matrices(S, K, mode):
    P = [torch.eye(S.shape[0], dtype=S.dtype)]
    if K >= 1:
        P.append(S.clone())
    for k in range(2, K + 1):
        P.append(S @ P[-1] if mode == "monomial" else 2.0 * S @ P[-1] - P[-2])
    return P


def basis_ref(S, x, K, mode):
    return torch.stack([P @ x for P in poly_matrices(S, K, mode)])


def combine_ref(S, a, c, K, mode, reverse=False):
    """a: [N, d] shared or [K+1, N, d]; c: [K+1] or None."""
    P = poly_matrices(S, K, mode)
    y = 0
    for k in range(K + 1):
        ak = a if a.dim() == 2 else a[K - k if reverse else k]
        y = y + (1.0 if c is None else c[k]) * (P[k] @ ak)
    return y


# ----------------------------------------------------------------------------- the networks (LearningFilters/models.py), dense
def bern_prop_ref(x, A, c, K):
    """models.py:326-340 on dense matrices, propagation by propagation (65 of them for K = 10), with c_i in place of
    comb(K, i) / 2^K * relu(coe_i):  out = c_0 tmp[K] + sum_i c_(i+1) L^(i+1) tmp[K-i-1], tmp[k] = (2I - L)^k x."""
    I = torch.eye(A.shape[0], dtype=A.dtype)
    L, M = I - A, I + A                             # L, and 2I - L
    tmp = [x]
    for _ in range(K):
        x = M @ x
        tmp.append(x)
    out = c[0] * tmp[K]
    for i in range(K):
        x = tmp[K - i - 1]
        x = L @ x
        for _ in range(i):
            x = L @ x
        out = out + c[i + 1] * x
    return out


def bern_conv_ref(x, A, coe, weight, bias, K):
    """models.py:316-345."""
    binom = torch.tensor([math.comb(K, i) / 2 ** K for i in range(K + 1)], dtype=A.dtype)
    return bern_prop_ref(x, A, binom * torch.relu(coe), K) @ weight + bias


def _n_layers(sd, prefix):
    return len({k.split(".")[1] for k in sd if k.startswith(prefix + ".")})


def net_ref(name, sd, x, ei, N):
    """Forward of the named network from its reference-keyed state_dict, in x's dtype."""
    dt = x.dtype
    sd = {k: v.to(dt) for k, v in sd.items()}
    h = x
    if name == "BernNet":
        A = dense_lap_adj(ei, N, dt)
        K = sd["coe"].numel() - 1
        for i in range(_n_layers(sd, "convs")):
            h = torch.relu(bern_conv_ref(h, A, sd["coe"], sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], K))
    elif name == "GPRNet":
        G = dense_gcn(ei, N, dt)
        for i in range(_n_layers(sd, "lins")):
            h = torch.relu(h @ sd[f"lins.{i}.weight"].t() + sd[f"lins.{i}.bias"])
        temp = sd["prop1.temp"]
        hidden = h * temp[0]
        for k in range(temp.numel() - 1):
            h = G @ h
            hidden = hidden + temp[k + 1] * h
        h = hidden
    elif name == "ChebNet":
        Lh = -dense_lap_adj(ei, N, dt)               # 2 L / lambda_max - I with lambda_max = 2
        for i in range(_n_layers(sd, "convs")):
            Ws = [sd[f"convs.{i}.lins.{k}.weight"] for k in range(len([q for q in sd if q.startswith(f"convs.{i}.lins.")]))]
            T0 = h
            out = T0 @ Ws[0].t()
            if len(Ws) > 1:
                T1 = Lh @ h
                out = out + T1 @ Ws[1].t()
            for W in Ws[2:]:
                T2 = 2.0 * (Lh @ T1) - T0
                out = out + T2 @ W.t()
                T0, T1 = T1, T2
            h = torch.relu(out + sd[f"convs.{i}.bias"])
    elif name == "GcnNet":
        G = dense_gcn(ei, N, dt)
        for i in range(_n_layers(sd, "convs")):
            h = torch.relu(G @ (h @ sd[f"convs.{i}.lin.weight"].t()) + sd[f"convs.{i}.bias"])
    else:
        raise ValueError(name)
    return h @ sd["fc2.weight"].t() + sd["fc2.bias"]


def net_ref_training(name, sd, feat, ei, N, y, m, lr=0.01, steps=4, dtype=torch.float64):
    """(prediction, first-step gradients, losses of `steps` Adam steps) of the restatement: training.py:132-143 with torch.optim.Adam."""
    params = {k: torch.nn.Parameter(v.detach().clone().to(dtype)) for k, v in sd.items()}
    feat, y, m = feat.to(dtype), y.to(dtype), m.to(dtype)
    with torch.no_grad():
        pre = net_ref(name, params, feat, ei, N).clone()
    opt = torch.optim.Adam(params.values(), lr=lr)
    losses, grads = [], {}
    for step in range(steps):
        opt.zero_grad()
        loss = torch.square(m * (net_ref(name, params, feat, ei, N) - y)).sum()
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().clone() for k, p in params.items()}
        opt.step()
        losses.append(float(loss.detach()))
    return pre, grads, torch.tensor(losses, dtype=torch.float64)


_FIXTURE = None


def fixture():
    """tests/golden/filter_baselines_grid6.npz (make_filter_baselines.py), loaded once: golden_util.load_filters' layout plus `lapfeat`,
    `restated` and `edge_index`."""
    global _FIXTURE
    if _FIXTURE is None:
        import os
        import golden_util as G
        fx = G.load_filters("filter_baselines_grid6")
        z = np.load(os.path.join(G.GOLDEN, "filter_baselines_grid6.npz"), allow_pickle=False)
        fx.lapfeat = {k.split("/", 1)[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lapfeat/")}
        fx.restated = tuple(str(s) for s in z["meta/restated"])
        fx.edge_index = fx.inp["edge_index"].long()
        fx.N = fx.side * fx.side
        _FIXTURE = fx
    return _FIXTURE


_REF64 = {}


def fixture_ref64(case):
    """The float64 restatement of one fixture case, computed once and shared."""
    if case not in _REF64:
        fx = fixture()
        c = fx.cases[case]
        _REF64[case] = net_ref_training(c["args"]["net"], c["sd"], c["feat"], fx.edge_index, fx.N, fx.inp["y"][:, 0:1], fx.inp["m"],
                                        lr=c["args"]["lr"])
    return _REF64[case]


NET_CASES = ("bernnet", "bernnet_eig_none", "bernnet_eig_abs", "gprnet", "chebnet", "gcnnet")


# ----------------------------------------------------------------------------- sparse float64 operators (graphs too large for dense)
def sparse_operator(ei, N, kind, transpose=False):
    """A float64 torch.sparse matrix of the 'lap' (dense_lap_adj) or 'gcn' (dense_gcn) definition, built from the edge list directly."""
    ei = torch.as_tensor(np.asarray(ei)).long().reshape(2, -1)
    keep = ei[0] != ei[1]
    s, t = ei[0][keep], ei[1][keep]
    if kind == "gcn":
        loop = torch.arange(N)
        s, t = torch.cat([s, loop]), torch.cat([t, loop])
    one = torch.ones(s.numel(), dtype=torch.float64)
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, s if kind == "lap" else t, one)
    dis = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    idx = torch.stack([s, t] if transpose else [t, s])
    return torch.sparse_coo_tensor(idx, dis[s] * dis[t], (N, N)).coalesce()


def basis_apply(W, diag_add, scale, x, K, mode):
    """P_k(S) x, S = diag_add I + scale W, by the defining recurrence on a (sparse or dense) float64 W."""
    S = lambda v: diag_add * v + scale * (W @ v)      # noqa: E731
    B = [x]
    if K >= 1:
        B.append(S(x))
    for _ in range(2, K + 1):
        B.append(S(B[-1]) if mode == "monomial" else 2.0 * S(B[-1]) - B[-2])
    return torch.stack(B)


def combine_apply(W, diag_add, scale, a, c, K, mode, reverse=False):
    """sum_k c_k P_k(S) a_k term by term: the k-th level of the basis of a_k (no Horner / Clenshaw)."""
    y = 0
    for k in range(K + 1):
        ak = a if a.dim() == 2 else a[K - k if reverse else k]
        y = y + (1.0 if c is None else c[k]) * basis_apply(W, diag_add, scale, ak, k, mode)[k]
    return y
