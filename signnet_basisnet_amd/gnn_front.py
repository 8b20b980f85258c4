"""The GINE stage's front record (csrc/gnn_front.hpp) on the host: the byte layout, a decoder for the device buffer, and a
restatement in plain torch of what a front workgroup of the plan launch writes — the graph-local CSR with in-edges by
(destination, edge id), the edge classes, the packed first-four in-edges of every node row, the (layer, class) rows of the edge
encoders and the encoder rows the lin_a stage multiplies.  Tests compare the three."""
from __future__ import annotations

import numpy as np
import torch

ROWS, EMAX, CLS, D = 64, 192, 16, 128
FR_INFO = 16
FR_ESRC = FR_INFO + 16 * ROWS
FR_ECLS = FR_ESRC + 4 * EMAX
FR_X1 = FR_ECLS + 4 * EMAX
FR_EE = FR_X1 + ROWS * D * 4


def decode(front: torch.Tensor, B: int, n_layers: int):
    """The records of a plan (plan.front, int32) as a list of dicts; an invalid record is {"valid": 0}."""
    raw = front.detach().cpu().contiguous().numpy().view(np.uint8)
    stride = raw.size // B
    out = []
    for b in range(B):
        r = raw[b * stride:(b + 1) * stride]
        hdr = r[:16].view(np.int32)
        if hdr[0] != 1:
            out.append({"valid": 0})
            continue
        n, ne, ncls = int(hdr[1]), int(hdr[2]), int(hdr[3])
        info = r[FR_INFO:FR_INFO + 16 * ROWS].view(np.int32).reshape(ROWS, 4)
        T = (n + 15) // 16
        out.append(dict(valid=1, n=n, ne=ne, ncls=ncls, info=info.copy(),
                        esrc=r[FR_ESRC:FR_ESRC + 4 * ne].view(np.int32).copy(),
                        ecls=r[FR_ECLS:FR_ECLS + 4 * ne].view(np.int32).copy(),
                        x1=r[FR_X1:FR_X1 + 16 * T * D * 4].view(np.float32).reshape(16 * T, D).copy(),
                        ee=r[FR_EE:FR_EE + n_layers * ncls * D * 4].view(np.float32).reshape(n_layers * ncls, D).copy()))
    return out


def host_record(g: int, batch, edge_index, x, edge_attr, node_table, edge_tables, lin_a=None, node_vocab=None, edge_vocab=None,
                ee_rows=39):
    """Graph g's record from CPU tensors.  node_table [V, 128]; edge_tables: one [Ve, 128] per layer; lin_a [128, 128] or None.
    -> dict like decode()'s, plus `eid` (edge id of every CSR slot) and `enc` (the encoder rows)."""
    batch = batch.reshape(-1)
    N = batch.numel()
    if N > 1 and bool((batch[1:] < batch[:-1]).any()):
        return {"valid": 0}
    nodes = (batch == g).nonzero().reshape(-1)
    n = nodes.numel()
    if n == 0 or n > ROWS:
        return {"valid": 0}
    gs = int(nodes[0])
    src, dst = edge_index[0], edge_index[1]
    eids = ((dst >= gs) & (dst < gs + n)).nonzero().reshape(-1)
    ne = eids.numel()
    if ne > EMAX:
        return {"valid": 0}
    s_in = src[eids]
    if bool(((s_in < gs) | (s_in >= gs + n)).any()):
        return {"valid": 0}
    xi = x.reshape(N, -1)[gs:gs + n, 0]
    nv = node_table.shape[0] if node_vocab is None else node_vocab
    ev_ = edge_tables[0].shape[0] if edge_vocab is None else edge_vocab
    if bool(((xi < 0) | (xi >= nv)).any()):
        return {"valid": 0}
    ea = edge_attr.reshape(edge_attr.shape[0], -1)[:, 0] if edge_attr.numel() else edge_attr.reshape(-1)
    vals = ea[eids]
    if bool(((vals < 0) | (vals >= ev_) | (vals >= 32)).any()):
        return {"valid": 0}
    # in-edges by (destination, edge id): a stable sort of the edge ids (ascending already) by destination
    order = torch.sort(dst[eids], stable=True).indices
    eid = eids[order]
    dl = (dst[eid] - gs).tolist()
    esrc = (src[eid] - gs).to(torch.int32).numpy()
    present = sorted(set(vals.tolist()))
    ncls = len(present)
    L = len(edge_tables)
    if ncls > CLS or L * ncls > ee_rows:
        return {"valid": 0}
    rank = {v: i for i, v in enumerate(present)}
    ecls = np.array([rank[int(v)] for v in ea[eid].tolist()], dtype=np.int32)
    erow = np.zeros(n + 1, dtype=np.int64)
    for d_ in dl:
        erow[d_ + 1] += 1
    erow = np.cumsum(erow)
    info = np.zeros((ROWS, 4), dtype=np.int32)
    info[:, 0] = -1
    info[:, 3] = ne
    for r in range(n):
        lo, dg = int(erow[r]), int(erow[r + 1] - erow[r])
        sr = er = 0
        for k in range(4):
            sr |= (int(esrc[lo + k]) if k < dg else ROWS) << (8 * k)
            er |= (int(ecls[lo + k]) if k < dg else 255) << (8 * k)
        info[r] = (dg, np.array(sr, dtype=np.uint32).view(np.int32), np.array(er, dtype=np.uint32).view(np.int32), lo)
    ee = torch.stack([edge_tables[l][v] for l in range(L) for v in present]).numpy() if ncls else np.zeros((0, D), np.float32)
    enc = node_table[xi]
    rec = dict(valid=1, n=n, ne=ne, ncls=ncls, info=info, esrc=esrc, ecls=ecls, ee=ee, eid=eid, enc=enc, gs=gs)
    if lin_a is not None:
        T = (n + 15) // 16
        x1 = torch.zeros(16 * T, D, dtype=torch.float64)
        x1[:n] = enc.double() @ lin_a.double().t()
        rec["x1"] = x1
        rec["x1_abs"] = torch.zeros(16 * T, D, dtype=torch.float64)
        rec["x1_abs"][:n] = enc.double().abs() @ lin_a.double().abs().t()
    return rec
