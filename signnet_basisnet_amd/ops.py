"""Thin Python wrappers over the C ABI (one per entry point of include/signnet_hip.h).

Each wrapper validates dtype/contiguity, allocates the output with torch (device memory is
PyTorch's job here), and launches on torch's current stream.  No arithmetic happens in Python.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import (EPI_AFFINE, EPI_BIAS, EPI_LEAKY, EPI_RELU, EPI_RELU_PRE, EPI_RESIDUAL, EPI_RESIDUAL_PRE, check, lib, ptr,
                   require_cuda, stream)

__all__ = ["KernelTimer", "KERNEL_ROOFLINE", "GraphPlan", "PlanBins", "build_plan", "pack_eig", "pack_weight", "gin_aggregate", "gine_aggregate",
           "masked_linear", "masked_colstats", "masked_affine", "masked_layernorm", "set_attention",
           "slot_sum", "embedding_sum", "segment_pool", "segment_max", "PackedLinear",
           "EPI_BIAS", "EPI_RELU_PRE", "EPI_AFFINE", "EPI_RELU", "EPI_RESIDUAL"]


# ----------------------------------------------------------------------------- kernel timing (bench.py)
class _NoSpan:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NOSPAN = _NoSpan()
_active_timer = None


class _Span:
    __slots__ = ("timer", "name", "e0")

    def __init__(self, timer, name):
        self.timer, self.name = timer, name

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e0.record()          # torch's current stream == the stream the kernel is launched on
        return self

    def __exit__(self, *a):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.timer.spans.append((self.name, self.e0, e1))
        return False


class KernelTimer:
    """HIP-event timing of C-ABI launches on torch's current stream (the stream every launch uses).
    `only` restricts recording to the named entry points and `stride` to every stride-th launch of each, so the timed
    region is barely perturbed (an event pair costs the stream ~4-5 us of marker packets)."""

    def __init__(self, only=None, stride=1):
        self.only = set(only) if only else None
        self.stride = max(1, int(stride))
        self.seen = {}
        self.spans = []

    def __enter__(self):
        global _active_timer
        _active_timer = self
        return self

    def __exit__(self, *a):
        global _active_timer
        _active_timer = None
        return False

    def summary(self):
        torch.cuda.synchronize()
        acc = {}
        for name, e0, e1 in self.spans:
            n, t = acc.get(name, (0, 0.0))
            acc[name] = (n + 1, t + e0.elapsed_time(e1))
        return {k: (n, t / n) for k, (n, t) in acc.items()}


def _span(name):
    t = _active_timer
    if t is None or (t.only is not None and name not in t.only):
        return _NOSPAN
    if t.stride > 1:
        k = t.seen.get(name, 0)
        t.seen[name] = k + 1
        if k % t.stride:
            return _NOSPAN
    return _Span(t, name)


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


@dataclass
class PlanBins:
    """Work bins of the fused phi / rho stages (device arrays written by sn_batch_plan; see signnet_hip.h)."""
    phi_bin_col: torch.Tensor    # int32 [phi_max_bins]
    phi_max_bins: int
    phi_col_bin0: torch.Tensor   # int32 [B+1]
    phi_col_mem: torch.Tensor    # int32 [B*8]
    phi_col_off: torch.Tensor    # int32 [B*8]
    rho_bin0: torch.Tensor       # int32 [B+1]
    meta: torch.Tensor           # int32 [8]
    cstruct: object              # ctypes mirror (sn_plan_bins) holding the device pointers
    phi_bin_mem: torch.Tensor = None   # int32 [phi_max_bins * 16] member records of every bin (meta[7] bins)


@dataclass
class GraphPlan:
    """Device-resident structure of one batch (built once per batch by `build_plan`)."""
    N: int
    B: int
    E: int
    kmax: int
    graph_ptr: torch.Tensor   # int32 [B+1]
    node_graph: torch.Tensor  # int32 [N]
    nvalid: torch.Tensor      # int32 [N]   valid eigenvector slots per node
    evoff: torch.Tensor       # int64 [B+1] offset of each graph's n_b x n_b eigenvector block
    rowptr: torch.Tensor      # int32 [N+1] dst-sorted CSR
    col: torch.Tensor         # int32 [E]   source node of each in-edge
    eperm: torch.Tensor       # int32 [E]   original edge id of each CSR slot
    status: torch.Tensor      # int32 [8]   [err bits, max nodes/graph, max in-degree, fused-stage flags, gnn completion counter,
                              #              embedding index out of range (layer path), -, -]
    bins: PlanBins | None
    flags: torch.Tensor = None   # status (+ bins meta) as one contiguous block
    front: torch.Tensor = None   # int32 view of the batch's GINE-stage front records (sn_batch_plan_front), or None

    def check(self):
        """Synchronising validity check (raises on malformed batches)."""
        return check_plan_status(self.status)


def check_plan_status(status):
    """GraphPlan.check() on the status words alone (one host read): what a forward that deferred its check hands to check_train()."""
    st = status.tolist()
    if st[0]:
        bits = [n for b, n in ((1, "batch not sorted"), (2, "graph id out of range"),
                               (4, "edge endpoint out of range"), (8, "edge crosses graphs")) if st[0] & b]
        raise ValueError("malformed graph batch: " + ", ".join(bits))
    if st[5] or (st[3] & 4):
        raise IndexError(EMBEDDING_INDEX_ERROR)
    return st


class DeferredStatus:
    """Mixin of the plain models of the PyG trees (pyg.GNN, pyg_baselines.NetGINE): where the differentiable forward's status words go."""

    def _finish_train(self, plan):
        """The forward's one host read — malformed batch, an id outside its embedding table — or, under `_defer_status` (a captured
        step must not synchronise), the status words handed to check_train()."""
        if getattr(self, "_defer_status", False):
            self._train_status = plan.status
        else:
            plan.check()

    def check_train(self):
        """What the last differentiable forward under `_defer_status` left unread: raises what plan.check() raises in the eager step."""
        st, self._train_status = getattr(self, "_train_status", None), None
        if st is not None:
            check_plan_status(st)


class _PlanBinsC(C.Structure):
    _fields_ = [("phi_bin_col", C.c_void_p), ("phi_max_bins", C.c_int64), ("phi_col_bin0", C.c_void_p),
                ("phi_col_mem", C.c_void_p), ("phi_col_off", C.c_void_p), ("rho_bin0", C.c_void_p), ("meta", C.c_void_p),
                ("node_graph", C.c_void_p), ("phi_bin_mem", C.c_void_p)]


class _PlanEarlyC(C.Structure):
    _fields_ = [("node_ids", C.c_void_p), ("n_node_ids", C.c_int64), ("node_vocab", C.c_int64),
                ("edge_ids", C.c_void_p), ("n_edge_ids", C.c_int64), ("edge_vocab", C.c_int64),
                ("max_graph_edges", C.c_int), ("reserved", C.c_int), ("host", C.c_void_p)]


class EarlyReport:
    """The batch's flags as sn_batch_plan_ex reports them to pinned host memory while the rest of the forward is still running
    (include/signnet_hip.h: sn_plan_early).  `wait()` polls the four done words (the plan is the first ~20 us of a forward: they
    are normally set by the time the host has queued the stage kernels) and returns the flag words as a list."""
    ERR, NMAX, DEGMAX, EDGES, PHI, RHO, IDS, DONE = 0, 1, 2, 3, 4, 5, 6, 8
    _pool = []
    _made = 0           # pinned slots ever allocated (= slots in the pool + slots of reports not yet released)

    def __init__(self):
        # (a pooled slot keeps its ctypes mirror: arming it again only rewrites the fields — the serving mode arms one per forward)
        if EarlyReport._pool:
            self.t, self.v, self._cbuf = EarlyReport._pool.pop()
        else:
            self.t = torch.zeros(16, dtype=torch.int32, pin_memory=True)
            self.v = self.t.numpy()
            self._cbuf = _PlanEarlyC(None, 0, 0, None, 0, 0, 0, 0, self.t.data_ptr())
            EarlyReport._made += 1
        self.v[:] = 0
        self.cstruct = None
        self._keep = None
        self.kword = 0      # serving mode: the slot count an all-eigenvector forward sized its tensors with (0: max_k given)

    def poll(self):
        """The 16 words as a list once all four done words are set, else None (never blocks; one read of the pinned words)."""
        w = self.v.tolist()
        return w if (w[8] and w[9] and w[10] and w[11]) else None

    def done(self):
        """All four done words are set (never blocks): the plan launch has written everything it writes to this slot."""
        return self.poll() is not None

    @classmethod
    def words_bad(cls, fl, kword=0):
        """Whether the polled words report anything check_last() raises for (the clean case: no list is built)."""
        return bool(fl[0] or fl[3] or fl[4] or fl[5] or fl[6] or (kword and fl[1] > kword))

    def status_words(self, fl=None):
        """The report in the layout of the stage kernels' flag block ([status(8) | bins meta(8)] + the host's slot-count word, what
        SignNetGNN._flags_bad / _flags_error judge) — call once done().  status[3] carries the GINE stage's bits as that stage would
        have set them: 1 a graph beyond the node / in-edge limits, 4 a feature id outside its table, 8 a graph without nodes."""
        if fl is None:
            fl = self.v.tolist()
        w = [0] * 32
        w[0], w[1], w[2] = fl[self.ERR], fl[self.NMAX], fl[self.DEGMAX]
        w[3] = (1 if (fl[self.EDGES] or (fl[self.PHI] & 1)) else 0) | (4 if fl[self.IDS] else 0) | (fl[self.PHI] & 8)
        w[9], w[13] = fl[self.PHI] & 5, fl[self.RHO]
        w[24] = int(self.kword)
        return w

    def arm(self, node_ids=None, node_vocab=0, edge_ids=None, edge_vocab=0, max_graph_edges=0):
        self._keep = (node_ids, edge_ids)
        c = self._cbuf
        c.node_ids, c.n_node_ids, c.node_vocab = ptr(node_ids), 0 if node_ids is None else node_ids.numel(), int(node_vocab)
        c.edge_ids, c.n_edge_ids, c.edge_vocab = ptr(edge_ids), 0 if edge_ids is None else edge_ids.numel(), int(edge_vocab)
        c.max_graph_edges = int(max_graph_edges)
        self.cstruct = c
        return self

    def wait(self, timeout_s=5.0):
        w = self.poll()
        if w is not None:
            return w[:8]
        v = self.v
        if not (v[8] and v[9] and v[10] and v[11]):
            import time
            t_end = time.perf_counter() + timeout_s
            while not (v[8] and v[9] and v[10] and v[11]):
                if time.perf_counter() > t_end:
                    torch.cuda.synchronize()
                    if not (v[8] and v[9] and v[10] and v[11]):
                        raise RuntimeError("sn_batch_plan_ex did not report its flags")
        return v[:8].tolist()

    def wait_nmax(self):
        """Only the largest graph (the rho-bins workgroup's word): what the all-eigenvector mode sizes its tensors from."""
        v = self.v
        if not v[10]:
            import time
            t_end = time.perf_counter() + 5.0
            while not v[10]:
                if time.perf_counter() > t_end:
                    torch.cuda.synchronize()
                    if not v[10]:
                        raise RuntimeError("sn_batch_plan_ex did not report the largest graph")
        return int(v[1])

    def release(self):
        """Back to the pool (only once the launch that writes it has completed: after wait())."""
        self._keep = self.cstruct = None
        EarlyReport._pool.append((self.t, self.v, self._cbuf))


_early_ok = {}      # (N, E, B) -> sn_batch_plan_early_supported: a serving loop asks for the same shapes at every forward


def early_supported(N: int, E: int, B: int) -> bool:
    key = (N, E, B)
    r = _early_ok.get(key)
    if r is None:
        if len(_early_ok) >= 4096:
            _early_ok.clear()
        r = _early_ok[key] = bool(lib().sn_batch_plan_early_supported(int(N), int(E), int(B)))
    return r


def build_plan(batch: torch.Tensor, edge_index: torch.Tensor, num_graphs: int, kmax: int = 0, bins: bool = False,
               early: "EarlyReport | None" = None, columns: bool = False, counts: torch.Tensor = None, front=None) -> GraphPlan:
    """bins=True also lays out the work bins of the fused stages (same launch, no host sync).  early: an armed EarlyReport — the
    batch's flags are also written to its pinned buffer by the plan kernel itself (one-launch plans only: early_supported()).
    columns=True: the planner's column arrays (phi_bin_col, phi_col_bin0, phi_col_mem, phi_col_off) are written too — the stage kernels
    walk the per-bin member records (phi_bin_mem) only, so the forward leaves them out.
    counts: the device count block of a padded batch (sn_bucket_pack): graphs >= counts[2] get no eigenvector slot (sn_batch_plan_padded).
    front: (sn_gnn_params, x [N, F] int64, edge_attr [E, F_e] int64, bytes per record) of the fused GINE stage that will consume this
    plan (fused.GnnPlan.front_args): the launch also writes the stage's front records (plan.front); needs bins and a one-launch plan."""
    require_cuda(batch, edge_index)
    if batch.dtype != torch.int64 or edge_index.dtype != torch.int64:
        raise ValueError("build_plan: batch and edge_index must be int64 (the reference's index dtype)")
    batch = batch.contiguous()
    edge_index = edge_index.contiguous()
    N, E, B = batch.numel(), edge_index.shape[1] if edge_index.numel() else 0, int(num_graphs)
    dev = batch.device
    # one int32 arena, carved into the plan arrays (single allocation per batch)
    sizes = [B + 1, N, N, N + 1, E, E, N + 8, 8]          # status last: [status(8) | bins meta(8)] is one 16-int block
    mb = 0
    if bins:
        mb = int(lib().sn_phi_bins_bound(B, int(kmax)))
        sizes += [8, mb if columns else 0, (B + 1) if columns else 0, (8 * B) if columns else 0, (8 * B) if columns else 0, B + 1, 16 * mb]
    if front is not None:
        if not bins or counts is not None or not early_supported(N, E, B) or B == 0:
            front = None
        else:
            sizes += [B * (int(front[3]) // 4)]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + ((s + 3) // 4) * 4)
    arena = torch.empty(offs[-1], dtype=torch.int32, device=dev)
    parts = [arena[offs[i]:offs[i] + sizes[i]] for i in range(len(sizes))]
    graph_ptr, node_graph, nvalid, rowptr, col, eperm, scratch, status = parts[:8]
    evoff = torch.empty(B + 1, dtype=torch.int64, device=dev)
    pb = None
    if bins:
        meta, bc, cb0, mem, off, rb0, bmem = parts[8:15]
        if columns:
            cs = _PlanBinsC(bc.data_ptr(), mb, cb0.data_ptr(), mem.data_ptr(), off.data_ptr(), rb0.data_ptr(), meta.data_ptr(),
                            node_graph.data_ptr(), bmem.data_ptr())
        else:
            bc = cb0 = mem = off = None
            cs = _PlanBinsC(None, mb, None, None, None, rb0.data_ptr(), meta.data_ptr(), node_graph.data_ptr(), bmem.data_ptr())
        pb = PlanBins(bc, mb, cb0, mem, off, rb0, meta, cs, bmem)
    if counts is not None:
        with _span("sn_batch_plan_padded"):
            check(lib().sn_batch_plan_padded(ptr(batch), N, B, ptr(edge_index), E, int(kmax), ptr(graph_ptr), ptr(node_graph),
                                             ptr(nvalid), ptr(evoff), ptr(rowptr), ptr(col), ptr(eperm), ptr(status),
                                             C.byref(pb.cstruct) if pb is not None else None, ptr(scratch),
                                             C.byref(early.cstruct) if early is not None else None, ptr(counts), stream()),
                  "sn_batch_plan_padded")
    elif front is not None:
        gp, fx, fe, _ = front
        with _span("sn_batch_plan"):
            check(lib().sn_batch_plan_front(ptr(batch), N, B, ptr(edge_index), E, int(kmax), ptr(graph_ptr), ptr(node_graph),
                                            ptr(nvalid), ptr(evoff), ptr(rowptr), ptr(col), ptr(eperm), ptr(status),
                                            C.byref(pb.cstruct), ptr(scratch), C.byref(early.cstruct) if early is not None else None,
                                            C.byref(gp), ptr(fx), fx.shape[1], ptr(fe), fe.shape[1], ptr(parts[-1]), stream()),
                  "sn_batch_plan_front")
    else:
        with _span("sn_batch_plan"):
            check(lib().sn_batch_plan_ex(ptr(batch), N, B, ptr(edge_index), E, int(kmax), ptr(graph_ptr), ptr(node_graph),
                                         ptr(nvalid), ptr(evoff), ptr(rowptr), ptr(col), ptr(eperm), ptr(status),
                                         C.byref(pb.cstruct) if pb is not None else None, ptr(scratch),
                                         C.byref(early.cstruct) if early is not None else None, stream()), "sn_batch_plan")
    plan = GraphPlan(N, B, E, int(kmax), graph_ptr, node_graph, nvalid, evoff, rowptr, col, eperm, status, pb)
    plan.flags = arena[offs[7]:offs[7] + 16] if bins else status      # [status(8) | meta(8)] contiguous
    if front is not None:
        plan.front = parts[-1]
    return plan


def pack_eig(plan: GraphPlan, eigen_vectors, eigen_values, K: int, want_values: bool):
    require_cuda(eigen_vectors)
    ev = _f32c(eigen_vectors, "eigen_vectors")
    x0 = torch.empty(plan.N, K, dtype=torch.float32, device=ev.device)
    s0 = torch.empty_like(x0) if want_values else None
    es = _f32c(eigen_values, "eigen_values") if want_values else None
    with _span("sn_pack_eig_f32"):
        check(lib().sn_pack_eig_f32(ptr(ev), ptr(es), ptr(plan.graph_ptr), ptr(plan.node_graph), ptr(plan.nvalid),
                                    ptr(plan.evoff), plan.N, K, ptr(x0), ptr(s0), stream()), "sn_pack_eig_f32")
    return x0, s0


PHI_BIN_ROWS = 64     # SN_PHI_BIN_ROWS


def bn_fold(bn, c_pad=None):
    """Eval-mode nn.BatchNorm1d -> (scale, shift), zero padded to c_pad channels."""
    Cc = bn.num_features
    cp = Cc if c_pad is None else int(c_pad)
    dev = bn.running_mean.device
    require_cuda(bn.running_mean)
    scale = torch.empty(cp, dtype=torch.float32, device=dev)
    shift = torch.empty(cp, dtype=torch.float32, device=dev)
    w = bn.weight.detach() if bn.affine else None
    b = bn.bias.detach() if bn.affine else None
    check(lib().sn_bn_fold_f32(ptr(w), ptr(b), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps), Cc, cp,
                               ptr(scale), ptr(shift), stream()), "sn_bn_fold_f32")
    return scale, shift


def pad_vec(v, c_pad):
    """Zero-pad a per-channel vector to c_pad floats (a copy, no arithmetic)."""
    v = v.detach().reshape(-1)
    out = torch.zeros(c_pad, dtype=torch.float32, device=v.device)
    out[:v.numel()].copy_(v)
    return out


def packed_floats(d_out: int, d_in: int) -> int:
    return int(lib().sn_packed_weight_floats(d_out, d_in))


def pack_weight(W: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """nn.Linear weight [d_out, d_in] -> MFMA fragment order (see csrc/common.hpp)."""
    require_cuda(W)
    if W.dtype != torch.float32 or W.dim() != 2 or W.stride(1) != 1:
        raise ValueError("pack_weight: expected a float32 [d_out, d_in] matrix with unit inner stride")
    d_out, d_in = W.shape
    n = packed_floats(d_out, d_in)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=W.device)
    check(lib().sn_pack_weight_f32(ptr(W), d_out, d_in, W.stride(0), ptr(out), stream()), "sn_pack_weight_f32")
    return out


def pack_weight_t(W: torch.Tensor) -> torch.Tensor:
    """Packed W^T of a [rows, cols] matrix, read in place (no transposed copy): the weight of dX = dY @ W."""
    require_cuda(W)
    if W.dtype != torch.float32 or W.dim() != 2 or W.stride(1) != 1:
        raise ValueError("pack_weight_t: expected a float32 matrix with unit inner stride")
    rows, cols = W.shape
    out = torch.empty(packed_floats(cols, rows), dtype=torch.float32, device=W.device)
    check(lib().sn_pack_weight_t_f32(ptr(W), rows, cols, W.stride(0), ptr(out), stream()), "sn_pack_weight_t_f32")
    return out


def pack_split(W: torch.Tensor, e0=None, e1=None, e2=None) -> torch.Tensor:
    """nn.Linear weight [d_out, d_in] (+ up to three per-output-channel epilogue vectors) -> the split-packed buffer
    of sn_pack_split_f32: exact 3 x bf16 significand split of every weight, fragment order of the fused phi / rho
    kernels (csrc/fused_common.hpp).  Returns a uint8 tensor that owns the buffer."""
    require_cuda(W)
    if W.dtype != torch.float32 or W.dim() != 2 or W.stride(1) != 1:
        raise ValueError("pack_split: expected a float32 [d_out, d_in] matrix with unit inner stride")
    d_out, d_in = W.shape
    vecs = []
    for e in (e0, e1, e2):
        if e is not None:
            e = e.detach().to(device=W.device, dtype=torch.float32).contiguous()
            if e.numel() < d_out:
                raise ValueError("pack_split: epilogue vector shorter than d_out")
        vecs.append(e)
    out = torch.empty(int(lib().sn_split_packed_bytes(d_out, d_in)), dtype=torch.uint8, device=W.device)
    check(lib().sn_pack_split_f32(ptr(W), d_out, d_in, W.stride(0), ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), ptr(out),
                                  stream()), "sn_pack_split_f32")
    return out


# matmul precision names of the fused eval stages -> SN_PREC_* (include/signnet_hip.h; documented in fused.py)
PRECISIONS = {"highest": 0, "high": 1, "medium": 2}


def mlp_chain(x, weights, d_pad, d_out, nvalid=None, K=0, precision="highest", d_in=None):
    """A whole MLP over the rows of x in one launch (sn_mlp_chain_prec_f32): y = W_{L-1} relu(... relu(W_0 x + b_0) ...) + b_{L-1}.
    weights: split-packed Linears (pack_split of the [d_pad, d_pad] zero-padded matrix, e0 = bias), d_pad a multiple of 16 in
    [48, 128].  x: [R, d_in] rows, or with nvalid (int32 [R]) the [R*K, d_in] slot rows whose first nvalid[r] are summed into row r.
    precision: "highest" | "high" | "medium", the product set of every Linear of the chain (every width is built).  -> [R, d_out]."""
    import ctypes as C
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)} (got {precision!r})")
    require_cuda(x)
    x = _f32c(x, "mlp_chain x")
    if x.dim() != 2:
        raise ValueError("mlp_chain: x must be [rows, d_in]")
    d_in = x.shape[1] if d_in is None else int(d_in)
    if nvalid is None:
        R = x.shape[0]
    else:
        if nvalid.dtype != torch.int32 or K <= 0 or x.shape[0] != nvalid.numel() * K:
            raise ValueError("mlp_chain: nvalid must be int32 [R] with x of R*K rows")
        R = nvalid.numel()
    ws = (C.c_void_p * len(weights))(*[ptr(w) for w in weights])
    y = torch.empty(R, d_out, dtype=torch.float32, device=x.device)
    with _span("sn_mlp_chain_f32"):
        check(lib().sn_mlp_chain_prec_f32(ptr(x), x.stride(0), R, d_in, ptr(nvalid), int(K), ws, len(weights), int(d_pad), ptr(y),
                                          d_out, d_out, PRECISIONS[precision], stream()), "sn_mlp_chain_prec_f32")
    return y


@dataclass
class PackedLinear:
    wp: torch.Tensor
    d_out: int
    d_in: int
    bias: torch.Tensor | None = None


def gin_aggregate(x, plan: GraphPlan, eps=None, negate=False, slab=False):
    """x [N, ...] -> (1+eps) x_i + sum_{j->i} x_j over the node axis (trailing dims flattened)."""
    require_cuda(x)
    x = _f32c(x, "x")
    N = x.shape[0]
    F = x.numel() // max(N, 1)
    out = torch.empty_like(x)
    if slab:
        with _span("sn_gin_aggregate_slab_f32"):
            check(lib().sn_gin_aggregate_slab_f32(ptr(x), ptr(out), N, F, plan.B, ptr(plan.graph_ptr), ptr(plan.rowptr),
                                                  ptr(plan.col), ptr(eps), int(negate), stream()),
                  "sn_gin_aggregate_slab_f32")
    else:
        with _span("sn_gin_aggregate_f32"):
            check(lib().sn_gin_aggregate_f32(ptr(x), ptr(out), N, F, ptr(plan.rowptr), ptr(plan.col), ptr(eps),
                                             int(negate), stream()), "sn_gin_aggregate_f32")
    return out


def doubled_plan(plan: GraphPlan):
    """The CSR of two disjoint copies of the batch (nodes N..2N-1 = the second copy): the phi(+x) / phi(-x) passes stacked group-major
    aggregate in ONE launch over [2N, K*d].  Index plumbing only (one launch: sn_plan_double_i32), kept on the plan."""
    d = getattr(plan, "_doubled", None)
    if d is None:
        import types
        E = plan.col.numel()
        rowptr2 = torch.empty(2 * plan.N + 1, dtype=torch.int32, device=plan.rowptr.device)
        col2 = torch.empty(2 * E, dtype=torch.int32, device=plan.rowptr.device)
        check(lib().sn_plan_double_i32(ptr(plan.rowptr), ptr(plan.col), plan.N, E, ptr(rowptr2), ptr(col2), stream()), "sn_plan_double_i32")
        d = types.SimpleNamespace(N=2 * plan.N, B=2 * plan.B, E=2 * E, rowptr=rowptr2, col=col2)
        plan._doubled = d
    return d


def gine_aggregate(x, ea, plan: GraphPlan, eps=None):
    require_cuda(x, ea)
    x, ea = _f32c(x, "x"), _f32c(ea, "edge_attr")
    if ea.shape != (plan.E, x.shape[1]):
        raise ValueError("gine_aggregate: edge features must be [E, C] with C == x.shape[1]")
    out = torch.empty_like(x)
    with _span("sn_gine_aggregate_f32"):
        check(lib().sn_gine_aggregate_f32(ptr(x), ptr(ea), ptr(out), x.shape[0], x.shape[1], ptr(plan.rowptr),
                                          ptr(plan.col), ptr(plan.eperm), ptr(eps), stream()), "sn_gine_aggregate_f32")
    return out


def gated_aggregate(Ah, Bh, Dh, Eh, Ce, plan: GraphPlan, want_den=False, epilogue=None):
    """GatedGCN message passing (gatedgcn_layer.py:51-56): -> (h [N,C], e [E,C][, den [N,C]]).
    Ah/Bh/Dh/Eh may be column blocks (views) of one [N, 4C] tensor.  epilogue = (h_scale, h_shift, e_scale, e_shift, h_res, e_res):
    eval-mode BatchNorm + ReLU + residual fused into the same pass (residuals may be None)."""
    require_cuda(Ah, Bh, Dh, Eh, Ce)
    N, Cc = Ah.shape
    ldn = Ah.stride(0)
    for t, n in ((Ah, "Ah"), (Bh, "Bh"), (Dh, "Dh"), (Eh, "Eh")):
        if t.dtype != torch.float32 or t.shape != (N, Cc) or t.stride(1) != 1 or t.stride(0) != ldn:
            raise ValueError(f"gated_aggregate: {n} must be a float32 [N, C] row block with the common row stride")
    Ce = _f32c(Ce, "Ce")
    if Ce.shape != (plan.E, Cc):
        raise ValueError("gated_aggregate: Ce must be [E, C]")
    h = torch.empty(N, Cc, dtype=torch.float32, device=Ah.device)
    e = torch.empty_like(Ce)
    den = torch.empty_like(h) if want_den else None
    ep = epilogue if epilogue is not None else (None,) * 6
    with _span("sn_gated_aggregate_f32"):
        check(lib().sn_gated_aggregate_f32(ptr(Ah), ptr(Bh), ptr(Dh), ptr(Eh), ldn, ptr(Ce), N, Cc, ptr(plan.rowptr), ptr(plan.col),
                                           ptr(plan.eperm), ptr(h), ptr(e), ptr(den), *(ptr(t) for t in ep), stream()),
              "sn_gated_aggregate_f32")
    return (h, e, den) if want_den else (h, e)


def masked_linear(x, pl: PackedLinear, nvalid=None, K=0, *, scale=None, shift=None, relu_pre=False, relu=False,
                  residual=None, use_bias=True, out=None, residual_pre=False, leaky=False):
    """y = epilogue(x @ W^T); x is a row matrix [..., d_in] (leading dims flattened to rows).
    residual_pre: the residual is added right behind the bias, in front of relu_pre / the affine / relu (BatchNorm(x + Linear(h)))."""
    require_cuda(x)
    x = _f32c(x, "x")
    if x.shape[-1] != pl.d_in:
        raise ValueError(f"masked_linear: x has {x.shape[-1]} channels, weight expects {pl.d_in}")
    R = x.numel() // pl.d_in
    flags = 0
    bias = pl.bias if use_bias else None
    if bias is not None:
        flags |= EPI_BIAS
    if relu_pre:
        flags |= EPI_RELU_PRE
    if scale is not None:
        flags |= EPI_AFFINE
    if relu:
        flags |= EPI_RELU
    if leaky:                   # LeakyReLU(0.01) in RELU's place (then + residual)
        flags |= EPI_LEAKY
    if residual is not None:
        flags |= EPI_RESIDUAL_PRE if residual_pre else EPI_RESIDUAL
        residual = _f32c(residual, "residual")
    if out is None:
        out = torch.empty(*x.shape[:-1], pl.d_out, dtype=torch.float32, device=x.device)
    if R == 0:
        return out
    with _span("sn_masked_linear_f32"):
        check(lib().sn_masked_linear_f32(ptr(x), pl.d_in, R, pl.d_in, ptr(pl.wp), pl.d_out, ptr(bias), ptr(nvalid),
                                         int(K), flags, ptr(scale), ptr(shift), ptr(residual), pl.d_out, ptr(out),
                                         pl.d_out, stream()), "sn_masked_linear_f32")
    return out


def linear_block_bias(x, pl: PackedLinear, block_bias, rows_per_block, *, scale=None, shift=None, relu_pre=False, relu=False):
    """y = epilogue(x @ W^T + b + block_bias[row // rows_per_block]): a Linear whose bias differs per block of consecutive rows (the
    equivariant 1->1 layers: Linear over cat[x, mean of the row's matrix] without the concatenation)."""
    require_cuda(x)
    x, block_bias = _f32c(x, "x"), _f32c(block_bias, "block_bias")
    R = x.numel() // pl.d_in
    if block_bias.shape[-1] != pl.d_out or block_bias.numel() // pl.d_out * int(rows_per_block) < R:
        raise ValueError("linear_block_bias: one bias row per block of rows expected")
    flags = (EPI_BIAS if pl.bias is not None else 0) | (EPI_RELU_PRE if relu_pre else 0) | (EPI_AFFINE if scale is not None else 0) | \
            (EPI_RELU if relu else 0)
    out = torch.empty(*x.shape[:-1], pl.d_out, dtype=torch.float32, device=x.device)
    with _span("sn_masked_linear_f32"):
        check(lib().sn_masked_linear_blockbias_f32(ptr(x), pl.d_in, R, pl.d_in, ptr(pl.wp), pl.d_out, ptr(pl.bias), ptr(block_bias),
                                                   int(rows_per_block), pl.d_out, flags, ptr(scale), ptr(shift), ptr(out), pl.d_out, stream()),
              "sn_masked_linear_blockbias_f32")
    return out


def masked_colstats(x, nvalid=None, K=0):
    """Per-channel mean / biased variance over the valid rows of a row matrix [..., C]."""
    require_cuda(x)
    x = _f32c(x, "x")
    Cc = x.shape[-1]
    R = x.numel() // Cc
    nb = int(lib().sn_colstats_blocks(R))
    mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
    var = torch.empty_like(mean)
    count = torch.empty(1, dtype=torch.float32, device=x.device)
    scratch = torch.empty(nb * Cc + nb, dtype=torch.float32, device=x.device)
    check(lib().sn_masked_colstats_f32(ptr(x), Cc, R, Cc, ptr(nvalid), int(K), ptr(mean), ptr(var), ptr(count),
                                       ptr(scratch), stream()), "sn_masked_colstats_f32")
    return mean, var, count


# `num_batches_tracked += 1` is one tiny launch per BatchNorm site; a training forward touches dozens.  Inside `batched_bn_counters()`
# the increments are collected and applied by one multi-tensor add at exit (same buffers, same values).
_BN_PENDING = None


def _count_batch(bn, n=1):
    if _BN_PENDING is None:
        bn.num_batches_tracked += n
    else:
        t = bn.num_batches_tracked
        ent = _BN_PENDING.get(id(t))
        if ent is None:
            _BN_PENDING[id(t)] = [t, n]
        else:
            ent[1] += n              # (one entry per buffer: a tensor listed twice in a foreach add is NOT reliably incremented twice)


class batched_bn_counters:
    def __enter__(self):
        global _BN_PENDING
        self._outer = _BN_PENDING
        if self._outer is None:
            _BN_PENDING = {}
        return self

    def __exit__(self, *exc):
        global _BN_PENDING
        if self._outer is None:
            pending, _BN_PENDING = _BN_PENDING, None
            if pending:
                with torch.no_grad():
                    torch._foreach_add_([e[0] for e in pending.values()], [e[1] for e in pending.values()])
        return False


def bn_train_stats(x, bn, nvalid=None, K=0):
    """Batch statistics of a train-mode BatchNorm1d over the valid rows of x, the folded (scale, shift), rstd, and the
    running-statistics side effect on `bn` — one C call (sn_bn_train_stats_f32).  -> (mean, var, rstd, scale, shift, count)."""
    require_cuda(x)
    x = _f32c(x, "x")
    Cc = x.shape[-1]
    R = x.numel() // Cc
    nb = int(lib().sn_colstats_blocks(R))
    out = torch.empty(5 * Cc + 1, dtype=torch.float32, device=x.device)
    mean, var, rstd, scale, shift = (out[i * Cc:(i + 1) * Cc] for i in range(5))
    count = out[5 * Cc:]
    scratch = torch.empty(nb * Cc + nb, dtype=torch.float32, device=x.device)
    track = bn.track_running_stats and bn.running_mean is not None
    if track and bn.momentum is None:
        raise NotImplementedError("BatchNorm1d(momentum=None) (cumulative moving average) is not supported")
    g = None if bn.weight is None else bn.weight.detach()
    b = None if bn.bias is None else bn.bias.detach()
    check(lib().sn_bn_train_stats_f32(ptr(x), Cc, R, Cc, ptr(nvalid), int(K), ptr(g), ptr(b), float(bn.eps),
                                      float(bn.momentum or 0.0), ptr(bn.running_mean) if track else None,
                                      ptr(bn.running_var) if track else None, ptr(mean), ptr(var), ptr(rstd), ptr(scale), ptr(shift),
                                      ptr(count), ptr(scratch), stream()), "sn_bn_train_stats_f32")
    if track:
        _count_batch(bn)
    return mean, var, rstd, scale, shift, count


def linear_bn_train(x, pl: PackedLinear, bn, nvalid=None, K=0):
    """z = x @ W^T + b (masked) and the train-mode BatchNorm1d statistics of z in one C call (sn_linear_bn_train_f32): for large row
    counts the moments come out of the Linear kernel's accumulators.  -> (z, mean, var, rstd, scale, shift, count); updates bn's
    running statistics like bn_train_stats."""
    require_cuda(x)
    x = _f32c(x, "x")
    if x.shape[-1] != pl.d_in:
        raise ValueError(f"linear_bn_train: x has {x.shape[-1]} channels, weight expects {pl.d_in}")
    R = x.numel() // pl.d_in
    Cc = pl.d_out
    z = torch.empty(*x.shape[:-1], Cc, dtype=torch.float32, device=x.device)
    out = torch.empty(5 * Cc + 1, dtype=torch.float32, device=x.device)
    mean, var, rstd, scale, shift = (out[i * Cc:(i + 1) * Cc] for i in range(5))
    count = out[5 * Cc:]
    scratch = torch.empty(max(int(lib().sn_linear_bn_scratch_floats(R, pl.d_in, Cc)), 1), dtype=torch.float32, device=x.device)
    track = bn.track_running_stats and bn.running_mean is not None
    if track and bn.momentum is None:
        raise NotImplementedError("BatchNorm1d(momentum=None) (cumulative moving average) is not supported")
    g = None if bn.weight is None else bn.weight.detach()
    b = None if bn.bias is None else bn.bias.detach()
    with _span("sn_linear_bn_train_f32"):
        check(lib().sn_linear_bn_train_f32(ptr(x), pl.d_in, R, pl.d_in, ptr(pl.wp), Cc, ptr(pl.bias), ptr(nvalid), int(K), ptr(z), Cc,
                                           ptr(g), ptr(b), float(bn.eps), float(bn.momentum or 0.0),
                                           ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None, ptr(mean),
                                           ptr(var), ptr(rstd), ptr(scale), ptr(shift), ptr(count), ptr(scratch), stream()),
              "sn_linear_bn_train_f32")
    if track:
        _count_batch(bn)
    return z, mean, var, rstd, scale, shift, count


def masked_affine(x, nvalid=None, K=0, *, scale=None, shift=None, relu_pre=False, relu=False, residual=None):
    require_cuda(x)
    x = _f32c(x, "x")
    Cc = x.shape[-1]
    R = x.numel() // Cc
    flags = (EPI_RELU_PRE if relu_pre else 0) | (EPI_AFFINE if scale is not None else 0) | \
            (EPI_RELU if relu else 0) | (EPI_RESIDUAL if residual is not None else 0)
    out = torch.empty_like(x)
    with _span("sn_masked_affine_f32"):
        check(lib().sn_masked_affine_f32(ptr(x), Cc, R, Cc, ptr(nvalid), int(K), flags, ptr(scale), ptr(shift),
                                         ptr(residual), Cc, ptr(out), Cc, stream()), "sn_masked_affine_f32")
    return out


def masked_layernorm(x, residual, gamma, beta, eps, nvalid=None, K=0):
    require_cuda(x)
    x = _f32c(x, "x")
    Cc = x.shape[-1]
    out = torch.empty_like(x)
    with _span("sn_masked_layernorm_f32"):
        check(lib().sn_masked_layernorm_f32(ptr(x), ptr(residual), x.numel() // Cc, Cc, ptr(gamma), ptr(beta),
                                            float(eps), ptr(nvalid), int(K), ptr(out), stream()),
              "sn_masked_layernorm_f32")
    return out


def attention_dropout_mask(N, K, heads, p, device):
    """Bernoulli keep-mask of the attention dropout (transformer_module.py:49,55), scaled: 0 or 1/(1-p), [N, heads, K, K].
    Drawn with torch's device generator (reproducible under torch.manual_seed); None when p == 0."""
    if not p:
        return None
    u = torch.rand(N, heads, K, K, device=device)
    # (the same draws as `(u >= p).float() * 1/(1-p)`, thresholded and scaled in place by one launch instead of three)
    check(lib().sn_keep_mask_f32(ptr(u), u.numel(), float(p), float(1.0 / (1.0 - p)), stream()), "sn_keep_mask_f32")
    return u


ATTN_DROP_SITE = 0x41540000      # + index of the rho layer (signnet_hip.h: disjoint from the small ordinals of the feature-dropout sites)


def attention_drop_args(drop, who="set_attention"):
    """drop = (p, snap, site) -> (threshold, scale, snap, site) of sn_set_attention_drop[_bwd]_f32, or None for p == 0 (no mask)."""
    p, snap, site = drop
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{who}: attention dropout probability has to be in [0, 1), but got {p}")
    if p == 0.0:
        return None
    require_cuda(snap)
    if snap.dtype != torch.int64 or snap.numel() != 2 or not snap.is_contiguous():
        raise ValueError(f"{who}: snap must be the int64 [2] {{seed, step}} tensor of a DropoutState")
    thr, scale = dropout_threshold(p)
    return thr, scale, snap, int(site) & 0xFFFFFFFF


def set_attention(q, k, v, N, K, heads, nvalid=None, prob_mask=None, drop=None):
    """prob_mask: an explicit [N, heads, K, K] mask of 0 / 1/(1-p) factors (attention_dropout_mask), or drop = (p, snap, site): the
    same factors from the counter-based generator inside the kernel (signnet_hip.h: the mask contract; snap = the {seed, step} words
    of a DropoutState).  Not both.  p == 0: no mask, the plain launch."""
    require_cuda(q, k, v)
    q, k, v = _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
    D = q.shape[-1]
    if prob_mask is not None and drop is not None:
        raise ValueError("set_attention: give prob_mask or drop, not both")
    if prob_mask is not None and (prob_mask.shape != (N, heads, K, K) or not prob_mask.is_contiguous()):
        raise ValueError("set_attention: prob_mask must be a contiguous [N, heads, K, K] tensor")
    out = torch.empty_like(q)
    args = None if drop is None else attention_drop_args(drop)
    if args is not None:
        thr, scale, snap, site = args
        with _span("sn_set_attention_drop_f32"):
            check(lib().sn_set_attention_drop_f32(ptr(q), ptr(k), ptr(v), N, K, heads, D // heads, ptr(nvalid), thr, scale, ptr(snap), site,
                                                  ptr(out), stream()), "sn_set_attention_drop_f32")
        return out
    with _span("sn_set_attention_f32"):
        check(lib().sn_set_attention_f32(ptr(q), ptr(k), ptr(v), N, K, heads, D // heads, ptr(nvalid), ptr(prob_mask), ptr(out),
                                         stream()), "sn_set_attention_f32")
    return out


def slot_sum(x, N, K):
    require_cuda(x)
    x = _f32c(x, "x")
    Cc = x.shape[-1]
    out = torch.empty(N, Cc, dtype=torch.float32, device=x.device)
    with _span("sn_slot_sum_f32"):
        check(lib().sn_slot_sum_f32(ptr(x), N, K, Cc, ptr(out), stream()), "sn_slot_sum_f32")
    return out


EMBEDDING_INDEX_ERROR = ("index out of range in embedding: a discrete node / edge feature value lies outside its table "
                         "(DiscreteEncoder's max_num_values) — nn.Embedding raises IndexError here too")


_DEFERRED_STATUS = None      # a list while a caller collects the ops' own status words instead of having each op read its own


class defer_status:
    """`with ops.defer_status() as words:` — ops that would read their own status word back (one host wait each: embedding_sum with
    status=None) append it to `words` instead; the caller checks them later (`ops.raise_deferred(words)`).  For steps that must not
    synchronise: a HIP-graph capture (serving.GraphedDGLForward), a loop that checks once per epoch."""

    def __enter__(self):
        global _DEFERRED_STATUS
        self._prev, _DEFERRED_STATUS = _DEFERRED_STATUS, []
        self.words = _DEFERRED_STATUS
        return self.words

    def __exit__(self, *exc):
        global _DEFERRED_STATUS
        _DEFERRED_STATUS = self._prev
        return False


def deferring() -> bool:
    return _DEFERRED_STATUS is not None


def defer(kind, tensor, message=None):
    """Hand a device-side check over to the collector of `defer_status`: kind 'embed' (non-zero: an index outside its embedding table),
    'plan' (a GraphPlan: its check()), 'flag' (non-zero: ValueError(message))."""
    _DEFERRED_STATUS.append((kind, tensor, message))


def raise_deferred(words):
    """The collected checks, read back now (a host wait): raises what the ops themselves would have raised."""
    for kind, t, msg in words:
        if kind == "plan":
            t.check()
        elif kind == "embed":
            if int(t.reshape(-1)[0]):
                raise IndexError(EMBEDDING_INDEX_ERROR)
        elif bool(t.reshape(-1)[0]):
            raise ValueError(msg)


def embedding_sum(idx, tables, status=None):
    """sum_f tables[f][idx[:, f]] — DiscreteEncoder; idx int64 [R] or [R, F].  An index outside its table is never
    dereferenced (it contributes 0) and sets bit 0 of `status` (device int32, e.g. a slot of the batch plan's status block
    that the caller checks later); with status=None the op checks it itself — one host sync — and raises IndexError like
    nn.Embedding does."""
    require_cuda(idx)
    if idx.dtype != torch.int64:
        raise ValueError("embedding_sum: integer features must be int64")
    if idx.dim() == 1:
        idx = idx.unsqueeze(1)
    idx = idx.contiguous()
    R, nf = idx.shape
    if nf > len(tables):
        raise ValueError("embedding_sum: more feature columns than embedding tables")
    tabs = [_f32c(t, "embedding table") for t in tables[:nf]]
    Cc = tabs[0].shape[1]
    arr = (C.c_void_p * nf)(*[t.data_ptr() for t in tabs])
    rows = (C.c_int64 * nf)(*[t.shape[0] for t in tabs])
    out = torch.empty(R, Cc, dtype=torch.float32, device=idx.device)
    if R == 0:                      # (a batch without edges / an empty shard)
        return out
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=idx.device)
    with _span("sn_embedding_sum_f32"):
        check(lib().sn_embedding_sum_f32(ptr(idx), nf, nf, R, arr, rows, Cc, ptr(out), ptr(status), stream()), "sn_embedding_sum_f32")
    if own and _DEFERRED_STATUS is not None:
        defer("embed", status)
    elif own and int(status.item()):
        raise IndexError(EMBEDDING_INDEX_ERROR)
    return out


def segment_pool(x, plan: GraphPlan, mode="add"):
    require_cuda(x)
    x = _f32c(x, "x")
    out = torch.empty(plan.B, x.shape[1], dtype=torch.float32, device=x.device)
    with _span("sn_segment_pool_f32"):
        check(lib().sn_segment_pool_f32(ptr(x), plan.B, x.shape[1], ptr(plan.graph_ptr), 1 if mode == "mean" else 0,
                                        ptr(out), stream()), "sn_segment_pool_f32")
    return out


def segment_max(x, plan: GraphPlan, want_arg=False):
    """dgl.max_nodes: out[g, :] = the channel maximum over graph g's rows of x (sn_segment_max_f32: of equal values the lowest row, a NaN
    kept, an empty graph 0).  want_arg: -> (out, arg), arg [B, C] int32 the row that attains it (-1: empty graph)."""
    require_cuda(x)
    x = _f32c(x, "x")
    out = torch.empty(plan.B, x.shape[1], dtype=torch.float32, device=x.device)
    arg = torch.empty(plan.B, x.shape[1], dtype=torch.int32, device=x.device) if want_arg else None
    with _span("sn_segment_max_f32"):
        check(lib().sn_segment_max_f32(ptr(x), plan.B, x.shape[1], ptr(plan.graph_ptr), ptr(out), ptr(arg), stream()),
              "sn_segment_max_f32")
    return (out, arg) if want_arg else out


def ign_contract_2to1(X):
    """X [b, 1, n, n] or [b, n, n] -> ops [b, n, 5] (IGN 2->1 contractions, ign.py:344-374)."""
    require_cuda(X)
    X = _f32c(X, "X")
    n = X.shape[-1]
    if X.shape[-2] != n or (X.dim() == 4 and X.shape[1] != 1) or X.dim() not in (3, 4):
        raise ValueError("ign_contract_2to1: expected [b, 1, n, n] or [b, n, n]")
    b = X.shape[0]
    out = torch.empty(b, n, 5, dtype=torch.float32, device=X.device)
    scratch = torch.empty(int(lib().sn_ign_contract_scratch_floats(b, n)), dtype=torch.float32, device=X.device)
    with _span("sn_ign_contract_2to1_f32"):
        check(lib().sn_ign_contract_2to1_f32(ptr(X), b, n, ptr(out), ptr(scratch), stream()), "sn_ign_contract_2to1_f32")
    return out


def pna_aggregate(msg, hself, plan: GraphPlan, avg_log: float):
    """PNA tower aggregation (pna_layer.py:50-56,69): msg [E, C] per-edge messages in edge-id order, hself [N, C] the tower's
    input rows -> [N, 13*C] = cat[hself, scalers(aggregators(msg over in-edges))]."""
    require_cuda(msg)
    msg, hself = _f32c(msg, "msg"), _f32c(hself, "hself")
    Cc = msg.shape[1]
    out = torch.empty(plan.N, 13 * Cc, dtype=torch.float32, device=msg.device)
    with _span("sn_pna_aggregate_f32"):
        check(lib().sn_pna_aggregate_f32(ptr(msg), Cc, ptr(hself), Cc, Cc, plan.N, ptr(plan.rowptr), ptr(plan.eperm), float(avg_log),
                                         ptr(out), 13 * Cc, stream()), "sn_pna_aggregate_f32")
    return out


def grouped_linear(x, W, bias, G, *, rowscale=None, scale=None, shift=None):
    """y[:, g*dout:(g+1)*dout] = ((x[:, g*din:(g+1)*din] @ W[g]^T + b_g) * rowscale[row]) * scale + shift — G independent column groups
    (a block-diagonal Linear); W [G, dout, din] float32 contiguous, dout <= 16, din % 4 == 0 and <= 256."""
    require_cuda(x)
    x = _f32c(x, "x")
    Gn, dout, din = W.shape
    if Gn != G or x.shape[-1] != G * din:
        raise ValueError("grouped_linear: x must be [R, G*din] for W [G, dout, din]")
    R = x.numel() // (G * din)
    y = torch.empty(R, G * dout, dtype=torch.float32, device=x.device)
    with _span("sn_grouped_linear_f32"):
        check(lib().sn_grouped_linear_f32(ptr(x), G * din, R, G, din, dout, ptr(W), ptr(bias), ptr(rowscale), ptr(scale), ptr(shift), ptr(y),
                                          G * dout, stream()), "sn_grouped_linear_f32")
    return y


def pna_aggregate_gather(psd, qe, hself, plan: GraphPlan, avg_log: float, tower_width: int = 0, qe_layer=None):
    """PNA aggregation with the pretrans message formed in the kernel: psd [N, 2C] = [W_s h | W_d h] per node, qe [E, C] = W_e e + b,
    message (j -> n, e) = psd[j, :C] + psd[n, C:] + qe[e]; -> [N, 13*C] = cat[hself, scalers(aggregators(.))] (all towers side by side;
    tower_width = it > 0: tower-major columns [tower][13 blocks][it], the input layout of grouped_linear)."""
    require_cuda(psd)
    psd, qe, hself = _f32c(psd, "psd"), _f32c(qe, "qe"), _f32c(hself, "hself")
    Cc, ldq, qoff = qe.shape[1], qe.shape[1], 0
    if qe_layer is not None:    # qe is [E, L*C], every layer's edge term side by side: this layer's column block is read in place
        Cc = hself.shape[1]
        if qe.shape[1] % Cc or not 0 <= qe_layer < qe.shape[1] // Cc:
            raise ValueError("pna_aggregate_gather: qe must be [E, L*C] with 0 <= qe_layer < L")
        qoff = 4 * qe_layer * Cc
    if psd.shape[1] != 2 * Cc or hself.shape[1] != Cc:
        raise ValueError("pna_aggregate_gather: psd must be [N, 2C], hself [N, C] for qe [E, C]")
    out = torch.empty(plan.N, 13 * Cc, dtype=torch.float32, device=psd.device)
    with _span("sn_pna_aggregate_gather_f32"):
        check(lib().sn_pna_aggregate_gather_f32(psd.data_ptr(), 2 * Cc, psd.data_ptr() + 4 * Cc, 2 * Cc, qe.data_ptr() + qoff, ldq, ptr(hself), Cc, Cc, plan.N,
                                                ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), float(avg_log), ptr(out), 13 * Cc, int(tower_width), stream()),
              "sn_pna_aggregate_gather_f32")
    return out


def edge_attention(Q, K, V, Ee, plan: GraphPlan, heads: int):
    """Sparse multi-head attention over the graph's edges with edge features (layers/transformer.py:150-228) -> [N, heads*dk]."""
    require_cuda(Q)
    Q, K, V, Ee = (_f32c(t, n) for t, n in ((Q, "Q"), (K, "K"), (V, "V"), (Ee, "E")))
    d = Q.shape[1]
    if d % heads or d // heads > 32:
        raise ValueError("edge_attention: heads must divide the width and the head width must be <= 32")
    out = torch.empty(plan.N, d, dtype=torch.float32, device=Q.device)
    with _span("sn_edge_attention_f32"):
        check(lib().sn_edge_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Ee), plan.N, int(heads), d // heads, ptr(plan.rowptr), ptr(plan.col),
                                          ptr(plan.eperm), ptr(out), stream()), "sn_edge_attention_f32")
    return out


def edge_attention_fused(qkv, Ee_all, layer: int, plan: GraphPlan, heads: int):
    """The same attention on the column blocks of fused projections: qkv [N, 3*d] = [Q | K | V] of one Linear over cat[W_Q; W_K; W_V],
    Ee_all [E, L*d] = every layer's E projection of the edge embedding side by side (layer `layer` is read) — no copies."""
    require_cuda(qkv)
    if qkv.dtype != torch.float32 or not qkv.is_contiguous() or Ee_all.dtype != torch.float32 or not Ee_all.is_contiguous():
        raise ValueError("edge_attention_fused: contiguous float32 matrices expected")
    d = qkv.shape[1] // 3
    if qkv.shape[1] != 3 * d or d % heads or d // heads > 32 or Ee_all.shape[1] % d or not 0 <= layer < Ee_all.shape[1] // d:
        raise ValueError("edge_attention_fused: qkv must be [N, 3*d], Ee_all [E, L*d], head width <= 32")
    out = torch.empty(plan.N, d, dtype=torch.float32, device=qkv.device)
    base, eb = qkv.data_ptr(), Ee_all.data_ptr() + 4 * d * layer
    with _span("sn_edge_attention_f32"):
        check(lib().sn_edge_attention_strided_f32(C.c_void_p(base), C.c_void_p(base + 4 * d), C.c_void_p(base + 8 * d), 3 * d, C.c_void_p(eb),
                                                  Ee_all.shape[1], plan.N, int(heads), d // heads, ptr(plan.rowptr), ptr(plan.col),
                                                  ptr(plan.eperm), ptr(out), stream()), "sn_edge_attention_strided_f32")
    return out


FULL_ATTENTION_MAX_CLASSES = 16


def _full_attention_blocks(fn, Q, K, V, Q2, K2):
    """The five [N, d] float32 blocks of a full-graph attention and their common row stride: separate contiguous matrices (stride d) or
    column views of one projection (unit column stride, one common row stride) — read in place, no copies."""
    N, d = Q.shape
    ld = Q.stride(0) if N > 1 else d
    for t, n in ((Q, "Q"), (K, "K"), (V, "V"), (Q2, "Q_2"), (K2, "K_2")):
        if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (N, d) or t.stride(1) != 1 or (N > 1 and t.stride(0) != ld) or ld < d:
            raise ValueError(f"{fn}: {n} must be a float32 [N, heads*dk] block with unit column stride and the row stride of Q")
    return N, d, ld


def _full_attention_tables(fn, d, heads, T_real, T_fake, gamma):
    if d % heads or d // heads > 32:
        raise ValueError(f"{fn}: heads must divide the width and the head width must be <= 32")
    T_real, T_fake = _f32c(T_real, "T_real"), _f32c(T_fake, "T_fake")
    Cc = T_real.shape[0]
    if T_real.dim() != 2 or T_real.shape != T_fake.shape or T_real.shape[1] != d:
        raise ValueError(f"{fn}: T_real and T_fake must both be [C, heads*dk]")
    if not 1 <= Cc <= FULL_ATTENTION_MAX_CLASSES:
        raise ValueError(f"{fn}: {Cc} edge classes not in [1, {FULL_ATTENTION_MAX_CLASSES}]")
    if gamma.dtype != torch.float32 or gamma.numel() != 1 or not gamma.is_cuda:
        raise ValueError(f"{fn}: gamma must be one float32 in device memory")
    return T_real, T_fake, Cc


def _full_attention_check(fn, d, heads, T_real, T_fake, codes, gamma, plan):
    T_real, T_fake, Cc = _full_attention_tables(fn, d, heads, T_real, T_fake, gamma)
    if codes.dtype != torch.int32 or not codes.is_contiguous() or codes.numel() != plan.E:
        raise ValueError(f"{fn}: codes must be a contiguous int32 vector with one entry (2 * class + real) per edge of the plan")
    return T_real, T_fake, Cc


def full_attention(Q, K, V, Q2, K2, T_real, T_fake, codes, gamma, plan: GraphPlan, heads: int, status=None, want_den=False):
    """Full-graph attention of the graph Transformer (layers/transformer.py:155-228, full_graph True) -> [N, heads*dk]: real pairs through
    Q / K / T_real, fake pairs through Q_2 / K_2 / T_fake, mixed by clamp(gamma, 0, 1) — sn_full_attention_f32.  T_*: [C, heads*dk] class
    tables (E(embedding_e.weight), E_2(embedding_e.weight)); codes int32 [E] = 2 * class + real in edge-id order; gamma: the Parameter
    (read on the device).  Q .. K_2 may be column views of one projection.  A class outside [0, C) sets bit 0 of `status` (device
    int32); with status=None the op checks it itself — one host sync, or ops.defer_status — and raises IndexError like nn.Embedding."""
    require_cuda(Q, codes, gamma)
    N, d, ld = _full_attention_blocks("full_attention", Q, K, V, Q2, K2)
    if N != plan.N:
        raise ValueError("full_attention: the blocks must have one row per node of the plan")
    T_real, T_fake, Cc = _full_attention_check("full_attention", d, heads, T_real, T_fake, codes, gamma, plan)
    out = torch.empty(N, d, dtype=torch.float32, device=Q.device)
    den = torch.empty(N, int(heads), dtype=torch.float32, device=Q.device)
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=Q.device)
    with _span("sn_full_attention_f32"):
        check(lib().sn_full_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), ld, ptr(T_real), ptr(T_fake), Cc, ptr(codes), ptr(gamma), N,
                                          int(heads), d // heads, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(out), ptr(den),
                                          ptr(status), stream()), "sn_full_attention_f32")
    if own and _DEFERRED_STATUS is not None:
        defer("embed", status)
    elif own and plan.E and int(status.item()):
        raise IndexError(EMBEDDING_INDEX_ERROR)
    return (out, den) if want_den else out


def full_attention_bwd(Q, K, V, Q2, K2, T_real, T_fake, codes, gamma, out, den, dout, plan: GraphPlan, rplan: GraphPlan, heads: int):
    """Adjoint of full_attention (sn_full_attention_bwd_f32) -> dQ, dK, dV, dQ_2, dK_2 [N, heads*dk], dT_real, dT_fake [C, heads*dk],
    dgamma [1]; rplan: the plan of the flipped edge list.  No atomics: bit-identical on repeated calls."""
    require_cuda(Q, dout)
    N, d, ld = _full_attention_blocks("full_attention_bwd", Q, K, V, Q2, K2)
    T_real, T_fake, Cc = _full_attention_check("full_attention_bwd", d, heads, T_real, T_fake, codes, gamma, plan)
    out, den, dout = _f32c(out, "out"), _f32c(den, "den"), _f32c(dout, "dout")
    dev = Q.device
    new = lambda r: torch.empty(r, d, dtype=torch.float32, device=dev)
    dQ, dK, dV, dQ2, dK2, dTr, dTf = new(N), new(N), new(N), new(N), new(N), new(Cc), new(Cc)
    dgamma = torch.empty(1, dtype=torch.float32, device=dev)
    scratch = torch.empty(max(int(lib().sn_full_attention_bwd_scratch_floats(N, plan.E, int(heads), d // heads, Cc)), 2), dtype=torch.float32,
                          device=dev)
    with _span("sn_full_attention_bwd_f32"):
        check(lib().sn_full_attention_bwd_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), ld, ptr(T_real), ptr(T_fake), Cc, ptr(codes), ptr(gamma),
                                              ptr(out), ptr(den), ptr(dout), N, plan.E, int(heads), d // heads, ptr(plan.rowptr), ptr(plan.col),
                                              ptr(plan.eperm), ptr(rplan.rowptr), ptr(rplan.col), ptr(rplan.eperm), ptr(dQ), ptr(dK), ptr(dV),
                                              ptr(dQ2), ptr(dK2), ptr(dTr), ptr(dTf), ptr(dgamma), ptr(scratch), stream()),
              "sn_full_attention_bwd_f32")
    return dQ, dK, dV, dQ2, dK2, dTr, dTf, dgamma


def full_graph_codes(e, real):
    """The int32 edge codes full_attention reads: 2 * class + real (index plumbing only)."""
    return (e.long().reshape(-1) * 2 + (real.reshape(-1) != 0).long()).to(torch.int32)


MAKE_FULL_GRAPH_ERROR = ("make_full_graph: the sparse graph has a self loop or a repeated (u, v) edge — the reference's assignment of the "
                         "real edges (data/molecules.py:233-234) gives neither a meaning")


def make_full_graph(g, e, status=None):
    """data/molecules.py:211-235 for a whole batch in one launch (sn_make_full_graph): the complete directed graph of every graph of
    `g` -> a dgl_deepsigns.Graph over sum n (n - 1) edges — per graph u-major, v ascending, v != u, the order of
    networkx.complete_graph(n).to_directed().edges() — with edata['real'] (int64 0 / 1) and edata['feat'] = the full `e` (int64: a real
    edge keeps its class, a fake edge gets 0), which is also returned: (full_g, e_full).  The sizes come from the graph object's
    batch_num_nodes() (free when it is a host tensor).  A self loop or a repeated (u, v) sets `status` (device int32 [1]); with
    status=None the op checks it itself — one host sync, or ops.defer_status — and raises ValueError."""
    from .dgl_deepsigns import Graph, cached_plan
    src, _ = g.edges()
    require_cuda(src, e)
    if e.dtype != torch.int64:
        raise ValueError("make_full_graph: the bond classes must be int64")
    e = e.reshape(-1).contiguous()
    bnn = g.batch_num_nodes()
    counts = bnn.detach().to("cpu", torch.int64)
    N = int(counts.sum())
    bne = counts * (counts - 1)
    E_full = int(bne.sum())
    plan = cached_plan(g, N)
    if e.numel() != plan.E:
        raise ValueError("make_full_graph: one bond class per edge of the graph expected")
    dev = src.device
    buf = torch.empty(4, E_full, dtype=torch.int64, device=dev)
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _span("sn_make_full_graph"):
        check(lib().sn_make_full_graph(ptr(plan.graph_ptr), plan.B, N, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(e), plan.E, E_full,
                                       ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), ptr(buf[3]), ptr(status), stream()), "sn_make_full_graph")
    if own and _DEFERRED_STATUS is not None:
        defer("flag", status, MAKE_FULL_GRAPH_ERROR)
    elif own and int(status.item()):
        raise ValueError(MAKE_FULL_GRAPH_ERROR)
    full = Graph(buf[0], buf[1], bnn, bne)
    full.edata["real"] = buf[2]
    full.edata["feat"] = buf[3]
    return full, buf[3]


BOND_GRAPH_ERROR = ("bond_full_attention: the bond graph has a self loop, a repeated (u, v) edge or a bond between two graphs — the "
                    "reference's assignment of the real edges (data/molecules.py:233-234) gives none a meaning")


def bond_attention_staged_nodes(dk: int, bwd: bool = False) -> int:
    """The largest graph whose rows and pair table sn_bond_full_attention_f32 (bwd: its adjoint) stage in LDS for head width dk; a
    larger graph takes the kernels' global-memory path (same arithmetic, same bits)."""
    return int(lib().sn_bond_full_attention_staged_nodes(int(dk), int(bool(bwd))))


def _bond_attention_check(fn, d, heads, T_real, T_fake, e, gamma, plan, graph_valid, edge_valid):
    T_real, T_fake, Cc = _full_attention_tables(fn, d, heads, T_real, T_fake, gamma)
    if e.dtype != torch.int64 or not e.is_cuda or e.numel() != plan.E:
        raise ValueError(f"{fn}: e must be the int64 bond classes in device memory, one per edge of the plan")
    for v, rows, n in ((graph_valid, plan.B, "graph_valid"), (edge_valid, plan.E, "edge_valid")):
        if v is not None and (v.dtype != torch.int32 or not v.is_cuda or not v.is_contiguous() or v.numel() < rows):
            raise ValueError(f"{fn}: {n} must be a contiguous int32 0/1 vector in device memory with an entry per row")
    return T_real, T_fake, Cc, e.reshape(-1).contiguous()


def bond_full_attention(Q, K, V, Q2, K2, T_real, T_fake, e, gamma, plan: GraphPlan, heads: int, status=None, graph_valid=None,
                        edge_valid=None, want_den=False):
    """Full-graph attention computed from the BOND graph (sn_bond_full_attention_f32) -> [N, heads*dk]: what full_attention gives on
    make_full_graph's output, without its edge list.  plan: cached_plan of the molecular graph; e: its bond classes, int64 [E], read in
    place; T_*, gamma and the five blocks as full_attention.  graph_valid / edge_valid: int32 0 / 1 (a padded batch): an invalid graph
    gets zeros and raises no flag, an invalid edge is not a bond.  status: device int32 [2] — [0] a bond class outside [0, C), [1] a self
    loop / repeated edge (make_full_graph's flags); with status=None the op checks both itself — one host sync, or ops.defer_status —
    and raises IndexError / ValueError."""
    require_cuda(Q, e, gamma)
    N, d, ld = _full_attention_blocks("bond_full_attention", Q, K, V, Q2, K2)
    if N != plan.N:
        raise ValueError("bond_full_attention: the blocks must have one row per node of the plan")
    T_real, T_fake, Cc, e = _bond_attention_check("bond_full_attention", d, heads, T_real, T_fake, e, gamma, plan, graph_valid, edge_valid)
    out = torch.empty(N, d, dtype=torch.float32, device=Q.device)
    den = torch.empty(N, int(heads), dtype=torch.float32, device=Q.device)
    own = status is None
    if own:
        status = torch.zeros(2, dtype=torch.int32, device=Q.device)
    elif status.dtype != torch.int32 or status.numel() < 2 or not status.is_contiguous():
        raise ValueError("bond_full_attention: status must be a contiguous int32 [2] in device memory")
    with _span("sn_bond_full_attention_f32"):
        check(lib().sn_bond_full_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), ld, ptr(T_real), ptr(T_fake), Cc, ptr(e), ptr(gamma), N,
                                               plan.B, plan.E, int(heads), d // heads, ptr(plan.graph_ptr), ptr(plan.rowptr), ptr(plan.col),
                                               ptr(plan.eperm), ptr(graph_valid), ptr(edge_valid), ptr(out), ptr(den), ptr(status), stream()),
              "sn_bond_full_attention_f32")
    if own:
        check_bond_status(status)
    return (out, den) if want_den else out


def check_bond_status(status):
    """The two words of a bond_full_attention status: handed to ops.defer_status where one collects, else read now (one host wait)."""
    if _DEFERRED_STATUS is not None:
        defer("embed", status[0:1])
        defer("flag", status[1:2], BOND_GRAPH_ERROR)
        return
    words = status.tolist()
    if words[0]:
        raise IndexError(EMBEDDING_INDEX_ERROR)
    if words[1]:
        raise ValueError(BOND_GRAPH_ERROR)


def bond_full_attention_bwd(Q, K, V, Q2, K2, T_real, T_fake, e, gamma, out, den, dout, plan: GraphPlan, heads: int, graph_valid=None,
                            edge_valid=None):
    """Adjoint of bond_full_attention (sn_bond_full_attention_bwd_f32) -> dQ, dK, dV, dQ_2, dK_2 [N, heads*dk], dT_real, dT_fake
    [C, heads*dk], dgamma [1].  No reverse plan, no per-pair array; no atomics: bit-identical on repeated calls."""
    require_cuda(Q, dout)
    N, d, ld = _full_attention_blocks("bond_full_attention_bwd", Q, K, V, Q2, K2)
    if N != plan.N:
        raise ValueError("bond_full_attention_bwd: the blocks must have one row per node of the plan")
    T_real, T_fake, Cc, e = _bond_attention_check("bond_full_attention_bwd", d, heads, T_real, T_fake, e, gamma, plan, graph_valid, edge_valid)
    out, den, dout = _f32c(out, "out"), _f32c(den, "den"), _f32c(dout, "dout")
    dev = Q.device
    new = lambda r: torch.empty(r, d, dtype=torch.float32, device=dev)
    dQ, dK, dV, dQ2, dK2, dTr, dTf = new(N), new(N), new(N), new(N), new(N), new(Cc), new(Cc)
    dgamma = torch.empty(1, dtype=torch.float32, device=dev)
    scratch = torch.empty(max(int(lib().sn_bond_full_attention_bwd_scratch_floats(N, plan.B, int(heads), d // heads, Cc)), 2),
                          dtype=torch.float32, device=dev)
    with _span("sn_bond_full_attention_bwd_f32"):
        check(lib().sn_bond_full_attention_bwd_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), ld, ptr(T_real), ptr(T_fake), Cc, ptr(e), ptr(gamma),
                                                   ptr(out), ptr(den), ptr(dout), N, plan.B, plan.E, int(heads), d // heads, ptr(plan.graph_ptr),
                                                   ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(graph_valid), ptr(edge_valid), ptr(dQ),
                                                   ptr(dK), ptr(dV), ptr(dQ2), ptr(dK2), ptr(dTr), ptr(dTf), ptr(dgamma), ptr(scratch), stream()),
              "sn_bond_full_attention_bwd_f32")
    return dQ, dK, dV, dQ2, dK2, dTr, dTf, dgamma


def gat_aggregate(feat, attn_l, attn_r, bias, plan: GraphPlan, heads: int, negative_slope=0.2, relu=True, want_lse=False):
    """DGL GATConv after its fc (gat_net.py:62-66): feat [N, heads*C] -> [N, heads*C]; see sn_gat_aggregate_f32."""
    require_cuda(feat)
    feat = _f32c(feat, "feat")
    d = feat.shape[1]
    if d % heads or d // heads > 128:
        raise ValueError("gat_aggregate: heads must divide the width and the head width must be <= 128")
    al, ar = _f32c(attn_l.reshape(-1), "attn_l"), _f32c(attn_r.reshape(-1), "attn_r")
    b = None if bias is None else _f32c(bias.reshape(-1), "bias")
    out = torch.empty(plan.N, d, dtype=torch.float32, device=feat.device)
    lse = torch.empty(plan.N, heads, dtype=torch.float32, device=feat.device) if want_lse else None
    with _span("sn_gat_aggregate_f32"):
        check(lib().sn_gat_aggregate_f32(ptr(feat), ptr(al), ptr(ar), ptr(b), plan.N, int(heads), d // heads, float(negative_slope), int(relu),
                                         ptr(plan.rowptr), ptr(plan.col), ptr(out), ptr(lse), stream()), "sn_gat_aggregate_f32")
    return (out, lse) if want_lse else out


def pointwise(x, *, rowscale=None, scale=None, shift=None, act="none", slope=0.01, residual=None):
    """y = act((x * rowscale[r]) * scale[c] + shift[c]) + residual, act in none / relu / leaky."""
    require_cuda(x)
    x = _f32c(x, "x")
    Cc = x.shape[-1]
    R = x.numel() // Cc
    out = torch.empty_like(x)
    a = {"none": 0, "relu": 1, "leaky": 2, "relu_sum": 3}[act]
    if rowscale is not None:
        rowscale = _f32c(rowscale.reshape(-1), "rowscale")
        if rowscale.numel() != R:
            raise ValueError("pointwise: one row scale per row expected")
    check(lib().sn_pointwise_f32(ptr(x), Cc, R, Cc, ptr(rowscale), ptr(scale), ptr(shift), a, float(slope),
                                 ptr(None if residual is None else _f32c(residual, "residual")), Cc, ptr(out), Cc, stream()),
          "sn_pointwise_f32")
    return out


def dense_attention(q, k, v, heads, want_lse=False):
    """softmax(q k^T / sqrt(dk)) v per head over whole sequences (LearningFilters/models.py:115-135's encoder attention).
    q, k, v: [Bt, L, heads*dk] (batch_first), dk <= 32."""
    require_cuda(q)
    q, k, v = _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
    if q.dim() != 3 or k.shape != q.shape or v.shape != q.shape or q.shape[-1] % heads:
        raise ValueError("dense_attention: q, k, v must be [Bt, L, heads*dk] of one shape")
    Bt, L, d = q.shape
    out = torch.empty_like(q)
    lse = torch.empty(Bt, heads, L, dtype=torch.float32, device=q.device)
    with _span("sn_dense_attention_f32"):
        check(lib().sn_dense_attention_f32(ptr(q), ptr(k), ptr(v), Bt, L, heads, d // heads, ptr(out), ptr(lse), stream()),
              "sn_dense_attention_f32")
    return (out, lse) if want_lse else out


class EigenspacePlan:
    """Device-side result of sn_eigenspace_group (LearningFilters/training.py:47-61 without the projectors) + the few numbers the
    host needs to size tensors (read back once: this is a per-graph one-off, as in the reference).
    mults: sorted distinct multiplicities; counts[i]: eigenspaces with multiplicity mults[i]; slot_base[i]: first slot of that
    multiplicity in the multiplicity-major stack (the order of the reference's {mult: torch.cat(projectors)} dict)."""

    def __init__(self, N, space_of, space_start, space_mult, space_slot, mults, counts, n_spaces, max_mult):
        self.N, self.space_of, self.space_start, self.space_mult, self.space_slot = N, space_of, space_start, space_mult, space_slot
        self.mults, self.counts, self.n_spaces, self.max_mult = mults, counts, n_spaces, max_mult
        self.slot_base = {}
        off = 0
        for m, c in zip(mults, counts):
            self.slot_base[m] = off
            off += c

    def group(self, stack, mult):
        """The rows of a [n_spaces, ...] slot-ordered stack that belong to multiplicity `mult`."""
        i = self.mults.index(mult)
        off = self.slot_base[mult]
        return stack[off:off + self.counts[i]]


def eigenspace_group(eigvals, decimals=5) -> EigenspacePlan:
    """`around(eigvals, 5)` + `unique(return_counts)` + the multiplicity grouping of training.py:47-73, on the device."""
    require_cuda(eigvals)
    ev = _f32c(eigvals, "eigvals")
    N = ev.numel()
    ints = torch.empty(6 * N + 8, dtype=torch.int32, device=ev.device)
    space_of, space_start, space_mult, space_slot = ints[:N], ints[N:2 * N + 1], ints[2 * N + 1:3 * N + 1], ints[3 * N + 1:4 * N + 1]
    mult_list, mult_count, meta = ints[4 * N + 1:5 * N + 1], ints[5 * N + 1:6 * N + 1], ints[6 * N + 1:6 * N + 5]
    check(lib().sn_eigenspace_group(ptr(ev), N, int(decimals), ptr(space_of), ptr(space_start), ptr(space_mult), ptr(space_slot),
                                    ptr(mult_list), ptr(mult_count), ptr(meta), stream()), "sn_eigenspace_group")
    ns, nm, err, mmax = meta.tolist()                   # one host sync (per graph, once)
    if err:
        raise ValueError("eigenspace_group: the eigenvalues must be in ascending order (as eigh returns them)")
    return EigenspacePlan(N, space_of, space_start, space_mult, space_slot, mult_list[:nm].tolist(), mult_count[:nm].tolist(), ns, mmax)


def eigenspace_projectors(eigvecs, plan: EigenspacePlan):
    """[n_spaces, N, N] stack of P_s = V_s V_s^T in multiplicity-major order (training.py:61-73)."""
    require_cuda(eigvecs)
    V = _f32c(eigvecs, "eigvecs")
    N = plan.N
    if V.shape != (N, N):
        raise ValueError("eigenspace_projectors: eigvecs must be [N, N] (V[node, eigenvector])")
    out = torch.empty(plan.n_spaces, N, N, dtype=torch.float32, device=V.device)
    with _span("sn_eigenspace_projectors_f32"):
        check(lib().sn_eigenspace_projectors_f32(ptr(V), N, N, ptr(plan.space_start), ptr(plan.space_slot), plan.n_spaces, ptr(out),
                                                 stream()), "sn_eigenspace_projectors_f32")
    return out


def ign_contract_eigvecs(eigvecs, plan: EigenspacePlan):
    """The 2->1 contractions [n_spaces, N, 5] of every projector V_s V_s^T, computed from V alone (no N x N matrix)."""
    require_cuda(eigvecs)
    V = _f32c(eigvecs, "eigvecs")
    N = plan.N
    out = torch.empty(plan.n_spaces, N, 5, dtype=torch.float32, device=V.device)
    with _span("sn_ign_contract_eigvecs_f32"):
        check(lib().sn_ign_contract_eigvecs_f32(ptr(V), N, N, ptr(plan.space_start), ptr(plan.space_slot), plan.n_spaces,
                                                plan.max_mult, ptr(out), stream()), "sn_ign_contract_eigvecs_f32")
    return out


EVD_STATUS = {1: "an edge leaves its graph (or a node id is out of range)", 2: "a graph has more than 64 nodes",
              4: "the Jacobi iteration did not converge", 8: "eigen_vectors buffer too small"}


def laplacian_evd(edge_index, graph_ptr, N, total, norm=None, pos_enc_dim=0, skip=1):
    """Batched Laplacian eigendecomposition on the device (transform.py:7-23 for every graph of a collated batch).

    edge_index [2,E] int64, graph_ptr [B+1] int32 (device), N nodes, total = sum n_b^2 (host int).
    Returns (eigen_values [N], eigen_vectors [total], evoff [B+1] int64, pos_enc [N,k] or None, status int32[4])."""
    require_cuda(edge_index, graph_ptr)
    if norm not in (None, "sym"):
        raise ValueError(f"unsupported normalization {norm!r} (None or 'sym')")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: expected int64 [2, E]")
    if graph_ptr.dtype != torch.int32:
        raise ValueError("graph_ptr: expected int32 [B+1]")
    edge_index = edge_index.contiguous()
    dev = edge_index.device
    B, E = graph_ptr.numel() - 1, edge_index.shape[1]
    val = torch.empty(N, dtype=torch.float32, device=dev)
    vec = torch.empty(total, dtype=torch.float32, device=dev)
    evoff = torch.empty(B + 1, dtype=torch.int64, device=dev)
    pe = torch.empty(N, pos_enc_dim, dtype=torch.float32, device=dev) if pos_enc_dim > 0 else None
    work = torch.empty(int(lib().sn_evd_work_ints(B)), dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    with _span("sn_laplacian_evd_f32"):
        check(lib().sn_laplacian_evd_f32(ptr(edge_index), E, ptr(graph_ptr), B, N, 0 if norm is None else 1, ptr(evoff),
                                         ptr(val), ptr(vec), total, ptr(pe), int(pos_enc_dim), int(skip), ptr(work),
                                         ptr(status), stream()), "sn_laplacian_evd_f32")
    return val, vec, evoff, pe, status


EVD_LARGE_MAX_NODES = 128          # = sn_evd_large_max_nodes(): graphs of 65 .. 128 nodes go through sn_laplacian_evd_large_f32
EVD_LARGE_STATUS = {1: EVD_STATUS[1], 2: "a graph has more than 128 nodes", 4: EVD_STATUS[4], 8: EVD_STATUS[8]}


def laplacian_evd_large(edge_index, graph_ptr, N, total, evoff, val, vec, pe=None, norm=None, pos_enc_dim=0, skip=1):
    """The graphs of 65 .. 128 nodes of a batch, into the buffers `laplacian_evd` returned (same val / vec / pe, `evoff` as laid out
    there): one launch for all of them; no byte of a smaller or larger graph is touched.  Returns status int32[4] of its own."""
    require_cuda(edge_index, graph_ptr, evoff, val, vec, pe)
    if norm not in (None, "sym"):
        raise ValueError(f"unsupported normalization {norm!r} (None or 'sym')")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: expected int64 [2, E]")
    if graph_ptr.dtype != torch.int32:
        raise ValueError("graph_ptr: expected int32 [B+1]")
    B, E = graph_ptr.numel() - 1, edge_index.shape[1]
    if evoff.dtype != torch.int64 or evoff.numel() != B + 1 or not evoff.is_contiguous():
        raise ValueError("evoff: expected contiguous int64 [B+1]")
    if val.dtype != torch.float32 or vec.dtype != torch.float32 or not (val.is_contiguous() and vec.is_contiguous()):
        raise ValueError("val / vec: expected contiguous float32")
    if val.numel() < N or vec.numel() < total:
        raise ValueError("val / vec: smaller than N / total")
    if pos_enc_dim > 0 and (pe is None or pe.dtype != torch.float32 or not pe.is_contiguous() or tuple(pe.shape) != (N, pos_enc_dim)):
        raise ValueError("pe: expected contiguous float32 [N, pos_enc_dim]")
    edge_index = edge_index.contiguous()
    dev = edge_index.device
    work = torch.empty(int(lib().sn_evd_large_work_ints(B)), dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    with _span("sn_laplacian_evd_large_f32"):
        check(lib().sn_laplacian_evd_large_f32(ptr(edge_index), E, ptr(graph_ptr), B, N, 0 if norm is None else 1, ptr(evoff),
                                               ptr(val), ptr(vec), total, ptr(pe) if pos_enc_dim > 0 else None, int(pos_enc_dim),
                                               int(skip), ptr(work), ptr(status), stream()), "sn_laplacian_evd_large_f32")
    return status


def bn_fold_stats(weight, bias, mean, var, eps, c_pad=None):
    """(scale, shift) of a BatchNorm from explicit statistics (batch statistics of the train-mode / no-running-stats case)."""
    Cc = mean.numel()
    cp = Cc if c_pad is None else int(c_pad)
    scale = torch.empty(cp, dtype=torch.float32, device=mean.device)
    shift = torch.empty(cp, dtype=torch.float32, device=mean.device)
    check(lib().sn_bn_fold_f32(ptr(weight), ptr(bias), ptr(mean), ptr(var), float(eps), Cc, cp, ptr(scale), ptr(shift),
                               stream()), "sn_bn_fold_f32")
    return scale, shift


def bn_running_update(bn, mean, var, count):
    """Side effect of a train-mode BatchNorm1d forward on its buffers (momentum None = cumulative average is not supported)."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm1d(momentum=None) (cumulative moving average) is not supported")
    check(lib().sn_bn_running_update_f32(ptr(mean), ptr(var), ptr(count), float(bn.momentum), bn.num_features,
                                         ptr(bn.running_mean), ptr(bn.running_var), stream()), "sn_bn_running_update_f32")
    _count_batch(bn)


# ----------------------------------------------------------------------------- roofline accounting (bench.py)
MFMA_F32_PEAK_TF = 157.3     # MI355X_MICROARCH.md: fp32-input MFMA dense peak (= fp32 vector peak)
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E spec


# fp32 GEMMs evaluated as six bf16 partial products (csrc/fused_common.hpp): the bound is the dense bf16 MFMA peak
# (MI355X_MICROARCH.md: ~2.5 PFLOP/s) divided by the 6 MFMAs each fp32 multiply-add costs.
MFMA_BF16_PEAK_TF = 2500.0
MFMA_SPLIT_F32_PEAK_TF = MFMA_BF16_PEAK_TF / 6.0


def _mfma_roof(label, flops, mean_ms, per_step, peak=None, peak_note=None):
    peak = MFMA_F32_PEAK_TF if peak is None else peak
    t = mean_ms * per_step * 1e-3
    ach = flops / t / 1e12
    out = {"kernel": label, "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
           "frac": ach / peak, "traffic": None, "flops_per_launch": flops / per_step, "mean_launch_us": mean_ms * 1e3}
    if peak_note:
        out["peak_note"] = peak_note
    return out


_SPLIT_NOTE = ("fp32-equivalent flops; each fp32 product = 6 v_mfma_f32_16x16x32_bf16 partial products (exact 3 x bf16 "
               "operand split, fp32 accumulate): peak = 2500 TFLOP/s dense bf16 / 6; the fp32-input MFMA peak is 157.3")


def _roof_linear(fl, wl, host, mean_ms, per_step):
    """Layer path: all dense contractions go through sn_masked_linear_f32 (attention's K x K part excepted)."""
    flops = fl["total"] - wl["nl_rho"] * 4 * sum(n * min(n, wl["k"]) ** 2 for n in host.sizes) * wl["hidden"]
    return _mfma_roof("sn_masked_linear_f32 (k_linear, all launches of a step)", flops, mean_ms, per_step)


def _roof_phi(fl, wl, host, mean_ms, per_step):
    """Fused phi: algorithmic flops = 2 signs x (L-1) layers x 2 Linear x 2*d*d per VALID (node, slot) row
    (SURVEY.md §8(d)); padding rows of the work bins are not counted."""
    return _mfma_roof("sn_phi_fused_f32 (k_phi_fused)", fl["phi"], mean_ms, per_step, MFMA_SPLIT_F32_PEAK_TF, _SPLIT_NOTE)


def _roof_rho(fl, wl, host, mean_ms, per_step):
    return _mfma_roof("sn_rho_fused_f32 (k_rho_fused)", fl["rho"] - 2 * fl["N"] * wl["hidden"] ** 2, mean_ms, per_step,
                      MFMA_SPLIT_F32_PEAK_TF, _SPLIT_NOTE)


def _roof_gnn(fl, wl, host, mean_ms, per_step):
    return _mfma_roof("sn_gnn_fused_f32 (k_gnn_coop)", fl["gnn"] + 2 * fl["N"] * wl["hidden"] ** 2, mean_ms, per_step,
                      MFMA_SPLIT_F32_PEAK_TF, _SPLIT_NOTE)


KERNEL_ROOFLINE = {"sn_masked_linear_f32": _roof_linear, "sn_phi_fused_f32": _roof_phi, "sn_rho_fused_f32": _roof_rho,
                   "sn_gnn_fused_f32": _roof_gnn}


# ----------------------------------------------------------------------------- bucketed (padded) training batches
class _BucketPackC(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_row_bytes", C.c_int64), ("edge_index", C.c_void_p), ("edge_attr", C.c_void_p),
                ("edge_row_bytes", C.c_int64), ("batch", C.c_void_p), ("eigen_values", C.c_void_p), ("eigen_vectors", C.c_void_p),
                ("target", C.c_void_p), ("target_row_bytes", C.c_int64),
                ("N", C.c_int64), ("E", C.c_int64), ("B", C.c_int64), ("S", C.c_int64),
                ("x_out", C.c_void_p), ("edge_index_out", C.c_void_p), ("edge_attr_out", C.c_void_p), ("batch_out", C.c_void_p),
                ("eigen_values_out", C.c_void_p), ("eigen_vectors_out", C.c_void_p), ("target_out", C.c_void_p),
                ("node_valid", C.c_void_p), ("edge_valid", C.c_void_p), ("graph_valid", C.c_void_p), ("counts", C.c_void_p),
                ("N_cap", C.c_int64), ("E_cap", C.c_int64), ("B_cap", C.c_int64), ("S_cap", C.c_int64)]


def _row_bytes(t):
    return t.element_size() * (t[0].numel() if t.dim() > 1 else 1)


def bucket_pack(data, target, out):
    """Copy a batch (and its target) of any shape into the capacity buffers `out` (a PaddedBatch of train_graph) in ONE launch
    (sn_bucket_pack): the padding rows, the node / edge / graph validity vectors and the device count block [N, E, B, S] too.
    A batch without eigen_vectors / eigen_values (the plain GNN baselines and NetGINE read none) goes through sn_bucket_pack_plain:
    S = 0 and zero-filled eigen capacity buffers."""
    x, ei, ea, bt = data.x.contiguous(), data.edge_index.contiguous(), data.edge_attr.contiguous(), data.batch.contiguous()
    ev, es = getattr(data, "eigen_vectors", None), getattr(data, "eigen_values", None)
    plain = ev is None or es is None
    if plain:
        ev = es = None
    else:
        ev, es = _f32c(ev, "eigen_vectors"), _f32c(es, "eigen_values")
    require_cuda(x, ei, ea, bt, ev, es)
    N, E, B, S = bt.numel(), (ei.shape[1] if ei.numel() else 0), int(data.num_graphs), 0 if plain else ev.numel()
    for name, src, dst in (("x", x, out.x), ("edge_attr", ea, out.edge_attr), ("batch", bt, out.batch)):
        if src.dtype != dst.dtype or tuple(src.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"bucket_pack: {name} is {src.dtype} {tuple(src.shape)}, the bucket holds {dst.dtype} {tuple(dst.shape)}")
    if ei.dtype != torch.int64 or ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError("bucket_pack: edge_index must be int64 [2, E]")
    if (N if plain else es.numel()) != N or x.shape[0] != N or ea.shape[0] != E:
        raise ValueError(f"bucket_pack: x / eigen_values / edge_attr rows ({x.shape[0]}, {N if plain else es.numel()}, {ea.shape[0]}) do not match "
                         f"N = {N}, E = {E}")
    t = None
    if target is not None:
        t = target.contiguous()
        if t.dtype != out.target.dtype or t.numel() != B * out.target[0].numel():
            raise ValueError(f"bucket_pack: target {t.dtype} {tuple(t.shape)} for {B} graphs, the bucket holds rows of "
                             f"{tuple(out.target.shape[1:])} {out.target.dtype}")
    a = _BucketPackC(ptr(x), _row_bytes(out.x), ptr(ei), ptr(ea), _row_bytes(out.edge_attr), ptr(bt), ptr(es), ptr(ev),
                     ptr(t), 0 if t is None else _row_bytes(out.target),
                     N, E, B, S, ptr(out.x), ptr(out.edge_index), ptr(out.edge_attr), ptr(out.batch), ptr(out.eigen_values),
                     ptr(out.eigen_vectors), ptr(out.target), ptr(out.node_valid), ptr(out.edge_valid), ptr(out.graph_valid),
                     ptr(out.counts), out.N_cap, out.E_cap, out.B_cap, out.S_cap)
    with _span("sn_bucket_pack"):
        if plain:
            check(lib().sn_bucket_pack_plain(C.byref(a), stream()), "sn_bucket_pack_plain")
        else:
            check(lib().sn_bucket_pack(C.byref(a), stream()), "sn_bucket_pack")
    return N, E, B, S


def bucket_validity(module):
    """Row validity of a PADDED batch while a bucketed step (train_graph.BucketedStep / DGLBucketedStep) runs `module` (its switch
    `_bucket`, set only during the step's warm-up and capture): the (node, edge, graph) 0/1 vectors bucket_pack / bucket_pack_dgl
    wrote and K = 1 — the nvalid, K every op over plain node / edge / graph rows takes, so padding rows enter no batch statistic and
    no parameter gradient.  Without the switch (None, None, None, 0): all rows valid, the arguments of the eager step."""
    pad = getattr(module, "_bucket", None)
    if pad is None:
        return None, None, None, 0
    return pad.node_valid, pad.edge_valid, pad.graph_valid, 1


class _BucketPackDglC(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("h", C.c_void_p), ("e", C.c_void_p), ("p", C.c_void_p),
                ("snorm_n", C.c_void_p), ("target", C.c_void_p), ("batch_num_nodes", C.c_void_p),
                ("N", C.c_int64), ("E", C.c_int64), ("B", C.c_int64), ("K", C.c_int64),
                ("src_out", C.c_void_p), ("dst_out", C.c_void_p), ("h_out", C.c_void_p), ("e_out", C.c_void_p), ("p_out", C.c_void_p),
                ("snorm_n_out", C.c_void_p), ("target_out", C.c_void_p), ("batch_num_nodes_out", C.c_void_p),
                ("node_valid", C.c_void_p), ("edge_valid", C.c_void_p), ("graph_valid", C.c_void_p), ("node_slots", C.c_void_p),
                ("counts", C.c_void_p), ("count_error", C.c_void_p), ("N_cap", C.c_int64), ("E_cap", C.c_int64), ("B_cap", C.c_int64)]


NODE_COUNT_ERROR = "batch_num_nodes does not sum to the number of feature rows"      # (the eager step's message: dgl_nets / dgl_deepsigns _plan)


def check_node_total(bnn, N):
    """A host-side batch_num_nodes() (a DGL batch on the CPU, a list of sizes) must sum to the N feature rows: the ValueError of the
    eager step, raised before any launch.  Device counts are checked by sn_bucket_pack_dgl itself (count_error)."""
    if not (torch.is_tensor(bnn) and bnn.is_cuda):
        t = torch.as_tensor(bnn)
        if int(t.sum()) != int(N) or (t.numel() and int(t.min()) < 0):
            raise ValueError(NODE_COUNT_ERROR)


def bucket_pack_dgl(g, h, p, e, snorm_n, target, out):
    """Copy a DGL batch of any shape — `g` (only edges() and batch_num_nodes() are read), atom ids h [N] / [N, 1], pos_enc p [N, K],
    bond ids e [E] or None, snorm_n [N, 1] or None, targets [B, 1] — into the capacity buffers `out` (a DGLPaddedBatch of train_graph)
    in ONE launch (sn_bucket_pack_dgl): the padding, the padded per-graph node counts, the node / edge / graph validity, the node-slot
    vector and the device count block [N, E, B] too.  No device read; a host-side batch_num_nodes() is checked against N here (ValueError)
    and copied through pinned memory; device counts that do not sum to N set out.count_error instead (the padded counts then still
    total N_cap: one graph holds every node)."""
    src, dst = g.edges()
    dev = out.h.device
    src, dst = src.long().contiguous(), dst.long().contiguous()
    bnn = torch.as_tensor(g.batch_num_nodes())
    check_node_total(bnn, h.shape[0])
    if bnn.is_cuda:
        bnn = bnn.long().contiguous()
    else:
        bnn = bnn.long().contiguous().pin_memory().to(dev, non_blocking=True)
    hh = h.long().reshape(-1).contiguous()
    pp = p.contiguous()
    t = target.contiguous()
    ee = None if e is None else e.long().reshape(-1).contiguous()
    sn = None if snorm_n is None else snorm_n.reshape(-1).contiguous()
    require_cuda(src, dst, hh, pp, t, ee, sn)
    N, E, B = hh.numel(), src.numel(), bnn.numel()
    if dst.numel() != E:
        raise ValueError(f"bucket_pack_dgl: src has {E} edges, dst {dst.numel()}")
    if pp.dtype != torch.float32 or tuple(pp.shape) != (N, out.K):
        raise ValueError(f"bucket_pack_dgl: p is {pp.dtype} {tuple(pp.shape)}, the bucket holds float32 [N, {out.K}] with N = {N}")
    if t.dtype != torch.float32 or t.numel() != B:
        raise ValueError(f"bucket_pack_dgl: targets {t.dtype} {tuple(t.shape)} for {B} graphs (one float32 score per graph)")
    for name, src_t, dst_t, n in (("e", ee, out.e, E), ("snorm_n", sn, out.snorm_n, N)):
        if (src_t is None) != (dst_t is None):
            raise ValueError(f"bucket_pack_dgl: {name} is {'missing' if src_t is None else 'given'}, the bucket was captured "
                             f"{'with' if src_t is None else 'without'} it")
        if src_t is not None and (src_t.numel() != n or src_t.dtype != dst_t.dtype):
            raise ValueError(f"bucket_pack_dgl: {name} is {src_t.dtype} with {src_t.numel()} entries, expected {dst_t.dtype} x {n}")
    a = _BucketPackDglC(ptr(src), ptr(dst), ptr(hh), ptr(ee), ptr(pp), ptr(sn), ptr(t), ptr(bnn), N, E, B, out.K,
                        ptr(out.src), ptr(out.dst), ptr(out.h), ptr(out.e), ptr(out.p), ptr(out.snorm_n), ptr(out.target),
                        ptr(out.batch_num_nodes), ptr(out.node_valid), ptr(out.edge_valid), ptr(out.graph_valid), ptr(out.node_slots),
                        ptr(out.counts), ptr(out.count_error), out.N_cap, out.E_cap, out.B_cap)
    with _span("sn_bucket_pack_dgl"):
        check(lib().sn_bucket_pack_dgl(C.byref(a), stream()), "sn_bucket_pack_dgl")
    return N, E, B


# ----------------------------------------------------------------------------- device-resident graph store (data.GraphStore)
STORE_NODE, STORE_EDGE, STORE_EIG, STORE_GRAPH = 0, 1, 2, 3
GATHER_COPY, GATHER_ENDPOINT, GATHER_GRAPH_ID, GATHER_CONST, GATHER_NODE_COUNT = 0, 1, 2, 3, 4
STORE_MAX_SEGS = 12
GATHER_BAD_INDEX, GATHER_MISMATCH = 1, 2          # flags of status[0]
STORE_INDEX_ERROR = "graph index out of range: a batch index lies outside [0, num_graphs) of the store"
STORE_TOTALS_ERROR = ("the graphs selected on the device do not have the node / edge / eigenvector totals the host computed "
                      "(the device index view does not hold the host's indices): the batch was replaced by padding")


class _StoreSegC(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64), ("kind", C.c_int32), ("op", C.c_int32),
                ("val", C.c_int32), ("reserved", C.c_int32)]


class _StoreGatherC(C.Structure):
    _fields_ = [("node_ptr", C.c_void_p), ("edge_ptr", C.c_void_p), ("eig_ptr", C.c_void_p), ("G", C.c_int64),
                ("index", C.c_void_p), ("B", C.c_int64), ("N", C.c_int64), ("E", C.c_int64), ("S", C.c_int64),
                ("N_cap", C.c_int64), ("E_cap", C.c_int64), ("B_cap", C.c_int64), ("S_cap", C.c_int64),
                ("exact", C.c_int32), ("nseg", C.c_int32), ("seg", _StoreSegC * STORE_MAX_SEGS),
                ("counts", C.c_void_p), ("ncounts", C.c_int64), ("count_error", C.c_void_p), ("status", C.c_void_p)]


def store_gather_max_graphs() -> int:
    return int(lib().sn_store_gather_max_graphs())


def store_gather_args(tables, G, caps, segs, status, counts=None, count_error=None, exact=False):
    """The parameter block of sn_store_gather for one (store, destination) pair, built once and reused every step (store_gather fills
    in the index view and the totals).  tables: (node_ptr, edge_ptr, eig_ptr or None), int64 [G + 1] on the device; caps: (N_cap,
    E_cap, B_cap, S_cap); segs: (src or None, dst, kind, op, val) — `dst` one capacity array [rows of its kind, ...], `src` the store's
    concatenated array of the same dtype and row shape (GATHER_COPY, GATHER_ENDPOINT).  Raises ValueError for a dtype / row-shape
    mismatch, a table that is not int64 or more than STORE_MAX_SEGS segments; the library checks alignment and capacities."""
    node_ptr, edge_ptr, eig_ptr = tables
    for name, t in (("node_ptr", node_ptr), ("edge_ptr", edge_ptr), ("eig_ptr", eig_ptr)):
        if t is not None and (t.dtype != torch.int64 or t.numel() != G + 1 or not t.is_contiguous()):
            raise ValueError(f"store_gather: {name} must be a contiguous int64 [G + 1] = [{G + 1}] table, got {t.dtype} {tuple(t.shape)}")
    if len(segs) > STORE_MAX_SEGS:
        raise ValueError(f"store_gather: {len(segs)} segments (at most {STORE_MAX_SEGS})")
    if status.dtype != torch.int32 or status.numel() < 4:
        raise ValueError("store_gather: status must be int32 [4]")
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() not in (3, 4)):
        raise ValueError("store_gather: the count block is int32 [3] or [4]")
    if count_error is not None and (count_error.dtype != torch.int32 or count_error.numel() < 1):
        raise ValueError("store_gather: count_error is int32 [1]")
    require_cuda(node_ptr, edge_ptr, eig_ptr, status, counts, count_error)
    a = _StoreGatherC()
    a.node_ptr, a.edge_ptr, a.eig_ptr, a.G = ptr(node_ptr), ptr(edge_ptr), ptr(eig_ptr), G
    a.N_cap, a.E_cap, a.B_cap, a.S_cap = (int(c) for c in caps)
    a.exact, a.nseg = int(bool(exact)), len(segs)
    wide = {GATHER_ENDPOINT: "edge endpoints", GATHER_GRAPH_ID: "the batch vector", GATHER_NODE_COUNT: "the node counts"}
    for i, (src, dst, kind, op, val) in enumerate(segs):
        require_cuda(src, dst)
        if not dst.is_contiguous() or (src is not None and not src.is_contiguous()):
            raise ValueError(f"store_gather: segment {i} is not contiguous")
        if kind not in (STORE_NODE, STORE_EDGE, STORE_EIG, STORE_GRAPH) or dst.dim() < 1 or \
                dst.shape[0] != (a.N_cap, a.E_cap, a.S_cap, a.B_cap)[kind]:
            raise ValueError(f"store_gather: segment {i} (kind {kind}) has {tuple(dst.shape)} rows, the capacities are "
                             f"N {a.N_cap}, E {a.E_cap}, B {a.B_cap}, S {a.S_cap}")
        if op in (GATHER_COPY, GATHER_ENDPOINT):
            if src is None or src.dtype != dst.dtype or tuple(src.shape[1:]) != tuple(dst.shape[1:]):
                raise ValueError(f"store_gather: segment {i}: the store holds {None if src is None else src.dtype} rows of "
                                 f"{None if src is None else tuple(src.shape[1:])}, the destination {dst.dtype} rows of {tuple(dst.shape[1:])}")
        if op in wide and dst.dtype != torch.int64:
            raise ValueError(f"store_gather: segment {i}: {wide[op]} are int64, the destination is {dst.dtype}")
        if op == GATHER_CONST and dst.dtype != torch.int32:
            raise ValueError(f"store_gather: segment {i}: a constant segment is int32, the destination is {dst.dtype}")
        s = a.seg[i]
        row = dst.element_size()
        for d in dst.shape[1:]:
            row *= int(d)               # (not _row_bytes: an exact-size destination may have no rows)
        s.src, s.dst, s.row_bytes, s.kind, s.op, s.val = ptr(src), ptr(dst), row, kind, op, int(val)
    a.counts, a.ncounts = ptr(counts), (0 if counts is None else counts.numel())
    a.count_error, a.status = ptr(count_error), ptr(status)
    return a


def store_gather(args, index, B, totals):
    """ONE launch (sn_store_gather): the B graphs `index` (int64, on the device: a view of the epoch's permutation) of the store go into
    the destination of `args` (store_gather_args).  totals: (N, E, S) of those graphs, from the host's copies of the size tables."""
    if index.dtype != torch.int64 or not index.is_contiguous() or index.numel() < B:
        raise ValueError(f"store_gather: index must be contiguous int64 with >= {B} entries, got {index.dtype} {tuple(index.shape)}")
    require_cuda(index)
    args.index, args.B = ptr(index), int(B)
    args.N, args.E, args.S = (int(v) for v in totals)
    with _span("sn_store_gather"):
        check(lib().sn_store_gather(C.byref(args), stream()), "sn_store_gather")


# ----------------------------------------------------------------------------- handle_lap's network-free branches (dgl_nets.handle_lap)
LAP_NONE, LAP_SIGN_FLIP, LAP_ABS_VAL, LAP_CANONICAL = 0, 1, 2, 3          # SN_LAP_* of include/signnet_hip.h
LAP_MODES = {"none": LAP_NONE, "sign_flip": LAP_SIGN_FLIP, "abs_val": LAP_ABS_VAL, "canonical": LAP_CANONICAL}


def lap_pe_transform(p, mode, u=None, graph_ptr=None, out=None):
    """ONE launch (sn_lap_pe_transform_f32), no host read: the positional encoding p [N, K] (float32, unit column stride) through
    `mode` — 'none' (copy), 'sign_flip' (column c times +1 if u[c] >= 0.5 else -1; u [K] float32 on the device), 'abs_val', 'canonical'
    (per graph and column: times -1 if there are fewer non-negative than negative entries or their sum is smaller than the negatives'
    absolute sum; graph_ptr [B + 1] int32 node offsets, a GraphPlan's) — or the SN_LAP_* integer.  `out`: the destination (may be p
    itself), else a new tensor.  Rows at or beyond graph_ptr[B] are copied."""
    m = LAP_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if m not in (LAP_NONE, LAP_SIGN_FLIP, LAP_ABS_VAL, LAP_CANONICAL):
        raise ValueError(f"lap_pe_transform: unknown mode {mode!r} (one of {sorted(LAP_MODES)})")
    require_cuda(p, u, graph_ptr, out)
    if p.dim() != 2 or p.dtype != torch.float32 or (p.shape[1] > 1 and p.stride(1) != 1):
        raise ValueError(f"lap_pe_transform: p must be float32 [N, K] with unit column stride, got {p.dtype} {tuple(p.shape)}")
    N, K = p.shape
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=p.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, K) or (K > 1 and out.stride(1) != 1):
        raise ValueError(f"lap_pe_transform: out must be float32 {(N, K)} with unit column stride, got {out.dtype} {tuple(out.shape)}")
    B = 0
    if m == LAP_SIGN_FLIP:
        if u is None or u.dtype != torch.float32 or u.numel() != K or not u.is_contiguous():
            raise ValueError(f"lap_pe_transform: sign_flip needs u, contiguous float32 [{K}]")
    if m == LAP_CANONICAL:
        if graph_ptr is None or graph_ptr.dtype != torch.int32 or graph_ptr.numel() < 1 or not graph_ptr.is_contiguous():
            raise ValueError("lap_pe_transform: canonical needs graph_ptr, contiguous int32 [B + 1]")
        B = graph_ptr.numel() - 1
    ldp = p.stride(0) if N > 1 else max(K, 1)
    ldo = out.stride(0) if N > 1 else max(K, 1)
    with _span("sn_lap_pe_transform_f32"):
        check(lib().sn_lap_pe_transform_f32(ptr(p), ldp, ptr(out), ldo, N, K, m, ptr(u) if m == LAP_SIGN_FLIP else None,
                                            ptr(graph_ptr) if m == LAP_CANONICAL else None, B, stream()), "sn_lap_pe_transform_f32")
    return out


# ----------------------------------------------------------------------------- Set2Set readout (Alchemy/baseline_gin.py:43,58)
def set2set(x, graph_ptr, w_ih, w_hh, b_ih, b_hh, steps, want_tape=False):
    """PyG's Set2Set(d, processing_steps=steps) with one LSTM layer, one launch: x [N, d], graph_ptr int32 [B+1], the four tensors of
    torch.nn.LSTM(2d, d) under their state_dict names -> q* [B, 2d].  want_tape: also the tape sn_set2set_bwd_f32 reads
    (in [T,B,3d], act [T,B,4d], cell [T,B,d], e [T,N], md [T,B,2]).  Graph b owns rows graph_ptr[b] .. graph_ptr[b+1] of x; the entries
    live on the device, so they are not read here: the kernel clamps them into [0, N] and rows outside every graph belong to none (a batch
    plan's graph_ptr — ops.build_plan — always ends at N)."""
    require_cuda(x, graph_ptr, w_ih, w_hh, b_ih, b_hh)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) != x.shape[1]):
        raise ValueError("set2set: x must be a dense float32 [N, d] block")
    if graph_ptr.dtype != torch.int32 or not graph_ptr.is_contiguous():
        raise ValueError("set2set: graph_ptr must be contiguous int32 [B+1]")
    if graph_ptr.dim() != 1 or graph_ptr.numel() < 1:
        raise ValueError("set2set: graph_ptr needs at least one entry (B + 1 node offsets, the last one N)")
    N, d = x.shape
    B, T = graph_ptr.numel() - 1, int(steps)
    if tuple(w_ih.shape) != (4 * d, 2 * d) or tuple(w_hh.shape) != (4 * d, d) or b_ih.numel() != 4 * d or b_hh.numel() != 4 * d:
        raise ValueError(f"set2set: LSTM tensors do not match d = {d}")
    w_ih, w_hh, b_ih, b_hh = (_f32c(t, n) for t, n in ((w_ih, "weight_ih_l0"), (w_hh, "weight_hh_l0"), (b_ih, "bias_ih_l0"), (b_hh, "bias_hh_l0")))
    dev = x.device
    out = torch.empty(B, 2 * d, dtype=torch.float32, device=dev)
    work = torch.empty(12 * d * d + 4 * d, dtype=torch.float32, device=dev)
    tape = None
    if want_tape:
        tape = tuple(torch.empty(s, dtype=torch.float32, device=dev)
                     for s in ((T, B, 3 * d), (T, B, 4 * d), (T, B, d), (T, N), (T, B, 2)))
    tp = [ptr(t) for t in tape] if tape is not None else [None] * 5
    with _span("sn_set2set_f32"):
        check(lib().sn_set2set_f32(ptr(x), N, d, ptr(graph_ptr), B, ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), T, ptr(out), ptr(work),
                                   *tp, stream()), "sn_set2set_f32")
    return (out, tape) if want_tape else out


# ----------------------------------------------------------------------------- polynomial filters of one sparse operator (csrc/poly_filter.hip)
POLY_MONOMIAL, POLY_CHEBYSHEV = 0, 1
POLY_MODES = {"monomial": POLY_MONOMIAL, "chebyshev": POLY_CHEBYSHEV}


@dataclass
class SparseOperator:
    """W of S = diag_add * I + scale * W in CSR by destination, for ONE graph of N nodes: (W x)_i = sum over e in row i of w[e] x[col[e]].
    `t` is the operator of W^T (the adjoints run over it); filter_baselines.FilterGraph builds both."""
    rowptr: torch.Tensor      # int32 [N + 1]
    col: torch.Tensor         # int32 [nnz]
    w: torch.Tensor           # float32 [nnz]
    N: int
    t: "SparseOperator" = None

    @property
    def nnz(self):
        return self.col.numel()


def poly_filter_max_nodes(K, mode="monomial"):
    """The LDS-bound node capacity of sn_poly_basis_f32 / sn_poly_combine_f32."""
    return int(lib().sn_poly_filter_max_nodes(int(K), POLY_MODES.get(mode, mode)))


def _poly_check(fn, op, K, mode, x):
    m = POLY_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if m not in (POLY_MONOMIAL, POLY_CHEBYSHEV):
        raise ValueError(f"{fn}: unknown mode {mode!r} (one of {sorted(POLY_MODES)})")
    K = int(K)
    if K < 0:
        raise ValueError(f"{fn}: K must be >= 0")
    cap = poly_filter_max_nodes(K, m)
    if op.N > cap:                                   # before any launch (and before the tensors are looked at)
        raise ValueError(f"{fn}: the graph has {op.N} nodes, above the LDS-bound capacity {cap} of the polynomial-filter kernels")
    require_cuda(x, op.rowptr, op.col, op.w)
    if op.N < 1 or op.rowptr.dtype != torch.int32 or op.rowptr.numel() != op.N + 1 or op.col.dtype != torch.int32 or \
            op.w.dtype != torch.float32 or op.w.numel() != op.nnz:
        raise ValueError(f"{fn}: malformed SparseOperator")
    return K, m


def _stack_strides(fn, t, N, d, K, name):
    """(sk, ld) of a [N, d] block shared by every k or a [K+1, N, d] stack: unit channel stride, any node / k strides."""
    if t.dtype not in (torch.float32, torch.float64) or t.stride(-1) != 1 and d > 1:
        raise ValueError(f"{fn}: {name} must be float32 (or a float64 stack) with unit channel stride")
    if t.dim() == 2 and tuple(t.shape) == (N, d):
        return 0, (t.stride(0) if N > 1 else d)
    if t.dim() == 3 and tuple(t.shape) == (K + 1, N, d):
        return (t.stride(0) if K > 0 else 0), (t.stride(1) if N > 1 else d)
    raise ValueError(f"{fn}: {name} must be [N, d] = {(N, d)} or [K+1, N, d] = {(K + 1, N, d)}, got {tuple(t.shape)}")


def poly_basis(x, op: SparseOperator, K, mode="monomial", diag_add=0.0, scale=1.0, *, want_stack=True, g=None, g_reverse=False,
               stack_dtype=torch.float32):
    """B_k = P_k(S) x, k = 0..K, in ONE launch (sn_poly_basis_f32): x [N, d] -> B [K+1, N, d] (want_stack=False: not
    stored).  g ([N, d] or a [K+1, N, d] stack, read in reverse order with g_reverse): also
    dots [K+1] = <B_k, g_k>, the per-slice partials finished in slice order by sn_train_reduce_parts_f32.  Returns B, dots or (B, dots).
    stack_dtype=torch.float64 (and a float64 `g`): the stack holds the kernel's doubles unrounded — for a stack that goes straight
    into poly_combine or back into poly_basis as `g` (Bernstein), where an fp32 rounding in between is amplified by the second launch."""
    K, m = _poly_check("poly_basis", op, K, mode, x)
    require_cuda(g)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] != op.N:
        raise ValueError(f"poly_basis: x must be contiguous float32 [N = {op.N}, d], got {x.dtype} {tuple(x.shape)}")
    N, d = x.shape
    B, bs = None, (0, d)
    if want_stack:
        if stack_dtype not in (torch.float32, torch.float64):
            raise ValueError("poly_basis: stack_dtype must be torch.float32 or torch.float64")
        B = torch.empty(K + 1, N, d, dtype=stack_dtype, device=x.device)
        bs = (N * d, d)
    elif g is None:
        raise ValueError("poly_basis: nothing to compute (want_stack=False and no g)")
    part = dots = None
    gs = (0, d)
    if g is not None:
        gs = _stack_strides("poly_basis", g, N, d, K, "g")
        slices = int(lib().sn_poly_filter_launch_shape(N, d, None, None))
        part = torch.empty(slices, K + 1, dtype=torch.float32, device=x.device)
        dots = torch.empty(K + 1, dtype=torch.float32, device=x.device)
    with _span("sn_poly_basis_f32"):
        check(lib().sn_poly_basis_f32(ptr(x), N, d, K, m, ptr(op.rowptr), ptr(op.col), ptr(op.w), op.nnz, float(diag_add), float(scale),
                                      ptr(B), bs[0], bs[1], int(B is not None and B.dtype == torch.float64), ptr(g), gs[0], gs[1],
                                      int(bool(g_reverse)), int(g is not None and g.dtype == torch.float64), ptr(part), stream()),
              "sn_poly_basis_f32")
    if part is not None:
        with _span("sn_train_reduce_parts_f32"):
            check(lib().sn_train_reduce_parts_f32(ptr(part), part.shape[0], K + 1, K + 1, ptr(dots), 0, stream()), "sn_train_reduce_parts_f32")
    return dots if B is None else (B if dots is None else (B, dots))


def poly_combine(a, op: SparseOperator, K, mode="monomial", diag_add=0.0, scale=1.0, c=None, reverse=False):
    """y [N, d] = sum_k c[k] P_k(S) a_k in ONE launch (sn_poly_combine_f32; Horner / Clenshaw, K applications of S).  a: [N, d] shared by
    every k, or a [K+1, N, d] stack (any k / node strides; float32 or float64), read in reverse order with reverse=True.  c: float32 [K+1] on the device, or
    None for ones."""
    K, m = _poly_check("poly_combine", op, K, mode, a)
    require_cuda(c)
    N, d = op.N, a.shape[-1]
    sk, ld = _stack_strides("poly_combine", a, N, d, K, "a")
    if c is not None and (c.dtype != torch.float32 or c.numel() != K + 1 or not c.is_contiguous()):
        raise ValueError(f"poly_combine: c must be contiguous float32 [{K + 1}]")
    y = torch.empty(N, d, dtype=torch.float32, device=a.device)
    with _span("sn_poly_combine_f32"):
        check(lib().sn_poly_combine_f32(ptr(a), sk, ld, int(bool(reverse)), int(a.dtype == torch.float64), N, d, K, m, ptr(op.rowptr), ptr(op.col), ptr(op.w), op.nnz,
                                        float(diag_add), float(scale), ptr(c), ptr(y), stream()), "sn_poly_combine_f32")
    return y


# ----------------------------------------------------------------------------- PyG's GATConv on one fixed graph (csrc/filter_attention.hip)
GAT_ACT_NONE, GAT_ACT_ELU = 0, 1
GAT_ACTS = {None: GAT_ACT_NONE, "none": GAT_ACT_NONE, "elu": GAT_ACT_ELU}


def gat_conv_limits():
    """(max heads, max channels per head) of sn_gat_conv_f32 / sn_gat_conv_bwd_f32."""
    return int(lib().sn_gat_conv_max_heads()), int(lib().sn_gat_conv_max_channels())


def gat_conv_group_width(C):
    """Lanes that own one (node, head) of C channels: min(64, the power of two >= C); 0 outside the limits.  The kernel's only dispatch
    thresholds are the widths at which this doubles, and C = 64 -> 65 (one -> two channels per lane)."""
    return int(lib().sn_gat_conv_group_width(int(C)))


def _gat_check(fn, feat, att_l, att_r, bias, op, heads, act):
    a = GAT_ACTS.get(act, act) if act is None or isinstance(act, str) else act
    if a not in (GAT_ACT_NONE, GAT_ACT_ELU):
        raise ValueError(f"{fn}: act must be one of {sorted(k for k in GAT_ACTS if k)} (or None / 0 / 1), got {act!r}")
    heads = int(heads)
    if heads < 1 or feat.dim() != 2 or feat.shape[1] < heads or feat.shape[1] % heads:
        raise ValueError(f"{fn}: feat must be [N, heads * C] with heads = {heads} >= 1, got {tuple(feat.shape)}")
    Cc = feat.shape[1] // heads
    mh, mc = gat_conv_limits()
    if heads > mh or Cc > mc:                         # before any launch (and before the tensors are looked at)
        raise ValueError(f"{fn}: heads = {heads}, C = {Cc} is beyond the kernel's limits (heads <= {mh}, C <= {mc})")
    require_cuda(feat, att_l, att_r, bias, op.rowptr, op.col)
    # (op.nnz IS op.col.numel(): the kernels clamp rowptr to exactly the entries col holds, provided both arrays are dense in memory)
    if op.N < 1 or feat.shape[0] != op.N or op.rowptr.dtype != torch.int32 or op.rowptr.numel() != op.N + 1 or op.col.dtype != torch.int32 \
            or op.col.dim() != 1 or not op.col.is_contiguous() or not op.rowptr.is_contiguous():
        raise ValueError(f"{fn}: feat has {feat.shape[0]} rows; the operator must be a contiguous CSR (int32) of as many nodes")
    feat = _f32c(feat, "feat")
    vecs = [None if t is None else _f32c(t.reshape(-1), n) for t, n in ((att_l, "att_l"), (att_r, "att_r"), (bias, "bias"))]
    if vecs[0] is None or vecs[1] is None or any(v is not None and v.numel() != heads * Cc for v in vecs):
        raise ValueError(f"{fn}: att_l, att_r (and bias, if given) must hold heads * C = {heads * Cc} values")
    return feat, vecs[0], vecs[1], vecs[2], heads, Cc, a


def gat_conv(feat, att_l, att_r, bias, op: SparseOperator, heads, act="elu", negative_slope=0.2):
    """torch_geometric's GATConv behind its Linear, with the activation that follows, in ONE launch (sn_gat_conv_f32).  feat [N, heads*C]:
    the Linear's output; att_l, att_r, bias (or None): heads*C values; op: the CSR by destination with the input self loops dropped
    (FilterGraph.lap's pattern; the weights are not read) — every node attends over its in-edges and itself.  act: 'elu' or None.
    -> (out [N, heads*C], lse [N, heads])."""
    feat, al, ar, b, heads, Cc, a = _gat_check("gat_conv", feat, att_l, att_r, bias, op, heads, act)
    N = op.N
    out = torch.empty(N, heads * Cc, dtype=torch.float32, device=feat.device)
    lse = torch.empty(N, heads, dtype=torch.float32, device=feat.device)
    with _span("sn_gat_conv_f32"):
        check(lib().sn_gat_conv_f32(ptr(feat), ptr(al), ptr(ar), ptr(b), N, heads, Cc, float(negative_slope), a, ptr(op.rowptr), ptr(op.col),
                                    op.nnz, ptr(out), ptr(lse), stream()), "sn_gat_conv_f32")
    return out, lse


def gat_conv_bwd(feat, att_l, att_r, out, lse, dout, op: SparseOperator, heads, act="elu", negative_slope=0.2):
    """Adjoint of gat_conv in two launches and one reduction (sn_gat_conv_bwd_f32, sn_train_reduce_parts_f32): op.t must be the operator
    of the flipped edge list.  dout is the cotangent of `out` (the activation's adjoint is applied inside, from `out`).
    -> (dfeat [N, heads*C], d att_l [heads*C], d att_r [heads*C], d bias [heads*C])."""
    feat, al, ar, _, heads, Cc, a = _gat_check("gat_conv_bwd", feat, att_l, att_r, None, op, heads, act)
    if op.t is None or op.t.N != op.N or op.t.nnz != op.nnz:
        raise ValueError("gat_conv_bwd: the operator has no transposed partner (.t) of the same size")
    require_cuda(out, lse, dout, op.t.rowptr, op.t.col)
    N, D = op.N, heads * Cc
    out, dout, lse = _f32c(out, "out"), _f32c(dout, "dout"), _f32c(lse, "lse")
    if tuple(out.shape) != (N, D) or tuple(dout.shape) != (N, D) or lse.numel() != N * heads:
        raise ValueError(f"gat_conv_bwd: out and dout must be [{N}, {D}], lse [{N}, {heads}]")
    blocks = int(lib().sn_gat_conv_bwd_blocks(N, heads, Cc))
    dfeat = torch.empty(N, D, dtype=torch.float32, device=feat.device)
    part = torch.empty(blocks, 3 * D, dtype=torch.float32, device=feat.device)
    work = torch.empty(5 * N * heads, dtype=torch.float64, device=feat.device)
    dpar = torch.empty(3 * D, dtype=torch.float32, device=feat.device)
    with _span("sn_gat_conv_bwd_f32"):
        check(lib().sn_gat_conv_bwd_f32(ptr(feat), ptr(al), ptr(ar), ptr(out), ptr(lse), ptr(dout), N, heads, Cc, float(negative_slope), a,
                                        ptr(op.rowptr), ptr(op.col), ptr(op.t.rowptr), ptr(op.t.col), op.nnz, ptr(dfeat), ptr(part),
                                        ptr(work), stream()), "sn_gat_conv_bwd_f32")
    with _span("sn_train_reduce_parts_f32"):
        check(lib().sn_train_reduce_parts_f32(ptr(part), blocks, 3 * D, 3 * D, ptr(dpar), 0, stream()), "sn_train_reduce_parts_f32")
    return dfeat, dpar[:D], dpar[D:2 * D], dpar[2 * D:]


def csr_drop_loops(plan: GraphPlan, rplan: GraphPlan):
    """The operator pair of gat_conv / gat_conv_bwd from a batch's two plans, on the device (sn_csr_drop_loops): the CSR by destination
    without the input self loops, rows in (source, input position) order — what pyg_gnn_types._gat_operator builds with boolean indexing
    and argsort — and its transposed partner, in buffers of the plans' sizes ([N + 1], [E]).  No shape depends on the data and nothing
    is read on the host: the form a captured step records.  The live entry count is rowptr[N] on the device; `nnz` is the capacity E.
    rplan: the plan of the flipped edge list."""
    if rplan.N != plan.N or rplan.E != plan.E or plan.N < 1:
        raise ValueError("csr_drop_loops: rplan must be the plan of the flipped edge list of the same batch (N >= 1)")
    N, E, dev = plan.N, plan.E, plan.rowptr.device
    buf = torch.empty(2 * (N + 1) + 2 * E, dtype=torch.int32, device=dev)
    rp, rpt, cl, clt = buf[:N + 1], buf[N + 1:2 * (N + 1)], buf[2 * (N + 1):2 * (N + 1) + E], buf[2 * (N + 1) + E:]
    with _span("sn_csr_drop_loops"):
        check(lib().sn_csr_drop_loops(N, E, ptr(plan.rowptr), ptr(plan.col), ptr(rplan.rowptr), ptr(rplan.col), ptr(rp), ptr(cl), ptr(rpt),
                                      ptr(clt), stream()), "sn_csr_drop_loops")
    fwd = SparseOperator(rp, cl, None, N)
    fwd.t = SparseOperator(rpt, clt, None, N, fwd)
    return fwd


_ONES = {}


def ones_vector(n, device):
    """A cached float32 vector of n ones (the unit scale of a bias-only masked_affine)."""
    key = (int(n), torch.device(device))
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones(int(n), dtype=torch.float32, device=device)
    return t


# ----------------------------------------------------------------------------- the 'gcn' / 'transformer' sign-invariant encoders (csrc/deepsigns_variants.hip)
def _row_block(t, name):
    """A float32 [R, C] block whose rows are contiguous (a column block of a wider row matrix, or a view at an offset) -> its row stride."""
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name}: expected a float32 [R, C] block with contiguous rows")
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def gcn_propagate(x, plan: GraphPlan, rplan: GraphPlan, bias=None, width=0):
    """dgl.nn.pytorch.GraphConv(norm='both') without its weight: out[i] = cin[i] * sum_{j -> i} cout[j] * x[j] (+ bias[c % width]) with
    cin / cout = clamp(in- / out-degree, 1)^-1/2 read from the two plans' row pointers (plan: sn_batch_plan of the batch, rplan: of its
    flipped edge list).  x: [N, C] with contiguous rows (any row stride).  The adjoint w.r.t. x is gcn_propagate(g, rplan, plan)."""
    require_cuda(x)
    ldx = _row_block(x, "gcn_propagate: x")
    N, Cc = x.shape
    if plan.N != N or rplan.N != N:
        raise ValueError(f"gcn_propagate: x has {N} rows, the plans {plan.N} and {rplan.N} nodes")
    if bias is not None:
        bias = _f32c(bias, "bias")
        if int(width) <= 0 or bias.numel() != int(width) or Cc % int(width):
            raise ValueError("gcn_propagate: bias must be [width] with width dividing the row length")
    out = torch.empty(N, Cc, dtype=torch.float32, device=x.device)
    if N == 0:
        return out
    with _span("sn_gcn_propagate_f32"):
        check(lib().sn_gcn_propagate_f32(ptr(x), ldx, N, Cc, ptr(plan.rowptr), ptr(plan.col), ptr(rplan.rowptr), ptr(bias), int(width),
                                         ptr(out), Cc, stream()), "sn_gcn_propagate_f32")
    return out


GRAPH_ATTENTION_MAX_HEAD = 64


def graph_attention(q, k, v, graph_ptr, N, S, heads):
    """Multi-head self-attention over the nodes of each graph, independently per slot (dgl's SetTransformerEncoder block 'sab'): a set is
    (graph, slot), its rows node * S + slot.  q, k, v: [N*S, heads*dh] blocks with one common row stride (column blocks of one
    projection); graph_ptr: int32 [B+1].  -> (out [N*S, heads*dh], lse [N*S, heads]).  dh <= 64."""
    require_cuda(q, k, v)
    ld = _row_block(q, "graph_attention: q")
    R, D = q.shape
    if k.shape != q.shape or v.shape != q.shape or _row_block(k, "graph_attention: k") != ld or _row_block(v, "graph_attention: v") != ld:
        raise ValueError("graph_attention: q, k, v must be blocks of one shape and one row stride")
    if D % heads or R != int(N) * int(S):
        raise ValueError("graph_attention: expected N * S rows of heads * dh columns")
    B = graph_ptr.numel() - 1
    out = torch.empty(R, D, dtype=torch.float32, device=q.device)
    lse = torch.empty(R, heads, dtype=torch.float32, device=q.device)
    with _span("sn_graph_attention_f32"):
        check(lib().sn_graph_attention_f32(ptr(q), ptr(k), ptr(v), ld, ptr(graph_ptr), int(N), B, int(S), int(heads), D // heads, ptr(out), D,
                                           ptr(lse), stream()), "sn_graph_attention_f32")
    return out, lse


def graph_attention_bwd(q, k, v, out, lse, dout, graph_ptr, N, S, heads):
    """Adjoint of graph_attention -> dqkv [N*S, 3 * heads*dh] (column blocks dq | dk | dv).  Rows of empty graphs do not exist; every
    row of the result is written."""
    ld = _row_block(q, "graph_attention_bwd: q")
    R, D = q.shape
    out, dout, lse = _f32c(out, "out"), _f32c(dout, "dout"), _f32c(lse, "lse")
    B = graph_ptr.numel() - 1
    g = torch.empty(R, 3 * D, dtype=torch.float32, device=q.device)
    delta = torch.empty(R, heads, dtype=torch.float32, device=q.device)
    with _span("sn_graph_attention_bwd_f32"):
        check(lib().sn_graph_attention_bwd_f32(ptr(q), ptr(k), ptr(v), ld, ptr(out), D, ptr(lse), ptr(dout), D, ptr(graph_ptr), int(N), B,
                                               int(S), int(heads), D // heads, ptr(g), ptr(g[:, D:]), ptr(g[:, 2 * D:]), 3 * D, ptr(delta),
                                               stream()), "sn_graph_attention_bwd_f32")
    return g


# ----------------------------------------------------------------------------- SimplifiedPNAConv's message side (csrc/simplified_pna.hip)
SPNA_MAX_CHANNELS = 384      # SN_SPNA_MAX_CHANNELS


def spna_vector_path(C, strides, pointers):
    """The dispatch predicate of the sn_spna_* launches, restated on the host: 16-byte accesses (a thread owns four consecutive channels)
    iff C and every row stride are multiples of 4 and every pointer is 16-byte aligned; one channel per thread otherwise."""
    return C % 4 == 0 and all(int(s) % 4 == 0 for s in strides) and all(int(p) % 16 == 0 for p in pointers)


def spna_cut(N, C, vector):
    """How the two column-reduction launches (statistics, adjoint sums) cut their work: (workgroups over consecutive node ranges, nodes per
    workgroup, column chunks, channel groups per chunk, node slots per workgroup) — make_cut of csrc/simplified_pna.hip."""
    G = C // 4 if vector else C
    ny = -(-G // 256)
    gw = -(-G // ny)
    slots = 256 // gw
    want = min(-(-max(int(N), 1) // (slots * 4)), 256)
    npb = -(-max(int(N), 1) // want)
    return -(-max(int(N), 1) // npb), npb, ny, gw, slots


def _spna_operands(fn, a, b, q, plan):
    require_cuda(a, b, q)
    lda, ldb, ldq = _row_block(a, fn + ": a"), _row_block(b, fn + ": b"), _row_block(q, fn + ": q")
    N, Cc = a.shape
    if b.shape != a.shape or q.shape[1] != Cc or q.shape[0] != plan.E or plan.N != N:
        raise ValueError(f"{fn}: a, b must be [N, C] and q [E, C] blocks of the plan's batch (N = {plan.N}, E = {plan.E})")
    if not 3 <= Cc <= SPNA_MAX_CHANNELS:
        raise ValueError(f"{fn}: C = {Cc} is outside [3, {SPNA_MAX_CHANNELS}]")
    return (ptr(a), lda, ptr(b), ldb, ptr(q), ldq, Cc, N, plan.E, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm)), N, Cc


def _spna_mask(fn, node_valid, counts, N):
    require_cuda(node_valid, counts)
    if counts is None or node_valid.dtype != torch.int32 or counts.dtype != torch.int32 or node_valid.numel() != N or counts.numel() < 2 \
            or not node_valid.is_contiguous() or not counts.is_contiguous():
        raise ValueError(f"{fn}: node_valid must be a contiguous int32 [N] vector and counts the int32 count block of the padded batch")


def spna_stats(a, b, q, plan: GraphPlan, bn, node_valid=None, counts=None):
    """Train-mode statistics of pre_nn.norms.0 over the E rows z_e = a[dst] + b[src] + q[e], formed on the fly (sn_spna_stats_f32): ->
    (state [5, C] = mean | biased variance | rstd | scale | shift, count [1]); moves bn's running statistics as BatchNorm1d does.
    node_valid / counts (a padded batch: the bucket's 0/1 node vector and device count block): sn_spna_stats_masked_f32 — the in-edges of
    invalid nodes are left out and the row count is counts[1], read on the device."""
    args, N, Cc = _spna_operands("spna_stats", a, b, q, plan)
    if plan.E < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size [{plan.E}, {Cc}]")
    track = bn.track_running_stats and bn.running_mean is not None
    if track and bn.momentum is None:
        raise NotImplementedError("BatchNorm1d(momentum=None) (cumulative moving average) is not supported")
    out = torch.empty(5 * Cc + 4, dtype=torch.float32, device=a.device)
    work = torch.empty(int(lib().sn_spna_blocks(N, Cc)) * 3 * Cc, dtype=torch.float32, device=a.device)
    g = None if bn.weight is None else bn.weight.detach()
    be = None if bn.bias is None else bn.bias.detach()
    tail = (ptr(g), ptr(be), float(bn.eps), float(bn.momentum or 0.0), ptr(bn.running_mean) if track else None,
            ptr(bn.running_var) if track else None, ptr(out), ptr(out[5 * Cc:]), ptr(work), stream())
    if node_valid is not None:
        _spna_mask("spna_stats", node_valid, counts, N)
        with _span("sn_spna_stats_masked_f32"):
            check(lib().sn_spna_stats_masked_f32(*args, ptr(node_valid), ptr(counts), *tail), "sn_spna_stats_masked_f32")
    else:
        with _span("sn_spna_stats_f32"):
            check(lib().sn_spna_stats_f32(*args, *tail), "sn_spna_stats_f32")
    if track:
        _count_batch(bn)
    return out[:5 * Cc].view(5, Cc), out[5 * Cc:5 * Cc + 1]


def spna_mean(a, b, q, plan: GraphPlan, scale, shift, out=None):
    """r[i] = mean over i's in-edges of relu((a[i] + b[src] + q[e]) * scale + shift), zeros without in-edges (sn_spna_mean_f32) -> [N, C]."""
    args, N, Cc = _spna_operands("spna_mean", a, b, q, plan)
    if scale.numel() != Cc or shift.numel() != Cc:
        raise ValueError("spna_mean: scale and shift must have C entries")
    if out is None:
        out = torch.empty(N, Cc, dtype=torch.float32, device=a.device)
    elif out.shape != a.shape:
        raise ValueError("spna_mean: out must be an [N, C] block")
    ldr = _row_block(out, "spna_mean: out")
    with _span("sn_spna_mean_f32"):
        check(lib().sn_spna_mean_f32(*args, ptr(scale), ptr(shift), ptr(out), ldr, stream()), "sn_spna_mean_f32")
    return out


def spna_bwd(a, b, q, plan: GraphPlan, rplan: GraphPlan, dr, *, scale=None, shift=None, state=None, gamma=None, out=None,
             node_valid=None, counts=None):
    """Adjoint of spna_mean for dr [N, C] (sn_spna_bwd_f32).  state (from spna_stats): the train-mode BatchNorm backward, -> (dA, dB, dQ,
    dgamma, dbeta); state None: eval mode with the folded scale / shift, -> (dA, dB, dQ, None, None).  rplan: the plan of the flipped edge
    list.  out: optional (dA, dB, dQ) blocks to write into.  node_valid / counts (train mode over a padded batch, as spna_stats):
    sn_spna_bwd_masked_f32 — invalid nodes' in-edges enter no sum, the means divide by counts[1], their dQ / dA / dB rows are zero."""
    args, N, Cc = _spna_operands("spna_bwd", a, b, q, plan)
    require_cuda(dr)
    lddr = _row_block(dr, "spna_bwd: dr")
    if dr.shape != a.shape or rplan.N != N or rplan.E != plan.E:
        raise ValueError("spna_bwd: dr must be [N, C] and rplan the plan of the flipped edge list")
    dev = a.device
    if out is None:
        dA, dB, dQ = (torch.empty(N, Cc, dtype=torch.float32, device=dev), torch.empty(N, Cc, dtype=torch.float32, device=dev),
                      torch.empty(plan.E, Cc, dtype=torch.float32, device=dev))
    else:
        dA, dB, dQ = out
    ld = [_row_block(t, "spna_bwd: out") for t in (dA, dB, dQ)]
    dg = db = work = None
    if state is not None:
        state = _f32c(state, "state")
        par = torch.empty(2, Cc, dtype=torch.float32, device=dev)
        dg, db = par[0], par[1]
        work = torch.empty(int(lib().sn_spna_blocks(N, Cc)) * 2 * Cc + 3 * Cc, dtype=torch.float32, device=dev)
    if node_valid is not None:
        _spna_mask("spna_bwd", node_valid, counts, N)
        if state is None:
            raise ValueError("spna_bwd: the masked form is the train-mode adjoint (state from spna_stats)")
        with _span("sn_spna_bwd_masked_f32"):
            check(lib().sn_spna_bwd_masked_f32(*args, ptr(rplan.rowptr), ptr(rplan.eperm), ptr(node_valid), ptr(counts), ptr(dr), lddr,
                                               ptr(state), ptr(gamma), ptr(dA), ld[0], ptr(dB), ld[1], ptr(dQ), ld[2], ptr(dg), ptr(db),
                                               ptr(work), stream()), "sn_spna_bwd_masked_f32")
        return dA, dB, dQ, dg, db
    with _span("sn_spna_bwd_f32"):
        check(lib().sn_spna_bwd_f32(*args, ptr(rplan.rowptr), ptr(rplan.eperm), ptr(dr), lddr, ptr(scale), ptr(shift), ptr(state),
                                    ptr(gamma), ptr(dA), ld[0], ptr(dB), ld[1], ptr(dQ), ld[2], ptr(dg), ptr(db), ptr(work), stream()),
              "sn_spna_bwd_f32")
    return dA, dB, dQ, dg, db


# ----------------------------------------------------------------------------- PyG's GCNConv propagation (csrc/pyg_gcn.hip)
def gcn_pyg_coef(plan: GraphPlan):
    """dis [N] = (1 + in-degree without self loops)^-1/2: both factors of torch_geometric's gcn_norm (add_self_loops=True, unit weights)."""
    dis = torch.empty(plan.N, dtype=torch.float32, device=plan.rowptr.device)
    with _span("sn_gcn_pyg_coef_f32"):
        check(lib().sn_gcn_pyg_coef_f32(plan.N, plan.E, ptr(plan.rowptr), ptr(plan.col), ptr(dis), stream()), "sn_gcn_pyg_coef_f32")
    return dis


def gcn_pyg_propagate(x, plan: GraphPlan, dis, out=None):
    """out[i] = dis[i] * (sum over i's in-edges from j != i of dis[j] x[j] + dis[i] x[i]): D^-1/2 (A + I) D^-1/2 x as torch_geometric's
    GCNConv normalises it (the input's self loops replaced by one unit loop per node).  x: [N, C] with contiguous rows (any row stride).
    The adjoint w.r.t. x is the same call on the plan of the flipped edge list with the same dis."""
    require_cuda(x, dis)
    ldx = _row_block(x, "gcn_pyg_propagate: x")
    N, Cc = x.shape
    if plan.N != N or dis.numel() != N or dis.dtype != torch.float32 or not dis.is_contiguous():
        raise ValueError(f"gcn_pyg_propagate: x has {N} rows, the plan {plan.N} nodes and dis {dis.numel()} entries")
    if out is None:
        out = torch.empty(N, Cc, dtype=torch.float32, device=x.device)
    elif out.shape != x.shape:
        raise ValueError("gcn_pyg_propagate: out must be an [N, C] block")
    ldo = _row_block(out, "gcn_pyg_propagate: out")
    if N == 0:
        return out
    with _span("sn_gcn_pyg_propagate_f32"):
        check(lib().sn_gcn_pyg_propagate_f32(ptr(x), ldx, N, Cc, plan.E, ptr(plan.rowptr), ptr(plan.col), ptr(dis), ptr(out), ldo, stream()),
              "sn_gcn_pyg_propagate_f32")
    return out


# ----------------------------------------------------------------------------- train-mode dropout (csrc/dropout.hip)
class DropoutState:
    """{seed, step} of the counter-based dropout masks: an int64 [2] DEVICE tensor the kernel reads when it runs, so a replay of a
    captured graph draws the current step's masks.  seed None takes torch.initial_seed() (reproducible under torch.manual_seed).
    Not a module buffer: it never enters a state_dict."""

    def __init__(self, seed=None, device="cuda", step=0):
        self.t = torch.zeros(2, dtype=torch.int64, device=device)
        self.set(torch.initial_seed() if seed is None else seed, step)

    def set(self, seed, step=0):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        host = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed, int(step)], dtype=torch.int64)
        self.t.copy_(host)
        return self

    def advance(self):
        """step += 1 on the device (a torch op: recordable in a captured graph)."""
        self.t[1:].add_(1)
        return self

    def snapshot(self):
        """A device clone: what one forward hands to all its sites and to its backward."""
        return self.t.clone()


def dropout_threshold(p):
    """(threshold, scale) of sn_dropout_f32 for 0 <= p < 1: floor(p * 2^32) in double precision, float32(1 / (1 - p))."""
    return int(math.floor(float(p) * 4294967296.0)), struct.unpack("f", struct.pack("f", 1.0 / (1.0 - float(p))))[0]


def _dropout_launch(x, ldx, R, Cc, p, snap, site, base, residual, ldr, out, ldo):
    thr, scale = dropout_threshold(p)
    with _span("sn_dropout_f32"):
        check(lib().sn_dropout_f32(ptr(x), ldx, R, Cc, thr, scale, ptr(snap), int(site), int(base), ptr(residual), ldr, ptr(out), ldo,
                                   stream()), "sn_dropout_f32")


def dropout(x, p, snap, site, residual=None, base=0):
    """Train-mode dropout of the logical row-major [R, C] tensor x (C = the last dimension): y = keep * x / (1 - p) + residual, the
    keep mask drawn by Philox4x32-10 from (snap = {seed, step}, site, base + r*C + c) — see signnet_hip.h.  The backward is the same
    call on dy.  p == 0: x itself, no launch (x + residual through `pointwise`); p == 1: zeros + residual."""
    p = float(p)
    if p < 0.0 or p > 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    if p == 0.0:
        return x if residual is None else pointwise(x, residual=residual)
    require_cuda(x, residual)
    if residual is not None and residual.shape != x.shape:
        raise ValueError("dropout: the residual must have x's shape")
    if p == 1.0:
        return torch.zeros_like(x) if residual is None else residual.clone()
    require_cuda(snap)
    if snap.dtype != torch.int64 or snap.numel() != 2 or not snap.is_contiguous():
        raise ValueError("dropout: snap must be the int64 [2] {seed, step} tensor of a DropoutState")
    x = _f32c(x, "x")
    residual = None if residual is None else _f32c(residual, "residual")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    Cc = x.shape[-1]
    _dropout_launch(x, Cc, x.numel() // Cc, Cc, p, snap, site, base, residual, Cc, out, Cc)
    return out


SIGNINV_DROP_SITE = 0x53490000   # + ordinal of the dropout call within one forward of a sign-invariant encoder (signnet_hip.h)


def affine_dropout(x, scale, shift, p, snap, site, nvalid=None, K=0, base=0):
    """BatchNorm apply and train-mode dropout of the row matrix x [..., C] in ONE launch (sn_affine_dropout_f32):
    y = rowvalid && keep ? fma(x, scale, shift) / (1 - p) : 0 — bit for bit `dropout(masked_affine(x, nvalid, K, scale=, shift=), p,
    snap, site)`.  scale = shift = None: dropout with a row mask.  p == 0: masked_affine itself, no new launch; p == 1: zeros."""
    p = float(p)
    if p < 0.0 or p > 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    if (scale is None) != (shift is None):
        raise ValueError("affine_dropout: scale and shift go together")
    if p == 0.0:
        return masked_affine(x, nvalid, K, scale=scale, shift=shift)
    require_cuda(x)
    if p == 1.0:
        return torch.zeros_like(x, dtype=torch.float32)
    require_cuda(snap)
    if snap.dtype != torch.int64 or snap.numel() != 2 or not snap.is_contiguous():
        raise ValueError("affine_dropout: snap must be the int64 [2] {seed, step} tensor of a DropoutState")
    x = _f32c(x, "x")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    Cc = x.shape[-1]
    if scale is not None and (scale.numel() != Cc or shift.numel() != Cc):
        raise ValueError(f"affine_dropout: scale / shift must have {Cc} elements")
    thr, ps = dropout_threshold(p)
    with _span("sn_affine_dropout_f32"):
        check(lib().sn_affine_dropout_f32(ptr(x), Cc, x.numel() // Cc, Cc, ptr(nvalid), int(K), ptr(scale), ptr(shift), thr, ps, ptr(snap),
                                          int(site), int(base), ptr(out), Cc, stream()), "sn_affine_dropout_f32")
    return out


class DropoutHolder:
    """Mixin of the models with feature dropout: a lazily created DropoutState kept OUT of the module's buffers (plain attribute: no
    state_dict key, not in model.buffers()).  A train-mode forward calls `_dropout_begin` once at its start: the step advances, and
    the snapshot it returns serves every site of that forward and its backward."""

    def seed_dropout(self, seed, step=0):
        """Masks of the next train-mode forward: those of (seed, step + 1); reproducible from here on."""
        self.__dict__["_sn_dropout_seed"] = (int(seed), int(step))
        st = self.__dict__.get("_sn_dropout_state")
        if st is not None:
            st.set(seed, step)
        return self

    def dropout_state(self, device):
        st = self.__dict__.get("_sn_dropout_state")
        if st is None or st.t.device != torch.device(device):
            seed, step = self.__dict__.get("_sn_dropout_seed", (None, 0))
            if st is not None:                              # the model moved: the state follows with its words
                seed, step = (int(v) for v in st.t.tolist())
            st = self.__dict__["_sn_dropout_state"] = DropoutState(seed, device, step)
        return st

    def _dropout_begin(self, device):
        return self.dropout_state(device).advance().snapshot()

    def _dropout_active(self):
        """Whether a train-mode forward of this model draws masks at all."""
        return any(float(getattr(m, n, 0.0) or 0.0) > 0.0 for m in [self] + list(getattr(self, "layers", []))
                   for n in ("dropout", "p_in_feat", "p_drop"))


def check_dropout_p(p, who):
    p = float(p)
    if p < 0.0 or p > 1.0:
        raise ValueError(f"{who}: dropout probability has to be between 0 and 1, but got {p}")
    return p


# ----------------------------------------------------------------------------- tanh / ELU of the sign-invariant encoders (csrc/activation.hip)
ACT_TANH, ACT_ELU = 1, 2                       # SN_ACT_* of signnet_hip.h
ACTIVATIONS = {"tanh": ACT_TANH, "elu": ACT_ELU}


def _act_code(act, who):
    if act not in ACTIVATIONS:
        raise ValueError(f"{who}: activation must be one of {sorted(ACTIVATIONS)}, got {act!r} (relu is the epilogue of masked_linear)")
    return ACTIVATIONS[act]


def act_affine(x, act, nvalid=None, K=0, scale=None, shift=None):
    """y = rowvalid ? fma(act(x), scale, shift) : 0 on the row matrix x [..., C] in ONE launch (sn_act_affine_f32): act 'tanh' | 'elu'
    (alpha 1), then the folded BatchNorm that follows the activation in the reference's MLP (mlp.py:40-51).  scale = shift = None:
    y = act(x) on valid rows."""
    code = _act_code(act, "act_affine")
    if (scale is None) != (shift is None):
        raise ValueError("act_affine: scale and shift go together")
    require_cuda(x)
    x = _f32c(x, "x")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    Cc = x.shape[-1]
    if scale is not None and (scale.numel() != Cc or shift.numel() != Cc):
        raise ValueError(f"act_affine: scale / shift must have {Cc} elements")
    with _span("sn_act_affine_f32"):
        check(lib().sn_act_affine_f32(ptr(x), Cc, x.numel() // Cc, Cc, ptr(nvalid), int(K), code, ptr(scale), ptr(shift), ptr(out), Cc,
                                      stream()), "sn_act_affine_f32")
    return out


def act_bwd(dy, a, act, nvalid=None, K=0):
    """dx = rowvalid ? dy * act'(a) : 0 with a = act(x), the saved output of act_affine WITHOUT an affine (sn_act_affine_bwd_f32)."""
    code = _act_code(act, "act_bwd")
    require_cuda(dy, a)
    dy, a = _f32c(dy, "dy"), _f32c(a, "a")
    if dy.shape != a.shape:
        raise ValueError("act_bwd: dy and a must have the same shape")
    dx = torch.empty_like(a)
    if a.numel() == 0:
        return dx
    Cc = a.shape[-1]
    with _span("sn_act_affine_bwd_f32"):
        check(lib().sn_act_affine_bwd_f32(ptr(dy), Cc, ptr(a), Cc, a.numel() // Cc, Cc, ptr(nvalid), int(K), code, ptr(dx), Cc, stream()),
              "sn_act_affine_bwd_f32")
    return dx
