"""A training step of fixed shape captured ONCE as a HIP graph and replayed (MI355X: HIP graphs instead of a tracing compiler).

The differentiable forward of `SignNetGNN` + loss + backward is ~350 kernel launches whose order and shapes depend only on the batch
SHAPE (nodes, edges, graphs, eigenvector entries): the kernels read graph sizes, CSR offsets and validity from device memory.  For a
fixed shape — the bench's synthetic batch, a padded / bucketed loader — the step is recorded once (`torch.cuda.graph` over the same
ctypes launches: the C ABI takes the capture stream) and replayed with ONE graph launch + the single Adam launch of
`optim.FlatAdam` (its bias correction depends on the step count, so it stays outside, as in learning_filters.GraphedEpoch).  Same
kernels, same order, same arithmetic as the eager step: bit-identical losses (tests/test_training_gpu.py).

Before constructing a GraphedStep drop every reference to the results of earlier EAGER steps of the same model (`del loss`): a live
loss keeps that step's autograd graph, and with it AccumulateGrad nodes bound to the default stream; the captured backward would then
have to synchronise with the default stream, which a capturing stream must not do.

What the reference does per step (Alchemy/main_alchemy.py:99-110, GINESignNetPyG/core/train.py:55-66): optimizer.zero_grad(),
model(data), L1 loss, loss.backward(), optimizer.step().
"""
from __future__ import annotations

import collections
import contextlib

import torch

_FIELDS = ("x", "edge_index", "edge_attr", "batch", "eigen_values", "eigen_vectors")


def l1_loss(y, target):
    return (y - target).abs().mean()


class GraphedStep:
    def __init__(self, model, optimizer, data, target, loss_fn=l1_loss, warmup=2):
        from .optim import FlatAdam
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("GraphedStep needs optim.FlatAdam (static flat parameter / gradient buffers)")
        if optimizer.dist is not None:
            # data parallel: the captured forward + backward is replayed per rank, then optimizer.step() all-reduces the flat gradient
            # (every bucket, after the replay — the hooks that issue buckets from inside an eager backward cannot run in a capture) and
            # launches Adam.  3.4 ms + one 27.6 MB all-reduce per step against the eager step's ~4.4 ms of host time.
            optimizer.disable_overlap()
        if not getattr(model, "max_k", None):
            raise ValueError("GraphedStep: the number of eigenvector slots must be fixed (max_k): the all-eigenvector mode sizes tensors from the batch")
        from . import train_stage
        train_stage.flush_deferred()          # (nothing of an earlier eager backward may be left for the captured one to reduce)
        self.model, self.optimizer, self.loss_fn = model, optimizer, loss_fn
        self.data, self.target = data, target
        self.shapes = {f: tuple(getattr(data, f).shape) for f in _FIELDS}
        model.train()
        # the attention dropout (transformer_module.py:46,55; the one dropout the reference leaves active) is random per step: its masks
        # are drawn OUTSIDE the graph with torch's device generator — the same draws in the same order as the eager step — into static
        # buffers the captured kernels read.  With model.attn_dropout_source == "counter" there is nothing to draw: (None, None), the
        # attention kernels evaluate the masks from the {seed, step} words whose advance is recorded inside the step
        self._draw, self._masks = _mask_buffers(model, int(data.batch.numel()), int(model.max_k), data.batch.device)
        self._status = None

        def fwd_bwd():
            optimizer.flat_g.zero_()
            y = model(self.data)
            loss = loss_fn(y, self.target)
            loss.backward()
            return loss, y

        self.graph, self.loss, self.y, self._status = _capture(self, fwd_bwd, data.batch.device, warmup)

    @contextlib.contextmanager
    def _scoped(self):
        """The two switches the captured step needs on the MODEL — no host read of the status words inside the forward, attention
        dropout masks read from this object's static buffers — are set only while this object runs the model (warm-up and capture;
        a replay does not call the model at all) and restored afterwards: an eager train-mode forward of the same model (a ragged last
        batch, a second loop) draws fresh masks and checks its embedding indices as if no GraphedStep existed."""
        m = self.model
        saved = (getattr(m, "_defer_status", False), getattr(m, "_attn_masks", None))
        m._defer_status, m._attn_masks = True, self._masks
        try:
            yield
        finally:
            m._defer_status, m._attn_masks = saved

    def check(self):
        """Reads the status words of the LAST replayed step (one host wait): raises IndexError for a discrete feature outside its
        embedding table, as nn.Embedding does in the reference's eager step.  step() calls it every `check_every` steps."""
        if self._status is not None and int(self._status[5]):
            from . import ops
            raise IndexError(ops.EMBEDDING_INDEX_ERROR)

    def _refresh_masks(self):
        if self._masks is not None:
            for dst, src in zip(self._masks, self._draw()):
                dst.copy_(src)

    def load(self, data=None, target=None):
        """Copy a new batch of the SAME shape into the static input buffers."""
        if data is not None:
            for f in _FIELDS:
                src, dst = getattr(data, f), getattr(self.data, f)
                if tuple(src.shape) != self.shapes[f]:
                    raise ValueError(f"GraphedStep: {f} has shape {tuple(src.shape)}, the captured step {self.shapes[f]}")
                dst.copy_(src, non_blocking=True)
            if int(data.num_graphs) != int(self.data.num_graphs):
                raise ValueError("GraphedStep: number of graphs differs from the captured step")
        if target is not None:
            self.target.copy_(target, non_blocking=True)

    check_every = 64     # replays between two reads of the status words (0 = only when the caller calls check())

    def step(self, data=None, target=None):
        self.load(data, target)
        self._refresh_masks()
        self.graph.replay()
        self.optimizer.step()
        self._nsteps = getattr(self, "_nsteps", 0) + 1
        if self.check_every and self._nsteps % self.check_every == 0:
            self.check()
        return self.loss


def _mask_buffers(model, N, K, dev):
    """(draw, static buffers) of the attention-dropout masks [N, H, K, K] per rho layer, or (None, None) without dropout — and with
    the counter source (model.attn_dropout_source == "counter"): the attention kernels evaluate the masks themselves from the model's
    {seed, step} words, whose advance and snapshot are recorded inside the captured step, so nothing is drawn, kept or copied here."""
    if not getattr(model, "attn_dropout", 0.0) or getattr(model, "attn_dropout_source", "generator") == "counter":
        return None, None
    from . import ops
    from .pyg import N_HEAD
    draw = lambda: [ops.attention_dropout_mask(N, K, N_HEAD, model.attn_dropout, dev) for _ in model.sign_net.rho.transformer_layers]
    st0 = torch.cuda.get_rng_state(dev)
    masks = [torch.empty_like(m) for m in draw()]
    torch.cuda.set_rng_state(st0, dev)       # (the sizing draw does not count)
    return draw, masks


def _capture(step, fwd_bwd, dev, warmup, check=None):
    """Warm up `fwd_bwd` on a side stream (lazy one-time setup: LDS limits, allocator pools) and capture it, under `step._scoped()`,
    without touching the model's state: buffers (running statistics, counters), the generator and the step word of the model's feature
    dropout (ops.DropoutHolder: its advance and snapshot are recorded inside `fwd_bwd`, so every replay draws the next step's masks) are
    restored afterwards — the step word of the `sign_inv_net`'s own state included.
    `check`: what raises for a bad batch after the warm-up (default: the model's check_train()).
    -> (graph, loss, y, the captured forward's status words)."""
    model = step.model
    saved = [b.detach().clone() for b in model.buffers()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rng = torch.cuda.get_rng_state(dev) if step._masks is not None else None
    # (the state exists before the capture: its creation copies from the host)
    # (likewise the state of a sign-invariant encoder with dropout of its own: dropout_signinv.py)
    holders = [m for m in (model, getattr(model, "sign_inv_net", None)) if getattr(m, "_dropout_active", lambda: False)()]
    drops = [m.dropout_state(dev) for m in holders]
    drops_saved = [d.t.clone() for d in drops]
    with step._scoped():
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step._refresh_masks()
                fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        (check or model.check_train)()
        graph = torch.cuda.CUDAGraph()
        # With a process group up, its watchdog THREAD polls the events of earlier collectives (WorkNCCL::isCompleted) whenever it wakes.
        # A capture in the default "global" error mode forbids an event query from every thread of the process: a poll that lands inside
        # the capture invalidates it and the watchdog's exception ends the process.  "thread_local" holds this thread to the same rules
        # and leaves the other thread alone; without a process group the mode stays as it was.
        import torch.distributed as D
        mode = "thread_local" if (D.is_available() and D.is_initialized()) else "global"
        with torch.cuda.graph(graph, capture_error_mode=mode):
            loss, y = fwd_bwd()
        # the captured forward's status words (static memory of the graph): every replay rewrites them, check() reads them
        status, model._train_status = getattr(model, "_train_status", None), None
    with torch.no_grad():
        for b, sv in zip(model.buffers(), saved):
            b.copy_(sv)
    if rng is not None:
        torch.cuda.set_rng_state(rng, dev)      # the warm-up's draws do not count: the first step draws what an eager one would
    for d, sv in zip(drops, drops_saved):
        d.t.copy_(sv)                           # nor do its dropout steps
    return graph, loss.detach(), y.detach(), status


# ----------------------------------------------------------------------------- variable-shape batches: one capture per capacity bucket
class Bucket(tuple):
    """The capacities of a padded batch: N_cap > N nodes (the spare graph holds >= 1 padding node), E_cap >= E edges, S_cap >= S
    eigenvector entries, K_cap eigenvector slots per node (max_k, or >= the largest graph in the all-eigenvector mode)."""
    __slots__ = ()
    _names = ("N", "E", "S", "K")

    def __new__(cls, N, E, S, K):
        return tuple.__new__(cls, (int(N), int(E), int(S), int(K)))

    N = property(lambda s: s[0])
    E = property(lambda s: s[1])
    S = property(lambda s: s[2])
    K = property(lambda s: s[3])

    def __repr__(self):
        return "Bucket(N=%d, E=%d, S=%d, K=%d)" % self


def _round_up(v, g):
    g = max(int(g), 1)
    return -(-int(v) // g) * g


class PaddedBatch:
    """The static buffers of one bucket: the padded batch the captured step reads (the PyG field names, `num_graphs` = B_cap), the
    padded target, the 0/1 validity vectors and the device count block [N, E, B, S] (ops.bucket_pack writes all of them)."""

    def __init__(self, bucket, B_cap, data, target, dev):
        self.N_cap, self.E_cap, self.S_cap, self.K = bucket.N, bucket.E, bucket.S, bucket.K
        self.B_cap = int(B_cap)
        z = lambda n, like: torch.zeros((n,) + tuple(like.shape[1:]), dtype=like.dtype, device=dev)
        self.x = z(self.N_cap, data.x)
        self.edge_index = torch.zeros(2, self.E_cap, dtype=torch.int64, device=dev)
        self.edge_attr = z(self.E_cap, data.edge_attr)
        self.batch = torch.zeros(self.N_cap, dtype=torch.int64, device=dev)
        self.eigen_values = torch.zeros(self.N_cap, dtype=torch.float32, device=dev)
        self.eigen_vectors = torch.zeros(self.S_cap, dtype=torch.float32, device=dev)
        self.target = torch.zeros(self.B_cap, target.numel() // max(int(data.num_graphs), 1), dtype=torch.float32, device=dev)
        self.node_valid = torch.zeros(self.N_cap, dtype=torch.int32, device=dev)
        self.edge_valid = torch.zeros(self.E_cap, dtype=torch.int32, device=dev)
        self.graph_valid = torch.zeros(self.B_cap, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int32, device=dev)
        self.num_graphs, self.num_nodes = self.B_cap, self.N_cap


class _BucketCapture:
    """One bucket's captured forward + masked L1 + backward (the machinery of GraphedStep: warm-up on a side stream, buffers and
    generator restored, the switches scoped to the capture) and its own memory pool."""

    def __init__(self, owner, bucket, data, target, warmup, fill=None):
        """`fill(pad)`: the call that fills the capacity buffers (default: ops.bucket_pack of `data` / `target`; a store's gather_into
        for step_from — `data` / `target` then only give the dtypes and row shapes)."""
        model, optimizer = owner.model, owner.optimizer
        dev = data.batch.device
        self.model, self.bucket = model, bucket
        r0 = torch.cuda.memory_reserved(dev)
        self.pad = PaddedBatch(bucket, owner.B_cap, data, target, dev)
        if fill is None:
            from . import ops
            ops.bucket_pack(data, target, self.pad)
        else:
            fill(self.pad)
        self._draw, self._masks = _mask_buffers(model, bucket.N, bucket.K, dev)
        self._status = None
        from .autograd import masked_l1_loss
        pad = self.pad

        def fwd_bwd():
            optimizer.flat_g.zero_()
            y = model(pad)
            loss = masked_l1_loss(y, pad.target.view_as(y), pad.graph_valid, pad.counts[2:3])
            loss.backward()
            return loss, y

        self.graph, self.loss, self.y, self._status = _capture(self, fwd_bwd, dev, warmup)
        self.memory_reserved = torch.cuda.memory_reserved(dev) - r0

    @contextlib.contextmanager
    def _scoped(self):
        m = self.model
        saved = (getattr(m, "_defer_status", False), getattr(m, "_attn_masks", None), getattr(m, "_bucket", None))
        m._defer_status, m._attn_masks, m._bucket = True, self._masks, self.pad
        try:
            yield
        finally:
            m._defer_status, m._attn_masks, m._bucket = saved

    _refresh_masks = GraphedStep._refresh_masks
    check = GraphedStep.check


class _CaptureLRU:
    """What BucketedStep and DGLBucketedStep share: the LRU of `max_captures` captured buckets (each with its own memory pool), the
    `captures` / `hits` counters, the replay (one graph launch + the one Adam launch of optim.FlatAdam) and check()."""

    check_every = 64     # replays between two reads of the status words (0 = only when the caller calls check())

    def _init_lru(self, max_captures):
        self.max_captures = int(max_captures)
        self._lru = collections.OrderedDict()       # bucket -> capture, least recently used first
        self.captures = self.hits = 0
        self._last, self._nsteps = None, 0
        self._from_store = False                    # the last step's batch came through a store's gather (step_from)

    @property
    def buckets(self):
        """The buckets captured now, least recently used first."""
        return list(self._lru)

    def _admit(self, bucket):
        """LRU bookkeeping for a bucket about to be used: True if it is captured already."""
        if bucket in self._lru:
            self._lru.move_to_end(bucket)
            return True
        while len(self._lru) >= self.max_captures:
            _, old = self._lru.popitem(last=False)
            if self._last is old:
                self._last = None
            old.graph.reset()           # (its private memory pool goes back to the allocator)
        return False

    def release(self):
        """Drop every capture (their memory pools go back to the allocator); the next step of any bucket captures again."""
        while self._lru:
            _, old = self._lru.popitem(last=False)
            old.graph.reset()
        self._last = None

    def _replay(self, cap):
        self._last = cap
        cap._refresh_masks()
        cap.graph.replay()
        self.optimizer.step()
        self._nsteps += 1
        if self.check_every and self._nsteps % self.check_every == 0:
            self.check()
        return cap.loss

    def check(self):
        """Reads the status words of the LAST replayed step (one host wait): raises IndexError for a discrete feature outside its
        embedding table, as nn.Embedding does in the reference's eager step (and, for a DGL GATNet, the eager step's batch errors).
        After step_from also the gather's status block: IndexError for a graph index outside the store."""
        if self._last is not None:
            if self._from_store:
                from . import ops
                flags = int(self._last.pad.gather_status[0])
                if flags & ops.GATHER_BAD_INDEX:
                    raise IndexError(ops.STORE_INDEX_ERROR)
                if flags & ops.GATHER_MISMATCH:
                    raise ValueError(ops.STORE_TOTALS_ERROR)
            self._last.check()

    def _step_from(self, store, idx, bucket, bucket_type, capture):
        """step_from of both step classes: the bucket from the store's host sizes, the batch through store.gather_into, then the LRU,
        capture and replay of step()."""
        from .data import _resolve
        idx = _resolve(idx, store.device)
        B = int(idx[0].size)
        if B > self.max_graphs:
            raise ValueError(f"{type(self).__name__}: a batch of {B} graphs exceeds max_graphs={self.max_graphs}")
        totals = store.totals(idx[0])
        b = store.bucket_of(idx[0], self.granule, getattr(self.model, "max_k", None), _totals=totals) if bucket is None \
            else bucket_type(*bucket)
        fill = lambda pad: store.gather_into(idx, pad, _totals=totals)
        if self._admit(b):
            cap = self._lru[b]
            fill(cap.pad)
            self.hits += 1
        else:
            from . import train_stage
            train_stage.flush_deferred()      # (nothing of an earlier eager backward may be left for the captured one to reduce)
            self.model.train()
            cap = capture(b, fill)
            self._lru[b] = cap
            self.captures += 1
        self._from_store = True
        return self._replay(cap)


_PLAIN_MODELS = "pyg.GNN (variant='gine'), pyg_gnn_types.GNN (any gnn_type), dropout_models.GNN, pyg_baselines.NetGINE"


def _admit_model(model):
    """Which models BucketedStep takes, by class: pyg.SignNetGNN -> False; the baseline models (_PLAIN_MODELS) -> True; anything else
    TypeError.  (The check used to be `model.variant in ("gine", "alchemy")`, which also let pyg.GNN and pyg_gnn_types.GNN through at a
    time when their forwards ignored the padded batch: padding rows entered every BatchNorm statistic.)"""
    from . import pyg, pyg_baselines
    if isinstance(model, pyg.SignNetGNN):
        return False
    if isinstance(model, pyg_baselines.NetGINE):
        return True
    if isinstance(model, pyg.GNN):                  # (pyg_gnn_types.GNN and dropout_models.GNN are subclasses)
        if model.variant != "gine":
            raise TypeError(f"BucketedStep: a pyg.GNN with variant={model.variant!r} is no model of its own (its forward is refused); "
                            f"needs a pyg.SignNetGNN or one of {_PLAIN_MODELS}")
        return True
    raise TypeError(f"BucketedStep needs a pyg.SignNetGNN or one of the baseline models: {_PLAIN_MODELS} (got {type(model).__name__})")


class BucketedStep(_CaptureLRU):
    """The captured training step for a real loader: batches of any shape (node count N, edge count E, eigenvector entries S, at most
    `max_graphs` graphs; max_k fixed or None = all eigenvectors) are padded into fixed-capacity buffers and run through a step captured
    ONCE per capacity bucket (the reference's loops: Alchemy/main_alchemy.py:99-110, GINESignNetPyG/core/train.py:55-66).

        step = BucketedStep(model, flat_adam, max_graphs=128, granule=dict(N=64, E=128, S=4096, K=8), max_captures=4)
        loss = step.step(data, target)

    step(): the bucket is chosen on the HOST from tensor shapes (each capacity rounded up to its granule; N_cap >= N + 1, B_cap =
    max_graphs + 1: the spare graph holds the padding nodes); a new bucket is captured on first use (`captures`), a known one replayed
    (`hits`); the captures live in an LRU of `max_captures`, each with its own memory pool.  A step is then ONE pack launch
    (sn_bucket_pack: batch + target + padding + validity + count block), one graph replay and the one Adam launch of optim.FlatAdam.
    Padding rows enter no batch statistic, no running statistic and no gradient: the losses and gradients are those of the eager step
    on the unpadded batch (up to summation order), and the padding content cannot change a bit of them.

    All-eigenvector mode (max_k=None): K_cap comes from the largest graph — from host bookkeeping when the batch carries it
    (pyg.host_max_nodes: data.sizes, PyG's _slice_dict / a CPU ptr); otherwise ONE device read of the largest graph size per step, as
    the reference itself does (`int(num_nodes.max())`, GINESignNetPyG/core/transform.py:29-38).

    Models: pyg.SignNetGNN, and the baselines of the two PyG trees — pyg.GNN (variant='gine'), pyg_gnn_types.GNN for every gnn_type,
    dropout_models.GNN and pyg_baselines.NetGINE (target [B, 12]).  The baselines read no eigen data: a batch may come without
    eigen_vectors / eigen_values (packed as S = 0), bucket_of returns S = K = 1 so only N and E pick a capture, and a GraphStore's
    eigen data is gathered and ignored.

    Loss: the reference's L1 (mean |y - target| over the batch's graphs), divided by the device graph count.  Data parallel training is
    not supported (optimizer.dist must be None)."""

    check_every = 64     # replays between two reads of the status words (0 = only when the caller calls check())

    def __init__(self, model, optimizer, loss="l1", max_graphs=128, granule=None, max_captures=4, warmup=2):
        from .optim import FlatAdam
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("BucketedStep needs optim.FlatAdam (static flat parameter / gradient buffers)")
        if optimizer.dist is not None:
            raise ValueError("BucketedStep: data-parallel training (FlatAdam with dist) is not supported; use GraphedStep or the eager step")
        if loss != "l1":
            raise ValueError(f"BucketedStep: loss {loss!r} is not supported (only 'l1', the reference's loss)")
        if int(max_graphs) < 1 or int(max_captures) < 1:
            raise ValueError("BucketedStep: max_graphs and max_captures must be >= 1")
        self.plain = _admit_model(model)            # a baseline model: reads no eigen data, so S and K never pick a capture
        self.model, self.optimizer = model, optimizer
        self.max_graphs, self.B_cap = int(max_graphs), int(max_graphs) + 1
        self.granule = dict(N=64, E=128, S=4096, K=8)
        for k, v in (granule or {}).items():
            if k not in self.granule or int(v) < 1:
                raise ValueError(f"BucketedStep: granule {k}={v} (keys N, E, S, K; values >= 1)")
            self.granule[k] = int(v)
        self.warmup = int(warmup)
        self._init_lru(max_captures)                # Bucket -> _BucketCapture

    def bucket_of(self, data):
        """The capacity bucket of a batch (host only, unless max_k is None and the batch has no host-side sizes: one device read)."""
        B = int(data.num_graphs)
        if B > self.max_graphs:
            raise ValueError(f"BucketedStep: a batch of {B} graphs exceeds max_graphs={self.max_graphs}")
        N = int(data.batch.numel())
        E = int(data.edge_index.shape[1]) if data.edge_index.numel() else 0
        g = self.granule
        if self.plain:          # the smallest legal S and K: only N and E decide which capture a batch gets (eigen fields may be absent)
            return Bucket(_round_up(N + 1, g["N"]), _round_up(max(E, 1), g["E"]), 1, 1)
        S = int(data.eigen_vectors.numel())
        mk = getattr(self.model, "max_k", None)
        if mk:
            K = int(mk)
        else:
            from .pyg import host_max_nodes
            nmax = host_max_nodes(data)
            if nmax is None:       # (the one allowed device read: the reference's int(num_nodes.max()))
                nmax = int(torch.bincount(data.batch).max()) if N else 1
            K = _round_up(max(nmax, 1), g["K"])
        return Bucket(_round_up(N + 1, g["N"]), _round_up(max(E, 1), g["E"]), _round_up(max(S, 1), g["S"]), K)

    def step(self, data, target, bucket=None):
        """One training step on `data` / `target` ([num_graphs, n_out]): returns the loss (a device scalar, rewritten by the next
        step of the same bucket).  `bucket`: explicit capacities (Bucket / (N, E, S, K)) instead of the granule rounding."""
        b = self.bucket_of(data) if bucket is None else Bucket(*bucket)
        if bucket is not None and int(data.num_graphs) > self.max_graphs:
            raise ValueError(f"BucketedStep: a batch of {int(data.num_graphs)} graphs exceeds max_graphs={self.max_graphs}")
        if self.plain and getattr(data, "eigen_vectors", None) is not None:
            # a baseline model reads no eigen data: a batch that carries some is packed without it (S = 0), so S_cap = 1 holds it
            import types
            data = types.SimpleNamespace(x=data.x, edge_index=data.edge_index, edge_attr=data.edge_attr, batch=data.batch,
                                         num_graphs=data.num_graphs)
        if self._admit(b):
            cap = self._lru[b]
            from . import ops
            ops.bucket_pack(data, target, cap.pad)
            self.hits += 1
        else:
            from . import train_stage
            train_stage.flush_deferred()      # (nothing of an earlier eager backward may be left for the captured one to reduce)
            self.model.train()
            cap = _BucketCapture(self, b, data, target, self.warmup)
            self._lru[b] = cap
            self.captures += 1
        self._from_store = False
        return self._replay(cap)

    def step_from(self, store, idx, bucket=None):
        """step() on the graphs `idx` of a data.GraphStore: host indices, or the (host indices, device view) pair an IndexLoader
        yields — then nothing is copied to the device.  The batch reaches the capacity buffers through store.gather_into (ONE
        sn_store_gather launch in place of the pack launch); same LRU, capture, replay and check().  `bucket`: explicit capacities,
        e.g. store.covering_bucket(...) — one capture for a whole run."""
        if getattr(store, "dgl", True):
            raise TypeError("BucketedStep.step_from needs a data.GraphStore")
        if self.plain and bucket is None:
            # a store's batch carries eigen data: gathered and ignored (as the DGL store's pos_enc is for 'no_pe'), so S_cap holds it;
            # K = 1, the smallest legal value
            from .data import _resolve
            bucket = store.bucket_of(_resolve(idx, store.device)[0], self.granule, 1)
        return self._step_from(store, idx, bucket, Bucket,
                               lambda b, fill: _BucketCapture(self, b, *store.proto(), self.warmup, fill=fill))


# ----------------------------------------------------------------------------- the DGL tree's loop (GraphPrediction)
_DGL_NETS = ("GINNet", "GatedGCNNet", "GATNet", "PNANet", "TransformerNet")


class DGLBucket(tuple):
    """The capacities of a padded DGL batch: N_cap > N nodes (the spare graph holds >= 1 padding node), E_cap >= E edges."""
    __slots__ = ()

    def __new__(cls, N, E):
        return tuple.__new__(cls, (int(N), int(E)))

    N = property(lambda s: s[0])
    E = property(lambda s: s[1])

    def __repr__(self):
        return "DGLBucket(N=%d, E=%d)" % self


class DGLPaddedBatch:
    """The static buffers of one DGL bucket (ops.bucket_pack_dgl writes all of them): edge list, atom / bond ids, pos_enc, snorm_n and
    targets in capacity buffers, the padded per-graph node counts, the 0/1 node / edge / graph validity, the node-slot vector (K on valid
    nodes, 0 on padding nodes), the device count block [N, E, B] — and `g`, the padded graph object the nets read.  Its host-side node
    counts are frozen (total N_cap): the plans' node-count check reads no device value; the node -> graph vector is rebuilt on the device
    from the padded counts by the recorded repeat_interleave(..., output_size=N_cap) at every replay.  The pack guarantees that they
    total N_cap, also for a batch whose counts do not sum to its N rows (count_error: check() raises the eager step's ValueError)."""

    def __init__(self, bucket, B_cap, K, has_e, has_snorm, dev):
        from .dgl_deepsigns import Graph
        self.N_cap, self.E_cap, self.B_cap, self.K = bucket.N, bucket.E, int(B_cap), int(K)
        i64, i32, f32 = (dict(dtype=t, device=dev) for t in (torch.int64, torch.int32, torch.float32))
        self.src, self.dst = torch.zeros(self.E_cap, **i64), torch.zeros(self.E_cap, **i64)
        self.h = torch.zeros(self.N_cap, **i64)
        self.e = torch.zeros(self.E_cap, **i64) if has_e else None
        self.p = torch.zeros(self.N_cap, self.K, **f32)
        self.snorm_n = torch.zeros(self.N_cap, 1, **f32) if has_snorm else None
        self.target = torch.zeros(self.B_cap, 1, **f32)
        self.batch_num_nodes = torch.zeros(self.B_cap, **i64)
        self.node_valid, self.node_slots = torch.zeros(self.N_cap, **i32), torch.zeros(self.N_cap, **i32)
        self.edge_valid = torch.zeros(self.E_cap, **i32)
        self.graph_valid = torch.zeros(self.B_cap, **i32)
        self.counts = torch.zeros(3, **i32)
        self.count_error = torch.zeros(1, **i32)                 # 1: the batch's node counts did not sum to N (check() raises)
        self.g = Graph(self.src, self.dst, self.batch_num_nodes)
        self.g._sn_node_counts = (self.N_cap, self.N_cap)       # (largest graph: an upper bound; only eval paths read it)


_LAP_METHODS = ("sign_inv", "sign_flip", "abs_val", "canonical", "none")


class _DGLBucketCapture:
    """One DGL bucket's captured step — handle_lap -> net -> masked L1 over the valid graphs -> backward (the loop body of
    train_ZINC_graph_regression.py:60-82) — with the host checks of its forward deferred (ops.defer_status) and its own memory pool.
    handle_lap is the net's lap_method (sign_inv_net, or the one recorded sn_lap_pe_transform_f32 launch) for pe_init 'lap_pe' and
    nothing for 'no_pe'.  For 'sign_flip' the k uniforms live in the static buffer `u`, redrawn before every replay (`_refresh_masks`,
    as the attention-dropout masks of GraphedStep): on the host (the reference's torch.rand(k) sequence, uploaded through pinned memory)
    or on the device (owner.flip_rng)."""

    _masks = None
    u = None

    def _refresh_masks(self):
        if self.u is None:
            return
        if self.flip_rng == "device":
            self.u.copy_(torch.rand(self.u.numel(), device=self.u.device))
        else:
            self.u.copy_(torch.rand(self.u.numel()).pin_memory(), non_blocking=True)

    def __init__(self, owner, bucket, batch, warmup, fill=None):
        """`fill(pad)`: the call that fills the capacity buffers (default: ops.bucket_pack_dgl of `batch`; a store's gather_into for
        step_from — `batch` then only tells the device and which optional arrays exist)."""
        net, optimizer = owner.model, owner.optimizer
        g, h, p, e, snorm_n, targets = batch
        dev = h.device
        self.model, self.bucket = net, bucket
        r0 = torch.cuda.memory_reserved(dev)
        self.pad = pad = DGLPaddedBatch(bucket, owner.B_cap, owner.K, e is not None, snorm_n is not None, dev)
        from . import ops
        if fill is None:
            ops.bucket_pack_dgl(g, h, p, e, snorm_n, targets, pad)
        else:
            fill(pad)
        self._words = []
        from .autograd import masked_l1_loss
        from .dgl_nets import handle_lap
        method, self.flip_rng = owner.lap_method, owner.flip_rng
        if method == "sign_flip":
            self.u = torch.zeros(owner.K, dtype=torch.float32, device=dev)
            if self.flip_rng == "device":
                self._masks = [self.u]               # (_capture then restores the device generator: the warm-up's draws do not count)

        def fwd_bwd():
            optimizer.flat_g.zero_()
            # (the embedding index checks and GAT's batch checks hand their device words over instead of reading them: check() does)
            with ops.defer_status() as words:
                if method is None:
                    pe = None                                                                   # pe_init 'no_pe' (:73)
                else:
                    if method == "canonical":
                        pad.g._sn_plans = {}         # its batch plan (graph_ptr) is rebuilt inside the recorded step
                    pe = handle_lap(net, pad.p, pad.g, u=self.u)                                # (:13-51; sign_inv: :20-25)
                y, _ = net(pad.g, pad.h, pe, pad.e, pad.snorm_n)
            self._words = words
            loss = masked_l1_loss(y, pad.target.view_as(y), pad.graph_valid, pad.counts[2:3])
            loss.backward()
            return loss, y

        cpu_rng = torch.get_rng_state() if (self.u is not None and self.flip_rng == "host") else None
        self.graph, self.loss, self.y, _ = _capture(self, fwd_bwd, dev, warmup, check=self.check)
        if cpu_rng is not None:
            torch.set_rng_state(cpu_rng)             # the warm-up's draws do not count: the first step draws what an eager one would
        self.memory_reserved = torch.cuda.memory_reserved(dev) - r0

    @contextlib.contextmanager
    def _scoped(self):
        """The switch `_bucket` on the net AND its sign_inv_net, set only while this object runs them (warm-up and capture)."""
        mods = [self.model] + ([self.model.sign_inv_net] if getattr(self.model, "sign_inv_net", None) is not None else [])
        saved = [getattr(m, "_bucket", None) for m in mods]
        for m in mods:
            m._bucket = self.pad
        try:
            yield
        finally:
            for m, s in zip(mods, saved):
                m._bucket = s

    def check(self):
        """The deferred checks of the captured forward, read now (one host wait): what the eager step raises at once."""
        from . import ops
        if int(self.pad.count_error[0]):
            raise ValueError(ops.NODE_COUNT_ERROR)
        ops.raise_deferred(self._words)


_FULL_GRAPH_REFUSAL = "DGLBucketedStep does not carry the edge flag edata['real'] of a full_graph=True net through its pack launch"


def carries_real_flag(g):
    """Whether a graph object holds edata['real']: the complete graph of ops.make_full_graph (the edge form of a full-graph net)."""
    ed = getattr(g, "edata", None)
    try:
        return ed is not None and "real" in ed
    except TypeError:
        return False


class DGLBucketedStep(_CaptureLRU):
    """The captured training step of the DGL tree's loop (GraphPrediction/train/train_ZINC_graph_regression.py:54-88): batches of any
    shape (N nodes, E edges, at most `max_graphs` graphs) are padded into fixed-capacity buffers and run through a step captured ONCE
    per capacity bucket.

        step = DGLBucketedStep(net, flat_adam, max_graphs=128, granule=dict(N=256, E=512), max_captures=4)
        loss = step.step(g, h, p, e, snorm_n, targets)      # p: the raw pos_enc [N, pos_enc_dim]; e / snorm_n None where unused

    `net`: GINNet, GatedGCNNet, GATNet, PNANet or TransformerNet of dgl_nets (a full_graph=True TransformerNet in its bond form only —
    net.full_graph_input = "bonds": `g` is then the molecular graph, the spare graph of a bucket is skipped by the attention) — pe_init 'lap_pe' with lap_method 'sign_inv' (and its
    sign_inv_net: GINDeepSigns / MaskedGINDeepSigns), 'sign_flip', 'abs_val', 'canonical' or 'none', or pe_init 'no_pe' (p may then be
    None in step(); step_from takes a store of any pos_enc width, gathered and ignored).  `flip_rng` ('sign_flip'): "host" — the k
    uniforms of a step are torch.rand(k) of the CPU default generator, the reference's sequence — or "device" —
    torch.rand(k, device=...) outside the capture: nothing is copied from the host per step.  `g`: a DGL batched graph or dgl_deepsigns.Graph (only edges() and batch_num_nodes() are
    read).  step(): the bucket is chosen on the HOST from tensor shapes, with no device read (N_cap >= N + 1 and E_cap >= max(E, 1),
    each rounded up to its granule; B_cap = max_graphs + 1: the spare graph holds the padding nodes; K = net.pos_enc_dim); a new bucket
    is captured on first use (`captures`), a known one replayed (`hits`); the captures live in an LRU of `max_captures`, each with its
    own memory pool.  The captured region is handle_lap -> net -> the L1 loss over the valid graphs divided by the device graph count
    -> backward; a step is then ONE pack launch (sn_bucket_pack_dgl), one graph replay and the one Adam launch of optim.FlatAdam.
    Padding rows enter no batch statistic, no running statistic and no gradient: losses and gradients are those of the eager step on
    the unpadded batch (up to summation order), and the padding content cannot change a bit of them.  The forward's host checks (atom /
    bond ids outside their tables, GAT's malformed batch and zero-in-degree tests, node counts on the device that do not sum to N) are
    read by check(), every `check_every` steps, and raise what the eager step raises; host-side node counts that do not sum to N raise
    that ValueError before any launch.  Data-parallel training is not supported (optimizer.dist must be None)."""

    def __init__(self, net, optimizer, max_graphs=128, granule=None, max_captures=4, warmup=2, flip_rng="host"):
        from . import dgl_nets
        from .optim import FlatAdam
        # (a full-graph net in its bond form takes the molecular graph: an ordinary DGL batch.  The form is recorded: the captured
        #  launches are those of the form the net had here)
        self._full_form = getattr(net, "full_graph_input", "edges") if getattr(net, "full_graph", False) else None
        if self._full_form not in (None, "bonds"):
            raise NotImplementedError(_FULL_GRAPH_REFUSAL)
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("DGLBucketedStep needs optim.FlatAdam (static flat parameter / gradient buffers)")
        if not isinstance(net, tuple(getattr(dgl_nets, n) for n in _DGL_NETS)):
            raise TypeError("DGLBucketedStep needs a dgl_nets network (" + ", ".join(_DGL_NETS) + ")")
        if optimizer.dist is not None:
            raise ValueError("DGLBucketedStep: data-parallel training (FlatAdam with dist) is not supported; use the eager step")
        method, has_net = getattr(net, "lap_method", None), getattr(net, "sign_inv_net", None) is not None
        lap = getattr(net, "pe_init", None) == "lap_pe"          # (:73: handle_lap runs for pe_init 'lap_pe' only)
        if lap and method not in _LAP_METHODS:
            raise ValueError(f"DGLBucketedStep: lap_method {method!r} is not supported (one of {', '.join(_LAP_METHODS)})")
        # (a net is built with a sign_inv_net exactly when its lap_method is 'sign_inv': anything else was altered after construction)
        if method != "sign_inv" and has_net:
            raise ValueError(f"DGLBucketedStep: lap_method {method!r} on a net that carries a sign_inv_net (built for 'sign_inv')")
        if getattr(net, "use_lapeig_loss", False):
            raise ValueError("DGLBucketedStep: use_lapeig_loss is not supported (the L1 task loss only)")
        if method == "sign_inv" and not has_net:
            raise ValueError("DGLBucketedStep: lap_method 'sign_inv' but the net has no sign_inv_net")
        if flip_rng not in ("host", "device"):
            raise ValueError(f"DGLBucketedStep: flip_rng {flip_rng!r} (\"host\" or \"device\")")
        self.lap_method, self.flip_rng = (method if lap else None), flip_rng
        if int(max_graphs) < 1 or int(max_captures) < 1:
            raise ValueError("DGLBucketedStep: max_graphs and max_captures must be >= 1")
        self.model, self.optimizer = net, optimizer
        self.max_graphs, self.B_cap = int(max_graphs), int(max_graphs) + 1
        self.K = int(net.pos_enc_dim)
        self.granule = dict(N=256, E=512)
        for k, v in (granule or {}).items():
            if k not in self.granule or int(v) < 1:
                raise ValueError(f"DGLBucketedStep: granule {k}={v} (keys N, E; values >= 1)")
            self.granule[k] = int(v)
        self.warmup = int(warmup)
        self._init_lru(max_captures)                # DGLBucket -> _DGLBucketCapture

    def _zero_p(self, N, dev):
        """[N, K] zeros for a NoPE step without p (a view of one buffer kept here: no allocation, no launch per step)."""
        z = getattr(self, "_zeros", None)
        if z is None or z.shape[0] < N or z.shape[1] != self.K or z.device != dev:
            z = self._zeros = torch.zeros(max(N, self.granule["N"]), self.K, dtype=torch.float32, device=dev)
        return z[:N]

    def _check_form(self, g=None):
        """A full-graph net keeps the input form it was given to this object with, and its batches are molecular graphs."""
        if self._full_form is None:
            return
        now = getattr(self.model, "full_graph_input", "edges")
        if now != self._full_form:
            raise RuntimeError(f"DGLBucketedStep: the net's full_graph_input changed from {self._full_form!r} to {now!r} since this step was "
                               "built: build a new DGLBucketedStep")
        if g is not None and carries_real_flag(g):
            raise NotImplementedError(_FULL_GRAPH_REFUSAL)

    def _num_graphs(self, g):
        B = int(g.batch_num_nodes().numel())
        if B > self.max_graphs:
            raise ValueError(f"DGLBucketedStep: a batch of {B} graphs exceeds max_graphs={self.max_graphs}")
        return B

    def bucket_of(self, g, h):
        """The capacity bucket of a batch: from tensor shapes on the host, no device read."""
        self._num_graphs(g)
        src, _ = g.edges()
        N, E = int(h.shape[0]), int(src.numel())
        return DGLBucket(_round_up(N + 1, self.granule["N"]), _round_up(max(E, 1), self.granule["E"]))

    def step(self, g, h, p, e, snorm_n, targets, bucket=None):
        """One training step on a batch (targets [num_graphs, 1]): returns the loss (a device scalar, rewritten by the next step of the
        same bucket).  `bucket`: explicit capacities (DGLBucket / (N_cap, E_cap)) instead of the granule rounding."""
        self._check_form(g)
        self._num_graphs(g)
        b = self.bucket_of(g, h) if bucket is None else DGLBucket(*bucket)
        N = int(h.shape[0])
        if p is None and self.lap_method is None:
            p = self._zero_p(N, h.device)                # pe_init 'no_pe': the pad keeps its pos_enc columns, all zero and never read
        if p is None or tuple(p.shape) != (N, self.K):
            raise ValueError(f"DGLBucketedStep: p has shape {None if p is None else tuple(p.shape)}, expected [N, pos_enc_dim] = "
                             f"[{N}, {self.K}] (the raw pos_enc)")
        from . import ops
        ops.check_node_total(g.batch_num_nodes(), N)     # (host counts; device counts: the pack flags them, check() raises)
        batch = (g, h, p, e, snorm_n, targets)
        if self._admit(b):
            cap = self._lru[b]
            ops.bucket_pack_dgl(*batch, cap.pad)
            self.hits += 1
        else:
            from . import train_stage
            train_stage.flush_deferred()      # (nothing of an earlier eager backward may be left for the captured one to reduce)
            self.model.train()
            cap = _DGLBucketCapture(self, b, batch, self.warmup)
            self._lru[b] = cap
            self.captures += 1
        self._from_store = False
        return self._replay(cap)

    def step_from(self, store, idx, bucket=None):
        """step() on the graphs `idx` of a data.DGLGraphStore: host indices, or the (host indices, device view) pair an IndexLoader
        yields — then nothing is copied to the device.  The batch reaches the capacity buffers through store.gather_into (ONE
        sn_store_gather launch in place of the pack launch); same LRU, capture, replay and check()."""
        if not getattr(store, "dgl", False):
            raise TypeError("DGLBucketedStep.step_from needs a data.DGLGraphStore")
        self._check_form()
        if store.K != self.K:
            if self.lap_method is not None or self._lru:
                raise ValueError(f"DGLBucketedStep: the store holds pos_enc of {store.K} columns, the net takes {self.K}" +
                                 ("" if self.lap_method is not None else " in the buckets captured so far (release() them first)"))
            self.K = int(store.K)                        # pe_init 'no_pe': the stored pos_enc is gathered and ignored
        return self._step_from(store, idx, bucket, DGLBucket,
                               lambda b, fill: _DGLBucketCapture(self, b, store.proto(), self.warmup, fill=fill))


class GraphedForward:
    """A no-grad forward of FIXED shape captured once as a HIP graph: `fn` is a closure over static device tensors (BasisNet on the one
    grid graph of LearningFilters, a serving loop with a padded batch); `replay()` re-runs its launches with one graph launch and
    returns the same output tensors, refreshed in place.  Copy new inputs into the tensors `fn` closes over before replaying.
    A module's `matmul_precision` travels with every stage launch, so the captured graph holds the mode the module had when `fn` was
    captured; changing the property afterwards affects eager forwards and later captures only."""

    def __init__(self, fn, warmup=2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = fn()

    def replay(self):
        self.graph.replay()
        return self.out
