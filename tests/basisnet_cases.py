"""Case tables, input generators and dtype-generic torch restatements for the BasisNet / LearningFilters grid
(tests/test_basisnet_grid_gpu.py runs the HIP kernels on them, tests/test_basisnet_cases_cpu.py checks the conditions that make that
comparison mean something).  Importable without a GPU: nothing here touches a device or the package's library.

The kernels of csrc/eigenspace.hip, csrc/ign_mlp.hip and the IGN contractions at the end of csrc/ops.hip pick a kernel, a template
instance or a code path from the shape, the pointer alignment and the data (eigenspace multiplicities).  A row of a table exists for
such a choice: its `branch` string names it (several names joined by " | " when one launch takes several), and the `*_branch` functions
restate the host code of the .hip file (shape, alignment -> branch string).  The CPU test asserts predicate(row) == row.branch and that
the rows of an op reach every name its predicate can return, so an edit of a table cannot silently move a case onto another path.

A restatement is the operation itself in the dtype it is given — never the kernel's blocking: float64 is the exact value, float32 is the
reference's own arithmetic.  Forward values only: they are continuous through ReLU, so no ReLU margin is needed.
"""
import zlib

import torch

F32, F64 = torch.float32, torch.float64
BN_EPS = 1e-5


class Case:
    def __init__(self, op, name, branch, **p):
        self.op, self.name, self.branch, self.p = op, name, branch, p

    @property
    def id(self):
        return f"{self.op}-{self.name}"

    def __repr__(self):
        return self.id


class Op:
    def __init__(self, cases, predicate, branches):
        self.cases, self.predicate, self.branches = cases, predicate, set(branches)


def rng(case, salt=0):
    """one generator per row (and per use inside the row)"""
    return torch.Generator().manual_seed((zlib.crc32(case.id.encode()) + 7919 * salt) % (2 ** 31))


def cdiv(a, b):
    return (a + b - 1) // b


def branches_of(cases):
    return {b for c in cases for b in c.branch.split(" | ")}


# ============================================================================ sn_ign_contract_2to1_f32 (csrc/ops.hip)
IGN_STRIP_MIN, IGN_PANEL = 64, 1024


def contract_branch(p):
    """sn_ign_contract_2to1_f32: 128-row strips from n = 512 on when that still gives 256 workgroups; k_ign_rowcol_v4 when n % 4 == 0 and
    X (and the scratch, which the caller aligns) is 16-byte aligned, else the scalar k_ign_rowcol; both walk 1024-column panels."""
    b, n = p["b"], p["n"]
    strip = 128 if n >= 512 else IGN_STRIP_MIN
    if b * cdiv(n, strip) < 256:
        strip = IGN_STRIP_MIN
    panels = cdiv(n, IGN_PANEL)
    assert panels <= 2
    if n % 4 == 0 and p.get("misaligned"):
        assert panels == 1 and strip == 64
        return "scalar (misaligned X)"
    return f"{'v4' if n % 4 == 0 else 'scalar'}, {panels} panel{'s' if panels > 1 else ''}, strip {strip}"


def _c(b, n, **kw):
    p = dict(b=b, n=n, **kw)
    return Case("ign_contract_2to1", f"b{b}-n{n}" + ("-misaligned" if kw.get("misaligned") else ""), contract_branch(p), **p)


CONTRACT = [
    _c(3, 1), _c(2, 4), _c(3, 37), _c(2, 64), _c(2, 65),
    _c(1, 1027),                    # scalar, second panel of 3 columns
    _c(1, 1028),                    # v4, second panel of one float4
    _c(64, 512),                    # 64 * 4 = 256 workgroups: the first count that takes the 128-row strip
    _c(52, 513),                    # 52 * 5 = 260: scalar, 128-row strip, a last strip of one row
    _c(2, 100, misaligned=True),
    # the second panel under the 128-row strip needs n > 1024 and b * ceil(n / 128) >= 256: b = 29 is the smallest (122 MB of input)
    _c(29, 1028), _c(29, 1027),
]
CONTRACT_BRANCHES = {f"{k}, {pn}, strip {s}" for k in ("scalar", "v4") for pn in ("1 panel", "2 panels") for s in (64, 128)} | \
                    {"scalar (misaligned X)"}
COLUMNS = ("diag", "trace/n", "rowsum/n", "colsum/n", "total/n^2")


def contract_gen(case):
    """uniform(0, 1) entries plus a distinct diagonal in [1, 2): all five columns are sums of positive terms (no cancellation), rows,
    columns and matrices differ"""
    b, n = case.p["b"], case.p["n"]
    X = torch.rand(b, n, n, generator=rng(case))
    X.diagonal(dim1=1, dim2=2).add_(1.0 + torch.arange(n, dtype=F32) / n)
    return X


def contractions_2to1(X):
    """contractions_2_to_1 with normalization 'inf' on X [b, n, n] -> [b, n, 5] = [X_ii, tr / n, rowsum_i / n, colsum_i / n, sum / n^2],
    in X's dtype"""
    n = X.shape[-1]
    diag = torch.diagonal(X, dim1=1, dim2=2)
    return torch.stack([diag, diag.sum(1, keepdim=True).expand(-1, n) / n, X.sum(2) / n, X.sum(1) / n,
                        X.sum((1, 2)).unsqueeze(1).expand(-1, n) / n ** 2], dim=2)


# ============================================================================ sn_eigenspace_group (csrc/eigenspace.hip)
EIG_MAXN, EIG_T = 8192, 256


def spectrum(mults, spacing, start=0.0):
    """ascending eigenvalues: the k-th distinct value start + k * spacing, repeated mults[k] times (float32)"""
    vals = start + spacing * torch.arange(len(mults), dtype=F64)
    return torch.repeat_interleave(vals.float(), torch.tensor(mults))


def fill(N, head=(), cycle=(1, 2, 3, 1, 1, 4)):
    """a multiplicity list that starts with `head` and sums to N"""
    out, i = list(head), 0
    assert sum(out) <= N
    while sum(out) < N:
        out.append(min(cycle[i % len(cycle)], N - sum(out)))
        i += 1
    return out


def group_branch(p):
    """k_eig_group has one launch shape; what varies is how the runs of equal keys meet the chunks of the scan (thread t owns
    [t * per, (t + 1) * per), per = ceil(N / 256)) — named from the row's expected multiplicities."""
    mults = p["mults"]
    N = sum(mults)
    per = cdiv(N, EIG_T)
    names = [f"per {per}"]
    starts = [sum(mults[:k]) for k in range(len(mults))]
    if p.get("values") is not None:
        names = ["edge values"]
    elif len(mults) == 1:
        names.append("N = 1" if N == 1 else "all equal")
    elif all(m == 1 for m in mults):
        names.append("all distinct")
    elif per > 1:
        if any((s + m - 1) // per - s // per >= 2 for s, m in zip(starts, mults)):
            names.append("run spans >= 3 chunks")
        if any(s > 0 and s % per == 0 and m > 1 for s, m in zip(starts, mults)):
            names.append("run starts at t * per")
    if p["decimals"] != 5:
        names.append(f"decimals {p['decimals']}")
    return " | ".join(names)


def _g(name, mults, spacing=0.01, decimals=5, values=None, start=0.0):
    p = dict(mults=list(mults), spacing=spacing, decimals=decimals, values=values, start=start)
    return Case("eigenspace_group", name, group_branch(p), **p)


GROUP = [
    _g("N1", [1]),
    _g("N5", [1, 2, 2]),
    _g("N5-all-equal", [5], start=0.3),
    _g("N255-all-distinct", [1] * 255),
    _g("N256-all-distinct", [1] * 256, spacing=2e-5),             # neighbours two rounding steps apart
    _g("N256-mixed", fill(256, (3, 1, 40))),
    _g("N257-mixed", fill(257, (1, 5, 2, 7))),                   # per 2: [1, 6) covers chunks 0..2; a run of 2 starts at 6 = 3 * per
    _g("N257-all-distinct", [1] * 257),
    _g("N300-mixed", fill(300, (2, 33, 1, 70, 4))),              # [2, 35) and [36, 106) span many chunks, the run of 4 starts at 106
    _g("N300-all-equal", [300], start=1.25),
    _g("N8192-mixed", fill(8192, (31, 1, 100, 28, 64, 700))),    # per 32: [32, 132) spans 4 chunks; the run of 64 starts at 160 = 5 * per
    _g("N8192-all-distinct", [1] * 8192),
    _g("N8192-all-equal", [8192], start=2.0),
    # explicit values (mults = the grouping they must give)
    _g("signed-zeros", [3], values=[-1e-7, 0.0, 1e-7]),                          # keys -0.0, +0.0, +0.0: one space
    _g("split-across-a-rounding-boundary", [1, 1], values=[0.500003, 0.500007]),  # 4e-6 apart: 50000.3 | 50000.7
    _g("merged-inside-a-rounding-step", [2], values=[0.5000055, 0.5000145]),      # 9e-6 apart: 50000.55, 50001.45 -> 50001
    _g("half-even-decimals0", [1, 2], decimals=0, values=[0.5, 1.5, 2.5]),        # -> 0, 2, 2
    _g("decimals0", fill(40, (2, 5)), decimals=0, spacing=1.0),
    _g("decimals7", [2, 3, 1, 1], decimals=7, values=[0.0, 0.0, 3e-7, 3e-7, 3e-7, 4e-7, 0.01]),
    _g("decimals7-N300", fill(300, (1, 2)), decimals=7, spacing=1e-6),
]
GROUP_BRANCHES = {"per 1", "per 2", "per 32", "run spans >= 3 chunks", "run starts at t * per", "all distinct", "all equal", "N = 1",
                  "edge values", "decimals 0", "decimals 7"}
GROUP_REFUSED = [dict(N=1, decimals=8, match="decimals"), dict(N=0, decimals=5, match="N=0"), dict(N=EIG_MAXN + 1, decimals=5, match="N=8193")]


def group_gen(case):
    p = case.p
    if p["values"] is not None:
        return torch.tensor(p["values"], dtype=F32)
    return spectrum(p["mults"], p["spacing"], p["start"])


def group_reference(eigvals, decimals):
    """The statements of the reference's preprocessing in float32 torch (`around` = round(x * 10**d) / 10**d, `unique`, the dict
    {multiplicity: cat(projectors)} in ascending multiplicity), as integer tables:
    space_of [N], space_start [ns + 1], space_mult [ns], space_slot [ns] (position in the multiplicity-major stack), mults, counts."""
    assert eigvals.dtype == F32
    rounded = torch.round(eigvals * 10 ** decimals) / (10 ** decimals)
    _, inv, counts = rounded.unique(return_inverse=True, return_counts=True)
    ns = counts.numel()
    mults = sorted(set(counts.tolist()))
    order = [s for m in mults for s in range(ns) if counts[s] == m]          # eigenvalue order inside a multiplicity
    slot = torch.empty(ns, dtype=torch.int32)
    slot[torch.tensor(order)] = torch.arange(ns, dtype=torch.int32)
    i32 = lambda t: t.to(torch.int32)
    return dict(space_of=i32(inv), space_start=i32(torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])), space_mult=i32(counts),
                space_slot=slot, mults=mults, counts=[int((counts == m).sum()) for m in mults], n_spaces=ns, max_mult=int(counts.max()))


# ============================================================================ sn_eigenspace_projectors_f32 / sn_ign_contract_eigvecs_f32
PROJ_KC = 32


def projector_branch(p):
    """k_eig_projectors: an eigenspace of multiplicity m takes ceil(m / 32) passes of min(32, rest) eigenvectors; a pass of mc eigenvectors
    runs proj_pass<2 | 4 | 8 | 32> (mc <= 2, <= 4, <= 8, else); passes after the first accumulate."""
    names = set()
    for m in p["mults"]:
        passes = cdiv(m, PROJ_KC)
        if passes > 1:
            names.add(f"{passes} passes")
        for kc in range(0, m, PROJ_KC):
            mc = min(PROJ_KC, m - kc)
            names.add(f"proj_pass<{2 if mc <= 2 else 4 if mc <= 4 else 8 if mc <= 8 else 32}>")
    if p.get("pad"):
        names.add("ldv > N")
    return " | ".join(sorted(names))


def _p(name, mults, pad=0):
    p = dict(mults=list(mults), pad=pad)
    return Case("eigenspace_projectors", name, projector_branch(p), **p)


PROJECTORS = [
    _p("N70-one-eigenspace", [70]),                                                      # 32 + 32 + 6
    _p("N70-ldv73", [1, 2, 3, 5, 9, 17, 33], pad=3),
    _p("N200", [1, 2, 3, 5, 9, 32, 33, 70, 45]),
    _p("N300", [70, 33, 32, 9, 5, 3, 2, 1, 64, 17, 8, 4, 6, 7, 39]),
]
PROJECTOR_BRANCHES = {"proj_pass<2>", "proj_pass<4>", "proj_pass<8>", "proj_pass<32>", "2 passes", "3 passes", "ldv > N"}
PROJECTOR_MULTS = {1, 2, 3, 5, 9, 32, 33, 70}         # each must occur in a row (m = 33: a second pass of one eigenvector)


def projector_gen(case):
    """-> (eigvals [N] float32 with the row's multiplicities, V [N, N] = float32 of the Q factor of a seeded float64 Gaussian matrix)"""
    mults = case.p["mults"]
    N = sum(mults)
    Q, _ = torch.linalg.qr(torch.randn(N, N, generator=rng(case), dtype=F64))
    return spectrum(mults, 0.01), Q.float()


def projectors(V, ref, dtype):
    """[n_spaces, N, N]: V_s V_s^T of the float32 V in `dtype`, stacked multiplicity-major (ref = group_reference(...))"""
    V = V.to(dtype)
    st, slot = ref["space_start"].tolist(), ref["space_slot"].tolist()
    out = torch.empty(ref["n_spaces"], V.shape[0], V.shape[0], dtype=dtype)
    for s in range(ref["n_spaces"]):
        Vs = V[:, st[s]:st[s + 1]]
        out[slot[s]] = Vs @ Vs.T
    return out


# ============================================================================ sn_ign_mlp_f32 (csrc/ign_mlp.hip)
IGN_WAVES = 8


def ign_mlp_supported(n, H, O):
    return H in (16, 32) and 1 <= n <= 1024 and 1 <= O <= 32


def ign_mlp_branch(p):
    """launch_h: tiles of 16 rows, 8 waves; tiles per wave rounded up to 1, 2, 4 or 8"""
    n, H, O = p["n"], p["H"], p["O"]
    if not ign_mlp_supported(n, H, O):
        return "not supported"
    tpw = cdiv(cdiv(n, 16), IGN_WAVES)
    T = 1 if tpw <= 1 else 2 if tpw <= 2 else 4 if tpw <= 4 else 8
    return f"k_ign_mlp<{H},{T}>"


def _m(b, n, H, O, **kw):
    p = dict(b=b, n=n, H=H, O=O, **kw)
    return Case("ign_mlp", f"b{b}-n{n}-H{H}-O{O}" + ("-no-fc2-bias" if kw.get("no_fc2_bias") else ""), ign_mlp_branch(p), **p)


IGN_MLP = [
    # (1, 300, 16, 32) is the row that found k_ign_mlp<16, 4> reading a tile's accumulator too early when the wave's next tile is invalid
    # as a whole
    _m(3, 1, 16, 1), _m(1, 7, 16, 5), _m(3, 16, 16, 17), _m(1, 129, 16, 16), _m(3, 256, 16, 31), _m(1, 300, 16, 32), _m(3, 512, 16, 4),
    _m(1, 650, 16, 17), _m(1, 1024, 16, 32),
    _m(1, 1, 32, 32), _m(3, 17, 32, 4), _m(1, 128, 32, 31), _m(3, 129, 32, 1), _m(1, 256, 32, 32), _m(1, 257, 32, 17), _m(3, 300, 32, 5),
    _m(1, 513, 32, 16), _m(3, 650, 32, 31), _m(1, 1024, 32, 1),
    _m(3, 300, 32, 17, no_fc2_bias=True),
]
IGN_MLP_BRANCHES = {f"k_ign_mlp<{H},{T}>" for H in (16, 32) for T in (1, 2, 4, 8)}
IGN_MLP_UNSUPPORTED = [_m(1, 1025, 16, 2), _m(2, 20, 8, 3), _m(2, 20, 64, 3), _m(2, 20, 16, 33)]
IGN_MLP_N = {1, 7, 16, 17, 128, 129, 256, 257, 300, 512, 513, 650, 1024}
IGN_MLP_O = {1, 4, 5, 16, 17, 31, 32}


def ign_mlp_gen(case):
    """-> (o [b, n, 5], state): random equivariant coefficients and biases, random fc weights, random BatchNorm affine and running
    statistics (the running statistics as parity_util.bn_randomize draws them); a different matrix per batch entry"""
    p = case.p
    H, O = p["H"], p["O"]
    g = rng(case)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"equi_layers.0.coeffs": r(1, H, 5) * 0.6, "equi_layers.0.bias": r(1, H, 1) * 0.3}
    for i in (1, 2):
        sd[f"equi_layers.{i}.coeffs"] = r(H, H, 2) * (1.0 / H ** 0.5)
        sd[f"equi_layers.{i}.bias"] = r(1, H, 1) * 0.3
    for i in range(3):
        sd[f"bns.{i}.weight"] = 1.0 + 0.3 * r(H)
        sd[f"bns.{i}.bias"] = 0.3 * r(H)
        sd[f"bns.{i}.running_mean"] = r(H) * 0.1
        sd[f"bns.{i}.running_var"] = torch.rand(H, generator=g) + 0.5
    sd["fc1.weight"], sd["fc1.bias"] = r(H, H) * (1.0 / H ** 0.5), r(H) * 0.3
    sd["fc2.weight"] = r(O, H) * (1.0 / H ** 0.5)
    sd["fc2.bias"] = torch.zeros(O) if p.get("no_fc2_bias") else r(O) * 0.3
    o = r(p["b"], p["n"], 5) + torch.arange(p["b"], dtype=F32).view(-1, 1, 1) * 0.25
    return o, sd


def ign_head(o, sd, dtype):
    """IGN2to1.forward behind the contractions, written out from o [b, n, 5] (eval-mode BatchNorm) -> [b, O, n]:
    layer_2_to_1 -> relu -> bn, two layer_1_to_1 (identity block + mean block) -> relu -> bn, fc1 -> relu -> fc2, transposed."""
    w = {k: v.to(dtype) for k, v in sd.items()}

    def bn(h, i):
        return (h - w[f"bns.{i}.running_mean"]) / torch.sqrt(w[f"bns.{i}.running_var"] + BN_EPS) * w[f"bns.{i}.weight"] + w[f"bns.{i}.bias"]

    h = o.to(dtype) @ w["equi_layers.0.coeffs"][0].T + w["equi_layers.0.bias"].reshape(-1)               # [b, n, H]
    h = bn(torch.relu(h), 0)
    for i in (1, 2):
        c = w[f"equi_layers.{i}.coeffs"]                                                                  # [D, S, 2]
        h = h @ c[:, :, 0] + h.mean(1, keepdim=True) @ c[:, :, 1] + w[f"equi_layers.{i}.bias"].reshape(-1)
        h = bn(torch.relu(h), i)
    h = torch.relu(h @ w["fc1.weight"].T + w["fc1.bias"])
    return (h @ w["fc2.weight"].T + w["fc2.bias"]).transpose(2, 1).contiguous()


# ============================================================================ sn_deepsets_tail_f32 (csrc/ign_mlp.hip)
DS_MAX_LAYERS, DS_W, DS_BUF = 8, 32, 16384


def deepsets_supported(n, widths):
    """the entry point's conditions: 2..8 layers, widths 1..32, n * (widest layer but the last) <= 16384"""
    return 2 <= len(widths) <= DS_MAX_LAYERS and all(1 <= w <= DS_W for w in widths) and n >= 1 and n * max(widths[:-1]) <= DS_BUF


def deepsets_branch(p):
    if not deepsets_supported(p["n"], p["widths"]):
        return "not supported"
    return f"split0 = {p['split0']}, use_bn = {p['use_bn']}"


def _d(n, widths, use_bn, split0, fin=6):
    p = dict(n=n, widths=list(widths), use_bn=use_bn, split0=split0, fin=fin)
    return Case("deepsets_tail", f"n{n}-w{'x'.join(str(w) for w in widths)}-bn{use_bn}-split{split0}", deepsets_branch(p), **p)


DEEPSETS = [
    _d(1, [10, 10], 1, 1),                                  # one row: batch variance 0
    _d(1, [32, 5], 0, 0),
    _d(31, [1, 1], 1, 0),
    _d(32, [31, 32], 0, 1),
    _d(33, [32, 24, 16, 8, 4, 3, 2, 3], 1, 1),              # SN_DEEPSETS_MAX_LAYERS, shrinking
    _d(1023, [1, 2, 4, 8, 10, 12, 14, 16], 0, 0),           # SN_DEEPSETS_MAX_LAYERS, growing
    _d(1024, [10, 16, 32], 1, 1),                           # the last layer wider than every LDS-resident one, 1024 * 16 at the limit
    _d(512, [32, 32, 7], 1, 0),                             # n * widest == 16384
    _d(512, [32, 10], 0, 1),
]
DEEPSETS_BRANCHES = {f"split0 = {s}, use_bn = {u}" for s in (0, 1) for u in (0, 1)}
DEEPSETS_OVER_LIMIT = _d(513, [32, 32, 7], 1, 1)


def deepsets_gen(case):
    """-> (x [n, fin], layers): layers[i] = dict(w1, b1, w2, b2[, gamma, beta]) of EqDeepSetsEncoder's layer i (fin -> widths[0] -> ...)"""
    p = case.p
    g = rng(case)
    r = lambda *s: torch.randn(*s, generator=g)
    dims = [p["fin"]] + p["widths"]
    layers = []
    for i in range(len(p["widths"])):
        din, dout = dims[i], dims[i + 1]
        L = dict(w1=r(dout, din) / din ** 0.5, b1=0.2 + 0.3 * torch.rand(dout, generator=g), w2=r(dout, din) / din ** 0.5, b2=0.3 * r(dout))
        if p["use_bn"] and i < len(p["widths"]) - 1:
            L["gamma"], L["beta"] = 1.0 + 0.3 * r(dout), 0.2 + 0.3 * torch.rand(dout, generator=g)
        layers.append(L)
    return r(p["n"], p["fin"]), layers


def layers_of(enc):
    """the same list from an EqDeepSetsEncoder module"""
    out = []
    for i, (l1, l2) in enumerate(zip(enc.lins1, enc.lins2)):
        L = dict(w1=l1.weight, b1=l1.bias, w2=l2.weight, b2=l2.bias)
        if enc.use_bn and i < len(enc.lins1) - 1:
            L["gamma"], L["beta"] = enc.bns[i].weight, enc.bns[i].bias
        out.append({k: v.detach().cpu() for k, v in L.items()})
    return out


def eq_deepsets(x, layers, dtype=F64, eps=BN_EPS):
    """EqDeepSetsEncoder.forward on one set x [n, F] written out: h = lin1(h) + lin2(mean_n h); behind every layer but the last relu and,
    where the layer has gamma / beta, BatchNorm with the statistics of the n rows (biased variance)."""
    h = x.detach().cpu().to(dtype)
    for i, L in enumerate(layers):
        w = {k: v.detach().cpu().to(dtype) for k, v in L.items()}
        h = h @ w["w1"].t() + w["b1"] + (h.mean(0, keepdim=True) @ w["w2"].t() + w["b2"])
        if i < len(layers) - 1:
            h = torch.relu(h)
            if "gamma" in w:
                h = (h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + eps) * w["gamma"] + w["beta"]
    return h


def deepsets_first_layer(x, L0, split0):
    """what the caller hands to sn_deepsets_tail_f32, in float32 on the host: split0 = 1: z [n, 2 w] = x [W1 ; W2]^T + [b1 ; b2];
    split0 = 0: z [n, w] = lin1(x) + lin2(mean x), the first layer's pre-activation"""
    if split0:
        return (x @ torch.cat([L0["w1"], L0["w2"]], 0).t() + torch.cat([L0["b1"], L0["b2"]], 0)).contiguous()
    return (x @ L0["w1"].t() + L0["b1"] + (x.mean(0, keepdim=True) @ L0["w2"].t() + L0["b2"])).contiguous()


OPS = {
    "ign_contract_2to1": Op(CONTRACT, contract_branch, CONTRACT_BRANCHES),
    "eigenspace_group": Op(GROUP, group_branch, GROUP_BRANCHES),
    "eigenspace_projectors": Op(PROJECTORS, projector_branch, PROJECTOR_BRANCHES),
    "ign_mlp": Op(IGN_MLP, ign_mlp_branch, IGN_MLP_BRANCHES),
    "deepsets_tail": Op(DEEPSETS, deepsets_branch, DEEPSETS_BRANCHES),
}
ALL = [c for op in OPS.values() for c in op.cases]
