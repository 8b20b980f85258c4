"""Case table, references and acceptance rule of the reduced-precision stage grid (tests/test_precision_stage_grid_gpu.py runs every
`high` / `medium` instance of the eval stage kernels on it, tests/test_precision_stage_cases_cpu.py checks without a GPU that the table
reaches every instance and that the rule is decided by the kernels, not by the reference).  Importable without a GPU.

`matmul_precision = "high" | "medium"` compiles its own instances of the phi, rho and DGL stage kernels (csrc/fused_phi_high.hip, ...,
dispatch_mlp<PREC>) at the tile counts fused.REDUCED_TILES / REDUCED_TILES_DGL.  The rows are those of tests/stage_cases.py at these
tile counts, the first per distinct (phi, rho) branch pair — the GINE stage stays at `highest` and is not a reason for a row — plus rows
for the LDS-attention instances the float64 grid reaches only at other widths.  Shapes, seeds and models are stage_cases'.

The rule (mode identification at stage level).  R(a, b) = rms(a - b) over a stage's output (phi: valid slots) or over one graph's rows
of it.  For SignNetGNN the kernels split exactly the weights precision_emulation.emulated_oracle splits (BatchNorm is an epilogue vector
there), for DeepSigns exactly those of emulated_dgl_oracle(folded=True), so kernel and float64 emulation of one mode differ by fp32
arithmetic alone.  With emu64_m the float64 emulation of mode m and gap_m = min over the neighbouring modes n of R(emu64_m, emu64_n):

    R(gpu_m, emu64_m) <= gap_m / 4        for the whole tensor, for every graph of the batch, and (SignNetGNN stages) for every
                                          16-channel tile of the output over all rows

(the tiles: fed an emulation that takes a neighbouring mode's products in the last 16-channel tile only, the whole-tensor and per-graph
ratios of a 128-wide row come out at 0.27 .. 0.36, over the line by a factor 1.1 .. 1.4; the tile alone is at 0.52 .. 0.65, and one graph of the batch served so is at 1.0.)  A result is nearer
its own product set than a neighbour's exactly when the ratio is below 1/2; the 4 leaves a factor 2 on that.  The CPU test holds the
float32 emulation (the same planes and products, multiplied and summed in float32) to gap / 8 on every row, stage, mode, graph and
tile, which leaves another factor 2 between what fp32 arithmetic alone does and what a kernel may do.  Nothing is taken from a
kernel's output.
"""
import functools

import pytest
import torch

import precision_emulation as PE
import stage_cases as SC
from signnet_basisnet_amd import fused

REDUCED = ("high", "medium")
NEIGHBOURS = {"high": ("highest", "medium"), "medium": ("high",)}
GPU_FACTOR, CPU_FACTOR = 4.0, 8.0


# Rows whose first draw of weights leaves the float32 emulation itself outside gap / 8 at `high` on some graph (mostly a one- or
# two-node graph: 60 to 128 numbers) or in some 16-channel tile, or within 20 % of it, so that the CPU test does not hinge on one BLAS's
# summation order.  The salt (stage_cases.seed_of) is the smallest whose draw brings the float32 emulation below 0.8 gap / 8 everywhere;
# the GPU never had a say.
SALT = {"pyg-gine-h64-kall-rho1": 1, "pyg-alchemy-h64-k7-rho2": 1, "pyg-gine-h60-k17-rho1": 2, "pyg-gine-h128-k7-rho1": 1,
        "pyg-alchemy-h64-kall-rho2": 1, "pyg-alchemy-h108-kall-rho2": 2, "pyg-alchemy-h128-k7-rho2": 2, "pyg-alchemy-h124-k7-rho2": 1,
        "pyg-gine-h128-kall-rho1": 1, "pyg-gine-h124-k16-rho1": 1, "pyg-gine-h60-k16-rho2": 3, "pyg-gine-h112-k16-rho2": 4,
        "pyg-alchemy-h64-k20-rho2": 3,
        "dgl-gin-h64-c3-k37": 1, "dgl-gin-h67-c3-k37": 1, "dgl-gin-h95-c4-k1": 4, "dgl-masked_gin-h64-c4-k1": 1, "dgl-masked_gin-h95-c17-k1": 1}


def _salted(c):
    return SC.Case(c.op, c.name, c.branch, **{**c.p, "salt": SALT[c.id]}) if c.id in SALT else c


# ============================================================================ the SignNetGNN rows
def _pair(c):
    return SC.phi_branch(c.p), SC.rho_branch(c.p)


def _pyg_rows():
    rows, seen = [], set()
    for c in SC.PYG:
        if SC.cdiv(c.p["hid"], 16) in fused.REDUCED_TILES and _pair(c) not in seen:
            seen.add(_pair(c))
            rows.append(c)
    # LDS attention (more than 16 slots and a width that k_rho_wide does not take) with per-graph bins: stage_cases has it at 4 and 8
    # tiles from all eigenvectors only, and at 7 tiles with the eigenvalue encoder only
    extra = [SC._r("gine", 112, 17), SC._r("gine", 60, 17), SC._r("alchemy", 60, 17), SC._r("gine", 124, 17), SC._r("alchemy", 124, 17)]
    ids = {c.id for c in rows}
    return [_salted(c) for c in rows + [c for c in extra if c.id not in ids]]


PYG = _pyg_rows()
PHI_BRANCHES = {f"k_phi_fused<{nt},{h}> {lay}" for nt in fused.REDUCED_TILES for h in ("HID1", "!HID1") for lay in ("columns", "slabs")}
RHO_BRANCHES = ({f"k_rho_fused<4,reg,{o},HP16>" for o in SC.ONES} | {f"k_rho_fused<8,reg,{o},HP32>" for o in SC.ONES} |
                {f"k_rho_fused<{nt},reg,{o}>" for nt in (4, 8) for o in SC.ONES} |
                {f"k_rho_wide<{nt},{o},{c}>" for nt in (4, 8) for o in SC.ONES for c in ("COLS", "!COLS")} |
                {f"k_rho_fused<{nt},lds,{o}>" for nt in fused.REDUCED_TILES for o in SC.ONES})


def stage_branch(case):
    """the row's `branch` without the GINE stage's names"""
    return " | ".join(_pair(case))


# ============================================================================ the DGL rows
def _dgl_rows():
    rows, seen = [], set()
    for c in SC.DGL:
        if SC.dgl_widths(c.p)[0] // 16 in fused.REDUCED_TILES_DGL and c.branch not in seen:
            seen.add(c.branch)
            rows.append(_salted(c))
    return rows


DGL = _dgl_rows()
DGL_PHI_BRANCHES = {f"k_phi_fused<{nt},!HID1,DGL>" for nt in fused.REDUCED_TILES_DGL}
DGL_BRANCHES = DGL_PHI_BRANCHES | {b for c in SC.DGL if c.branch.split(" | ")[0] in DGL_PHI_BRANCHES for b in c.branch.split(" | ")}

# widths without reduced kernels: every other tile count (tests: the launch is refused, nothing is substituted)
REFUSED_HIDDEN = (16, 32, 48, 80, 96)
REFUSED_DGL_HIDDEN = (40, 100)                 # pads to 48 and 112


# ============================================================================ references
def _mp():
    return pytest.MonkeyPatch()


@functools.lru_cache(maxsize=2)
def emulations(case):
    """-> {mode: {phi [N, K, d], rho_sum [N, d], y}} float64, precision_emulation.emulated_oracle in all three modes on stage_cases.reference's
    weights and batch; computed once per row and never modified"""
    sd = SC.reference(case)[0]
    cfg, data, out = SC.oracle_cfg(case.p), SC.batch_of(case), {}
    for mode in PE.MODES:
        _, o = PE.emulated_oracle(mode, _mp(), sd, cfg, data, case.p["max_k"])
        out[mode] = {s: o[s] for s in SC.STAGES}
    return out


def emulations32(case):
    """the same with acc = float32, reduced modes only: the stand-in for a kernel in the CPU test"""
    sd = SC.reference(case)[0]
    cfg, data, out = SC.oracle_cfg(case.p), SC.batch_of(case), {}
    for mode in REDUCED:
        _, o = PE.emulated_oracle(mode, _mp(), sd, cfg, data, case.p["max_k"], acc=torch.float32)
        out[mode] = {s: o[s] for s in SC.STAGES}
    return out


def _dgl_emu(case, mode, **kw):
    p = case.p
    sd, x, _, _ = SC.dgl_reference(case)
    ei = SC.batch_of(case).edge_index
    return PE.emulated_dgl_oracle(mode, _mp(), p["kind"], sd, ei[0], ei[1], torch.tensor(p["sizes"]), x, p["layers"], p["K"], folded=True, **kw)


@functools.lru_cache(maxsize=2)
def dgl_emulations(case):
    """-> {mode: y [N, K, 1]} float64, emulated_dgl_oracle(folded=True) in all three modes"""
    return {mode: _dgl_emu(case, mode) for mode in PE.MODES}


def dgl_emulations32(case):
    return {mode: _dgl_emu(case, mode, acc=torch.float32) for mode in REDUCED}


def dgl_folding_alone(case):
    """the folded restatement with every Linear a plain float64 matmul on the unrounded W': equals the float64 oracle up to rounding"""
    return _dgl_emu(case, None, round_w=False)


# ============================================================================ the rule
def rms(t):
    return t.double().pow(2).mean().sqrt().item() if t.numel() else 0.0


def graph_rows(sizes):
    """[(first row, end row)] of every graph"""
    out, off = [], 0
    for n in sizes:
        out.append((off, off + n))
        off += n
    return out


def _parts(t, mask, sizes):
    """the whole tensor (phi: valid slots) and one part per graph"""
    whole = t if mask is None else t[mask]
    per = [(t[a:b] if mask is None else t[a:b][mask[a:b]]) for a, b in graph_rows(sizes)]
    return whole, per


def rule_ratios(got, emu, mode, stage, sizes, mask=None):
    """-> (R(got, emu64_mode) / gap of the whole tensor, the same of the worst graph, index of that graph).  emu: {mode: {stage: t}} or
    {mode: t}.  got on the host, rows in the emulation's order.  A part with gap 0 and R 0 counts as 0, with gap 0 and R > 0 as inf."""
    pick = lambda m: (emu[m][stage] if isinstance(emu[m], dict) else emu[m]).double()
    own = pick(mode)
    got = got.detach().cpu().double().reshape(own.shape)
    gw, gp = _parts(got, mask, sizes)
    ow, op = _parts(own, mask, sizes)
    nb = [_parts(pick(n), mask, sizes) for n in NEIGHBOURS[mode]]

    def ratio(g, o, others):
        gap, r = min(rms(o - x) for x in others), rms(g - o)
        return r / gap if gap > 0 else (0.0 if r == 0 else float("inf"))

    whole = ratio(gw, ow, [n[0] for n in nb])
    per = [ratio(gp[i], op[i], [n[1][i] for n in nb]) for i in range(len(sizes))]
    worst = max(range(len(sizes)), key=lambda i: per[i])
    return whole, per[worst], worst


def tile_ratios(got, emu, mode, stage, mask=None):
    """-> (R(got, emu64_mode) / gap of the worst 16-channel tile of the stage's output over all rows (phi: valid slots), its index).
    One wrong tile of eight moves the whole-tensor ratio by sqrt(1/8) only; taken alone it shows in full."""
    own = emu[mode][stage].double()
    got = got.detach().cpu().double().reshape(own.shape)
    sel = (lambda t: t) if mask is None else (lambda t: t[mask])
    g, o, nb = sel(got), sel(own), [sel(emu[n][stage].double()) for n in NEIGHBOURS[mode]]
    out = []
    for c in range(0, own.shape[-1], 16):
        gap, r = min(rms(o[..., c:c + 16] - x[..., c:c + 16]) for x in nb), rms(g[..., c:c + 16] - o[..., c:c + 16])
        out.append(r / gap if gap > 0 else (0.0 if r == 0 else float("inf")))
    worst = max(range(len(out)), key=lambda i: out[i])
    return out[worst], worst
