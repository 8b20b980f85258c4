"""Full-graph attention from the bond graph (sn_bond_full_attention_f32, TransformerNet.full_graph_input = "bonds"): case tables and
helpers shared by tests/test_bond_attention_cpu.py and tests/test_bond_attention_gpu.py.

A case is an input set of tests/full_graph_cases.py (`FC.op_inputs`) restated as bonds: the real pairs of its edge list, in list order,
are the bonds (source, destination, class); every other pair is class 0 of the fake table, so the fake codes of the edge form are
zeroed.  The float64 reference of the bond form is then FC.full_attention_ref on that edge list — which `expand` rebuilds from the bonds
alone with FC.make_full_graph_ref (tests/test_bond_attention_cpu.py holds the two equal)."""
import types

import torch

import full_graph_cases as FC

# the kernels' LDS staging budgets (csrc/bond_attention.hip: BA_FWD_LDS, BA_BWD_LDS) and their layout — restated here so that the
# tables below are plain data; tests/test_bond_attention_cpu.py asserts that the library answers the same numbers
FWD_LDS, BWD_LDS = 32768, 36864


def lds_bytes(n, dk, bwd):
    return 4 * n * (6 * dk + 2 if bwd else 3 * dk) + (n * n + 3) // 4 * 4


def staged_nodes(dk, bwd):
    n = 0
    while lds_bytes(n + 1, dk, bwd) <= (BWD_LDS if bwd else FWD_LDS):
        n += 1
    return n


PATTERNS = ("molecule", "all_real", "none_real", "one_direction", "shuffled")       # ("incomplete", "both_kinds": no bond form)


def bond_inputs(heads, dk, C=4, pattern="molecule", gamma=0.1, seed=0, scale=1.0, sizes=tuple(FC.GRID_SIZES)):
    """One case: FC.op_inputs' blocks, tables, gamma and cotangent; its edge list with the fake codes zeroed (src, dst, codes: the
    reference's input); and the bonds bsrc, bdst, bcls (int64) the kernel gets.  'shuffled' permutes the BONDS' edge order."""
    inp = FC.op_inputs(heads, dk, C=C, pattern="molecule" if pattern == "shuffled" else pattern, gamma=gamma, seed=seed, scale=scale,
                       sizes=sizes)
    real = (inp.codes.long() & 1).bool()
    inp.codes = torch.where(real, inp.codes, torch.zeros_like(inp.codes))
    inp.bsrc, inp.bdst, inp.bcls = inp.src[real].contiguous(), inp.dst[real].contiguous(), (inp.codes[real].long() >> 1).contiguous()
    if pattern == "shuffled":
        perm = torch.randperm(inp.bsrc.numel(), generator=torch.Generator().manual_seed(77 + seed))
        inp.bsrc, inp.bdst, inp.bcls = inp.bsrc[perm].contiguous(), inp.bdst[perm].contiguous(), inp.bcls[perm].contiguous()
    inp.pattern = pattern
    return inp


def expand(inp):
    """The edge form rebuilt from the bonds alone: FC.make_full_graph_ref, then codes = 2 * class + real."""
    out = types.SimpleNamespace(**vars(inp))
    fs, fd, real, ef = FC.make_full_graph_ref(inp.sizes, inp.bsrc, inp.bdst, inp.bcls)
    out.src, out.dst, out.codes = fs, fd, (2 * ef + real).to(torch.int32)
    return out


def bond_attention_ref(inp, dtype=torch.float64):
    """The torch restatement of the bond form: expand, then FC.full_attention_ref."""
    a = FC.to_dtype(expand(inp), dtype)
    return FC.full_attention_ref(a.Q, a.K, a.V, a.Q2, a.K2, a.Tr, a.Tf, a.codes, a.gamma, a.src, a.dst, a.heads)


# ----------------------------------------------------------------------------- the op grid
SHAPES = [(8, 8), (4, 32), (1, 3), (3, 10), (8, 4), (2, 16), (5, 24), (6, 5), (7, 2)]      # heads 1..8, dk 3, 4, 8, 10, 16, 24, 32 and two odd ones
GAMMAS = [0.6, -0.3, 1.7]
# graphs around the staging limits at d = 128 (4 heads of 32): the largest staged graph and the first unstaged one, adjoint and forward
LIMIT_DK, LIMIT_HEADS = 32, 4
LIMIT_SIZES = (staged_nodes(LIMIT_DK, True), staged_nodes(LIMIT_DK, True) + 1, staged_nodes(LIMIT_DK, False), staged_nodes(LIMIT_DK, False) + 1)
LIMIT_CASE = dict(heads=LIMIT_HEADS, dk=LIMIT_DK, gamma=0.6, seed=8, sizes=LIMIT_SIZES)
# a graph whose n x n byte table alone (202 500 bytes) exceeds the 160 KiB of LDS a workgroup can have: no staging scheme holds it
HUGE_CASE = dict(heads=2, dk=4, gamma=0.6, seed=9, sizes=(3, 450))
EMPTY_CASE = dict(heads=3, dk=5, gamma=0.6, seed=10, sizes=(5, 0, 9, 1))
CLAMP_CASE = dict(FC.CLAMP_CASE)

CASES = ([dict(heads=h, dk=k) for h, k in SHAPES] +
         [dict(heads=3, dk=5, pattern=p, gamma=0.6, seed=2) for p in PATTERNS if p != "molecule"] +
         [dict(heads=8, dk=8, gamma=g, seed=3) for g in GAMMAS] +
         [dict(heads=3, dk=5, C=c, gamma=0.6) for c in (1, 16)] +
         [CLAMP_CASE, LIMIT_CASE, HUGE_CASE, EMPTY_CASE])


def case_sizes(case):
    return tuple(case.get("sizes", FC.GRID_SIZES))


def path_of(n, dk, bwd):
    """Which path the kernel takes for a graph of n nodes: 'skip' (no node), 'staged' or 'global'."""
    if n <= 0:
        return "skip"
    return "staged" if lds_bytes(n, dk, bwd) <= (BWD_LDS if bwd else FWD_LDS) else "global"


# ----------------------------------------------------------------------------- wrappers: the captured step's comparison rule
# (tests/test_dgl_bucketed_step_gpu.py: the padded step against the eager step, scaled by the eager step's own sensitivity to a 1e-6
#  relative perturbation of pos_enc — zero for a NoPE net, which leaves the floors)
MARGIN = 20.0


def close_losses(eager, noisy, padded, first=1e-6, rel=1e-6):
    assert abs(eager[0] - padded[0]) <= first * abs(eager[0]), (eager, padded)
    scale = 0.0
    for a, n, c in zip(eager, noisy, padded):
        scale = max(scale, abs(a - n))
        assert abs(a - c) <= rel * abs(a) + MARGIN * scale, (eager, noisy, padded)


def close_grads(ge, gn, gp):
    gmax = max(g.abs().max().item() for g in ge.values() if g is not None)
    nmax = max((ge[n] - gn[n]).abs().max().item() for n in ge if ge[n] is not None)
    for n in ge:
        a, b = ge[n], gp[n]
        if a is None or b is None:
            assert (a is None or a.abs().max().item() == 0) and (b is None or b.abs().max().item() == 0), n
            continue
        e = (a - b).abs().max().item()
        noise = max((a - gn[n]).abs().max().item(), 0.05 * nmax)
        print(f"d {n}: |padded - eager| {e:.3e} (gmax {gmax:.3e}, eager noise {noise:.3e})")
        assert e <= 1e-5 * gmax + 1e-6 + MARGIN * noise, f"{n}: {e:.3e} (gmax {gmax:.3e}, eager noise {noise:.3e})"
