"""-m gpu: every `high` / `medium` instance of the eval stage kernels — phi (sn_phi_fused_prec_f32), rho (sn_rho_fused_prec_f32) and the
DGL pair (sn_deepsigns_phi_prec_f32 + sn_mlp_chain_prec_f32) — held to the float64 emulation of its own product set, stage by stage.

One parametrized test over the SignNetGNN rows of tests/precision_stage_cases.py x the two reduced modes, one over its DGL rows.  The
acceptance rule is that module's (mode identification at stage level): with R the rms difference over a stage's output (phi: valid
slots) or over one graph's rows of it, and gap the smallest R between the float64 emulations of the mode and of a neighbouring mode,

    R(gpu, emu64) <= gap / 4        for the whole tensor, for every graph and (SignNetGNN stages) for every 16-channel tile of the output,
                                    in the batch's order and with the graphs reversed

so a kernel that runs a neighbouring mode's products anywhere a graph can see, or drops one, fails.  Every figure is printed before it
is asserted.  The project's coarse bound stays as well: max|gpu - f64| / max|f64| <= 4 x the emulation's + 1e-6 for phi, rho_sum and the
default forward's y.  Then, per SignNetGNN row and mode: each stage once more through its entry point into a sentinel-guarded buffer
(guards intact, phi leaves every invalid slot at the sentinel and writes every valid one, both stages repeat the return_stages values
bit for bit); sign invariance is exact (a seeded random subset of eigenvector columns flipped: phi_fused and y torch.equal); and
`highest` afterwards gives the bits of a forward taken before the mode was first set.  The span recorder names the Python-side stage
(the prec entry points record under "sn_phi_fused_f32" / "sn_rho_fused_f32", as the default ones do).  Widths without reduced
instances refuse the launch with the library's error and leave a sentinel-filled output untouched.

tests/test_precision_stage_cases_cpu.py asserts, without a GPU, that the rows reach every reduced instance and that the float32
emulation — fp32 arithmetic alone — stays within gap / 8 on every row, stage, mode, graph and tile.

Worst R(gpu, emu64) / gap measured on an MI355X (allowed 0.25), beside the float32 emulation's on the same rows (allowed 0.125), as
whole tensor / worst graph / worst 16-channel tile, reversed order included.  Over all: `high` 0.085 / 0.207 / 0.102 against the float32
emulation's 0.076 / 0.100 / 0.092, `medium` 0.021 / 0.031 / 0.044 against 0.016 / 0.030 / 0.023.  The worst graphs are the one- and
two-node ones (37 to 128 numbers).  The DeepSigns rows sit a little above the float32 emulation throughout; the kernels' W' is folded
in float32 on the device and can differ from the emulation's by an ulp, which would move a bf16 plane of about one weight in 256 (a
supposition, not measured).

    stage [branch]                                                            high: gpu             float32           medium: gpu             float32
    phi [k_phi_fused<4,!HID1> columns]                              0.046 / 0.050 / 0.051 0.046 / 0.053 / 0.052   0.007 / 0.019 / 0.008 0.003 / 0.009 / 0.004
    phi [k_phi_fused<4,!HID1> slabs]                                0.034 / 0.041 / 0.058 0.035 / 0.038 / 0.061   0.018 / 0.031 / 0.044 0.004 / 0.007 / 0.006
    phi [k_phi_fused<4,HID1> columns]                               0.042 / 0.046 / 0.048 0.048 / 0.065 / 0.054   0.004 / 0.008 / 0.005 0.004 / 0.009 / 0.005
    phi [k_phi_fused<4,HID1> slabs]                                 0.047 / 0.060 / 0.073 0.046 / 0.059 / 0.073   0.002 / 0.004 / 0.003 0.003 / 0.009 / 0.004
    phi [k_phi_fused<7,!HID1> columns]                              0.027 / 0.031 / 0.033 0.027 / 0.056 / 0.032   0.004 / 0.010 / 0.005 0.001 / 0.002 / 0.001
    phi [k_phi_fused<7,!HID1> slabs]                                0.031 / 0.034 / 0.055 0.031 / 0.033 / 0.055   0.003 / 0.004 / 0.005 0.003 / 0.006 / 0.005
    phi [k_phi_fused<7,HID1> columns]                               0.052 / 0.059 / 0.088 0.055 / 0.070 / 0.092   0.002 / 0.003 / 0.002 0.004 / 0.007 / 0.007
    phi [k_phi_fused<7,HID1> slabs]                                 0.015 / 0.053 / 0.023 0.014 / 0.053 / 0.021   0.001 / 0.003 / 0.002 0.002 / 0.008 / 0.003
    phi [k_phi_fused<8,!HID1> columns]                              0.038 / 0.059 / 0.057 0.036 / 0.051 / 0.058   0.004 / 0.018 / 0.006 0.004 / 0.007 / 0.007
    phi [k_phi_fused<8,!HID1> slabs]                                0.032 / 0.052 / 0.051 0.033 / 0.052 / 0.053   0.003 / 0.005 / 0.005 0.003 / 0.007 / 0.004
    phi [k_phi_fused<8,HID1> columns]                               0.046 / 0.055 / 0.064 0.045 / 0.053 / 0.063   0.005 / 0.012 / 0.009 0.005 / 0.011 / 0.008
    phi [k_phi_fused<8,HID1> slabs]                                 0.039 / 0.081 / 0.073 0.041 / 0.073 / 0.081   0.002 / 0.004 / 0.004 0.003 / 0.010 / 0.005
    rho_sum [k_rho_fused<4,lds,!ONE>]                               0.025 / 0.142 / 0.026 0.024 / 0.064 / 0.025   0.005 / 0.008 / 0.008 0.007 / 0.010 / 0.008
    rho_sum [k_rho_fused<4,lds,ONE>]                                0.016 / 0.089 / 0.019 0.015 / 0.040 / 0.018   0.001 / 0.003 / 0.002 0.003 / 0.004 / 0.003
    rho_sum [k_rho_fused<4,reg,!ONE,HP16>]                          0.035 / 0.082 / 0.045 0.035 / 0.066 / 0.045   0.007 / 0.011 / 0.008 0.004 / 0.007 / 0.006
    rho_sum [k_rho_fused<4,reg,!ONE>]                               0.080 / 0.091 / 0.102 0.076 / 0.100 / 0.086   0.010 / 0.022 / 0.014 0.006 / 0.014 / 0.008
    rho_sum [k_rho_fused<4,reg,ONE,HP16>]                           0.061 / 0.070 / 0.078 0.043 / 0.074 / 0.055   0.000 / 0.000 / 0.000 0.001 / 0.002 / 0.001
    rho_sum [k_rho_fused<4,reg,ONE>]                                0.032 / 0.060 / 0.038 0.034 / 0.096 / 0.041   0.002 / 0.004 / 0.002 0.004 / 0.009 / 0.005
    rho_sum [k_rho_fused<7,lds,!ONE>]                               0.013 / 0.098 / 0.017 0.013 / 0.077 / 0.017   0.005 / 0.010 / 0.007 0.006 / 0.016 / 0.008
    rho_sum [k_rho_fused<7,lds,ONE>]                                0.032 / 0.075 / 0.050 0.031 / 0.056 / 0.050   0.004 / 0.006 / 0.005 0.004 / 0.007 / 0.007
    rho_sum [k_rho_fused<8,lds,!ONE>]                               0.020 / 0.083 / 0.036 0.020 / 0.074 / 0.035   0.006 / 0.010 / 0.012 0.007 / 0.009 / 0.013
    rho_sum [k_rho_fused<8,lds,ONE>]                                0.065 / 0.071 / 0.087 0.062 / 0.071 / 0.081   0.005 / 0.014 / 0.008 0.007 / 0.014 / 0.011
    rho_sum [k_rho_fused<8,reg,!ONE,HP32>]                          0.037 / 0.117 / 0.055 0.037 / 0.093 / 0.055   0.012 / 0.027 / 0.021 0.016 / 0.020 / 0.023
    rho_sum [k_rho_fused<8,reg,!ONE>]                               0.036 / 0.084 / 0.048 0.036 / 0.083 / 0.049   0.011 / 0.018 / 0.015 0.015 / 0.023 / 0.020
    rho_sum [k_rho_fused<8,reg,ONE,HP32>]                           0.051 / 0.056 / 0.065 0.052 / 0.068 / 0.065   0.004 / 0.008 / 0.006 0.004 / 0.007 / 0.005
    rho_sum [k_rho_fused<8,reg,ONE>]                                0.029 / 0.077 / 0.043 0.033 / 0.049 / 0.049   0.007 / 0.014 / 0.012 0.008 / 0.013 / 0.012
    rho_sum [k_rho_wide<4,!ONE,!COLS>]                              0.019 / 0.074 / 0.023 0.020 / 0.044 / 0.024   0.006 / 0.012 / 0.008 0.005 / 0.008 / 0.006
    rho_sum [k_rho_wide<4,!ONE,COLS>]                               0.016 / 0.122 / 0.019 0.016 / 0.060 / 0.019   0.009 / 0.013 / 0.013 0.008 / 0.016 / 0.009
    rho_sum [k_rho_wide<4,ONE,!COLS>]                               0.020 / 0.046 / 0.027 0.023 / 0.046 / 0.030   0.003 / 0.007 / 0.004 0.001 / 0.001 / 0.001
    rho_sum [k_rho_wide<4,ONE,COLS>]                                0.051 / 0.061 / 0.082 0.052 / 0.062 / 0.088   0.003 / 0.004 / 0.004 0.001 / 0.008 / 0.001
    rho_sum [k_rho_wide<8,!ONE,!COLS>]                              0.019 / 0.093 / 0.028 0.019 / 0.096 / 0.028   0.008 / 0.010 / 0.011 0.007 / 0.012 / 0.011
    rho_sum [k_rho_wide<8,!ONE,COLS>]                               0.015 / 0.158 / 0.020 0.014 / 0.083 / 0.018   0.010 / 0.013 / 0.013 0.011 / 0.014 / 0.016
    rho_sum [k_rho_wide<8,ONE,!COLS>]                               0.044 / 0.074 / 0.055 0.044 / 0.063 / 0.054   0.003 / 0.007 / 0.004 0.004 / 0.006 / 0.005
    rho_sum [k_rho_wide<8,ONE,COLS>]                                0.011 / 0.076 / 0.015 0.010 / 0.079 / 0.014   0.004 / 0.009 / 0.005 0.003 / 0.006 / 0.004
    deepsigns y [k_phi_fused<4,!HID1,DGL> | k_mlp_chain<4>]         0.075 / 0.106         0.061 / 0.082           0.000 / 0.000         0.000 / 0.000
    deepsigns y [k_phi_fused<4,!HID1,DGL> | k_mlp_chain<4> masked]  0.062 / 0.115         0.057 / 0.091           0.001 / 0.001         0.001 / 0.001
    deepsigns y [k_phi_fused<4,!HID1,DGL> | k_mlp_chain<7>]         0.080 / 0.127         0.058 / 0.064           0.021 / 0.031         0.003 / 0.005
    deepsigns y [k_phi_fused<4,!HID1,DGL> | k_mlp_chain<8>]         0.052 / 0.067         0.040 / 0.054           0.006 / 0.010         0.006 / 0.012
    deepsigns y [k_phi_fused<5,!HID1,DGL> | k_mlp_chain<5>]         0.072 / 0.098         0.060 / 0.087           0.000 / 0.000         0.000 / 0.000
    deepsigns y [k_phi_fused<5,!HID1,DGL> | k_mlp_chain<5> masked]  0.054 / 0.123         0.035 / 0.054           0.000 / 0.000         0.001 / 0.002
    deepsigns y [k_phi_fused<5,!HID1,DGL> | k_mlp_chain<7>]         0.050 / 0.055         0.037 / 0.044           0.004 / 0.010         0.004 / 0.010
    deepsigns y [k_phi_fused<5,!HID1,DGL> | k_mlp_chain<8>]         0.055 / 0.061         0.034 / 0.042           0.011 / 0.028         0.011 / 0.030
    deepsigns y [k_phi_fused<6,!HID1,DGL> | k_mlp_chain<6>]         0.033 / 0.054         0.027 / 0.043           0.000 / 0.000         0.000 / 0.000
    deepsigns y [k_phi_fused<6,!HID1,DGL> | k_mlp_chain<6> masked]  0.071 / 0.092         0.067 / 0.095           0.000 / 0.000         0.000 / 0.000
    deepsigns y [k_phi_fused<6,!HID1,DGL> | k_mlp_chain<7>]         0.085 / 0.207         0.058 / 0.065           0.018 / 0.030         0.009 / 0.013
    deepsigns y [k_phi_fused<6,!HID1,DGL> | k_mlp_chain<8>]         0.045 / 0.059         0.039 / 0.049           0.003 / 0.005         0.007 / 0.014
"""
import copy

import pytest
import torch

import precision_emulation as PE
import precision_stage_cases as PC
import stage_cases as SC
from test_stage_grid_gpu import SENTINEL, check_guards, guarded, written

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIMIT = 1 / PC.GPU_FACTOR


def _params(cases):
    return [pytest.param(c, m, id=f"{c.id}-{m}") for c in cases for m in PC.REDUCED]


def hold(failures, case, branch, stage, mode, what, ratios, tile=None):
    """print R(gpu, emu64) / gap of the whole tensor, of the worst graph and of the worst 16-channel tile, then note what exceeds the rule"""
    whole, worst, g = ratios
    print(f"\nRULE | {case.id} | {branch} | {stage} | {mode} | {what} | whole {whole:.4f} | worst graph {worst:.4f} (graph {g}) | "
          f"worst tile {'-' if tile is None else f'{tile[0]:.4f} (tile {tile[1]})'} | allowed {LIMIT}", end="")
    if tile is not None and tile[0] > LIMIT:
        failures.append(f"{stage} {mode} {what}: channel tile {tile[1]} {tile[0]:.4f} of the mode gap")
    if whole > LIMIT:
        failures.append(f"{stage} {mode} {what}: whole tensor {whole:.4f} of the mode gap")
    if worst > LIMIT:
        failures.append(f"{stage} {mode} {what}: graph {g} {worst:.4f} of the mode gap")


def coarse(case, stage, mode, got, emu, r64):
    e_gpu, e_emu = PE.relmax(got, r64), PE.relmax(emu, r64)
    print(f"\nCOARSE | {case.id} | {stage} | {mode} | e_gpu {e_gpu:.3e} | e_emu {e_emu:.3e}", end="")
    assert e_gpu <= 4 * e_emu + 1e-6, f"{case.id} {mode} {stage}: e_gpu {e_gpu:.3e} > 4 x e_emu {e_emu:.3e} + 1e-6"


def flip_columns(data, seed):
    """the batch with a seeded random subset of every graph's eigenvector columns negated"""
    g = torch.Generator().manual_seed(seed)
    out = copy.copy(data)
    ev, off = data.eigen_vectors.clone(), 0
    for n in data.sizes:
        s = (torch.rand(n, generator=g) < 0.5).float().mul(2).sub(1)
        ev[off:off + n * n] = (ev[off:off + n * n].view(n, n) * s[None, :]).reshape(-1)
        off += n * n
    out.eigen_vectors = ev
    assert not torch.equal(ev, data.eigen_vectors)
    return out


@pytest.mark.parametrize("case,mode", _params(PC.PYG))
def test_signnet_reduced_stage_row(case, mode):
    from signnet_basisnet_amd import fused, ops, synth
    p = case.p
    sd, o32, o64, mask = SC.reference(case)
    emu = PC.emulations(case)
    data = SC.batch_of(case)
    dd = synth.batch_to(data, DEV)
    model = SC.build_model(case).to(DEV).eval()
    B, N, K, d = len(p["sizes"]), sum(p["sizes"]), SC.slot_count(p), p["hid"]
    sizes, code = list(p["sizes"]), fused.PRECISIONS[mode]
    br = {"phi": SC.phi_branch(p), "rho_sum": SC.rho_branch(p)}
    failures = []
    with torch.no_grad():
        y_first = model(dd).clone()
        model.check_last()
    model.matmul_precision = mode
    rec = ops.KernelTimer()
    with rec, torch.no_grad():
        _, st = model(dd, return_stages=True)
    ran = {s[0] for s in rec.spans}
    assert {"sn_batch_plan", "sn_phi_fused_f32", "sn_rho_fused_f32"} <= ran, sorted(ran)
    assert st["phi_fused"].shape == (N, K, d) and st["rho_sum_fused"].shape == (N, d)
    phi = st["phi_fused"].cpu()
    assert not bool(phi[~mask].any()), f"{case.id}: phi left a nonzero in an invalid slot of a zero-filled buffer"

    # ---- the rule, and the coarse bound
    hold(failures, case, br["phi"], "phi", mode, "batch order", PC.rule_ratios(phi, emu, mode, "phi", sizes, mask),
         PC.tile_ratios(phi, emu, mode, "phi", mask))
    hold(failures, case, br["rho_sum"], "rho_sum", mode, "batch order", PC.rule_ratios(st["rho_sum_fused"], emu, mode, "rho_sum", sizes),
         PC.tile_ratios(st["rho_sum_fused"], emu, mode, "rho_sum"))
    coarse(case, "phi", mode, phi, emu[mode]["phi"], o64["phi"])
    coarse(case, "rho_sum", mode, st["rho_sum_fused"], emu[mode]["rho_sum"], o64["rho_sum"])
    with torch.no_grad():
        y = model(dd).clone()
        model.check_last()
    assert y.shape == o64["y"].shape
    coarse(case, "y", mode, y, emu[mode]["y"], o64["y"])

    # ---- each stage once more through its entry point, into guarded sentinel buffers
    P = model._prep
    plan = ops.build_plan(dd.batch, dd.edge_index, B, p["max_k"] or 0, bins=True)
    dmask = mask.to(DEV)
    with torch.no_grad():
        buf, out = guarded((N, K, d))
        P["phi_fused"].run(plan, dd.eigen_vectors, K, out=out, precision=code)
        check_guards(buf, f"{case.id} {mode} phi")
        assert bool((out.view(torch.int32)[~dmask] == SENTINEL).all()), f"{case.id} {mode}: phi wrote into an invalid slot"
        written(out[dmask], f"{case.id} {mode} phi (valid slots)")
        assert torch.equal(out[dmask], st["phi_fused"][dmask]), f"{case.id} {mode}: two runs of phi differ"

        ev = dd.eigen_values if SC.has_eig_encoder(p) else None
        buf, out = guarded((N, d))
        P["rho_fused"].run(plan, st["phi_fused"].contiguous().view(N * K, d), ev, K, precision=code, out=out)
        check_guards(buf, f"{case.id} {mode} rho")
        written(out, f"{case.id} {mode} rho")
        assert torch.equal(out, st["rho_sum_fused"]), f"{case.id} {mode}: two runs of rho differ"

        # ---- sign invariance: exact in every mode
        fd = synth.batch_to(flip_columns(data, SC.seed_of(case, 2)), DEV)
        _, st_f = model(fd, return_stages=True)
        assert torch.equal(st_f["phi_fused"], st["phi_fused"]), f"{case.id} {mode}: phi changes when eigenvector columns change sign"
        assert torch.equal(model(fd), y), f"{case.id} {mode}: y changes when eigenvector columns change sign"

        # ---- the same graphs in reversed order: the rule again, per graph
        rev, perm = SC.reorder(data, list(range(B))[::-1])
        _, st_r = model(synth.batch_to(rev, DEV), return_stages=True)
    emu_r = {m: {"phi": emu[m]["phi"][perm], "rho_sum": emu[m]["rho_sum"][perm]} for m in PE.MODES}
    phi_r = st_r["phi_fused"].cpu()
    assert not bool(phi_r[~mask[perm]].any())
    hold(failures, case, br["phi"], "phi", mode, "reversed", PC.rule_ratios(phi_r, emu_r, mode, "phi", sizes[::-1], mask[perm]),
         PC.tile_ratios(phi_r, emu_r, mode, "phi", mask[perm]))
    hold(failures, case, br["rho_sum"], "rho_sum", mode, "reversed", PC.rule_ratios(st_r["rho_sum_fused"], emu_r, mode, "rho_sum", sizes[::-1]),
         PC.tile_ratios(st_r["rho_sum_fused"], emu_r, mode, "rho_sum"))

    # ---- back to the default: the bits of the forward taken before the mode was set
    model.matmul_precision = "highest"
    with torch.no_grad():
        assert torch.equal(model(dd), y_first), f"{case.id}: highest after {mode} is not the default forward"
        model.check_last()
    assert not failures, f"{case.id} [{br['phi']} | {br['rho_sum']}]: " + "; ".join(failures)


@pytest.mark.parametrize("case,mode", _params(PC.DGL))
def test_deepsigns_reduced_stage_row(case, mode):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import ops
    p = case.p
    sd, x, y32, y64 = SC.dgl_reference(case)
    emu = PC.dgl_emulations(case)
    data = SC.batch_of(case)
    sizes = list(p["sizes"])
    net = SC.build_dgl(case).to(DEV).eval()
    failures = []

    def run(batch, xin):
        ei = batch.edge_index
        g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), torch.tensor(batch.sizes))
        rec = ops.KernelTimer()
        with rec, torch.no_grad():
            y = net(g, xin.to(DEV)).clone()
        ran = {s[0] for s in rec.spans}
        assert {"sn_deepsigns_phi_f32", "sn_mlp_chain_f32"} <= ran, sorted(ran)
        return y

    y_first = run(data, x)
    net.matmul_precision = mode
    y = run(data, x)
    assert y.shape == y64.shape and bool(torch.isfinite(y).all())
    hold(failures, case, case.branch, "deepsigns y", mode, "batch order", PC.rule_ratios(y, emu, mode, "y", sizes))
    coarse(case, "deepsigns y", mode, y, emu[mode], y64)
    assert torch.equal(run(data, x), y), f"{case.id} {mode}: two runs differ"
    rev, perm = SC.reorder(data, list(range(len(sizes)))[::-1])
    emu_r = {m: emu[m][perm] for m in PE.MODES}
    hold(failures, case, case.branch, "deepsigns y", mode, "reversed", PC.rule_ratios(run(rev, x[perm]), emu_r, mode, "y", sizes[::-1]))
    net.matmul_precision = "highest"
    assert torch.equal(run(data, x), y_first), f"{case.id}: highest after {mode} is not the default forward"
    assert not failures, f"{case.id} [{case.branch}]: " + "; ".join(failures)


def test_widths_without_reduced_kernels_refuse_the_launch_and_write_nothing():
    """Every tile count outside the built sets — SignNetGNN hidden 16, 32, 48, 80, 96 (phi; rho with more than 16 slots: with fewer it
    runs the head-padded packing, whose 4 and 8 tiles are built), DeepSigns padded widths 48 and 112 — asked for `high` and `medium`
    at the stage launch, behind the property's back: the library's error, a sentinel-filled output unchanged."""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import ops, synth
    for hid in PC.REFUSED_HIDDEN:
        case = next(c for c in SC.PYG if c.name == f"gine-h{hid}-kall-rho1")
        p = case.p
        dd = synth.batch_to(SC.batch_of(case), DEV)
        model = SC.build_model(case).to(DEV).eval()
        for name in PC.REDUCED:
            with pytest.raises(ValueError, match="16-channel tiles"):
                model.matmul_precision = name
        with torch.no_grad():
            y = model(dd).clone()
            P, B, N, K = model._prep, len(p["sizes"]), sum(p["sizes"]), SC.slot_count(p)
            plan = ops.build_plan(dd.batch, dd.edge_index, B, 0, bins=True)
            x = torch.randn(N * K, hid, device=DEV)
            for code in (1, 2):
                buf, out = guarded((N, K, hid))
                with pytest.raises(RuntimeError, match="matmul precision"):
                    P["phi_fused"].run(plan, dd.eigen_vectors, K, out=out, precision=code)
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), f"hidden {hid}: the refused phi launch wrote"
                buf, out = guarded((N, hid))
                with pytest.raises(RuntimeError, match="matmul precision"):
                    P["rho_fused"].run(plan, x, None, K, precision=code, out=out)
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), f"hidden {hid}: the refused rho launch wrote"
            assert torch.equal(model(dd), y)
            model.check_last()
    for hidden in PC.REFUSED_DGL_HIDDEN:
        case = next(c for c in SC.DGL if c.name == f"gin-h{hidden}-c4-k8")
        data = SC.batch_of(case)
        x = SC.dgl_reference(case)[1].to(DEV)
        net = SC.build_dgl(case).to(DEV).eval()
        for name in PC.REDUCED:
            with pytest.raises(ValueError, match="16-channel tiles"):
                net.matmul_precision = name
        g = DS.Graph(data.edge_index[0].to(DEV), data.edge_index[1].to(DEV), torch.tensor(data.sizes))
        with torch.no_grad():
            y = net(g, x).clone()
            N, K = x.shape[0], case.p["K"]
            assert net._fused is not None and net._fused.ok
            for code in (1, 2):
                with pytest.raises(RuntimeError, match="matmul precision"):
                    net._fused.run(DS.cached_plan(g, N, K), x.view(N, K).contiguous(), N, code)
            assert torch.equal(net(g, x), y)
