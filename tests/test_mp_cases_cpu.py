"""No GPU: the conditions under which the message-passing grid (tests/test_mp_grid_gpu.py) can tell a right kernel of
csrc/dgl_layers.hip from a wrong one, checked on every row of every table of tests/mp_cases.py.

  graphs        the facts the rows rely on: nodes without in-edges and without out-edges, the hub's in-degree, duplicate edges, self
                loops, an edge list that is neither symmetric nor sorted — and that the molecule batch is none of that
  branch        the host restatement of the dispatch returns the row's `branch`, and the rows of an op reach every kernel instance
  conditioning  the float32 restatement's forward is within parity_util.REL of float64 (the PNA std columns, which cancel in fp32:
                within the bound that the existing forward test derives for them)
  decisions     (float64) attention scores stay MARGIN * rms off +-5, with at least 5 % of them clamped at scale 3 and at most 1 % at
                scale 1; GAT logits stay MARGIN * rms off zero; the GAT cotangent is zero where the output before the ReLU is within
                MARGIN * rms of zero, on at most 1 % of the elements; PNA maxima / minima are MARGIN * rms(msg) clear of the runner-up,
                or — `ties` rows — attained by bit-identical rows, on at least 20 (node, channel) pairs each
  cotangents    the two PNA cotangents split the columns: one zero on the three std blocks, one non-zero only there

Run with -s to see the seeds, the clamped shares and the tie counts.
"""
import pytest
import torch

import adjoint_cases as AC
import mp_cases as MP
import parity_util as PU


def ids(rows):
    return [r.id for r in rows]


# ---------------------------------------------------------------------------- graphs
def test_topology_batch_has_the_hazards_the_rows_name():
    g = MP.graph("topo")
    f = MP.graph_facts(g)
    print(f"\ntopology batch: {f}", end="")
    for k, v in MP.TOPOLOGY_FACTS.items():
        assert f[k] == v, (k, f[k], v)
    assert f["duplicates"] >= 7 and f["self_loops"] >= 9 and f["directed_only"] > 0 and not f["sorted"]
    # the in-edge CSR and the CSR of the flipped list differ in their degree sequence: a mix-up of the two cannot go unnoticed
    assert not torch.equal(g.deg_in, g.deg_out)
    assert int(g.deg_in.max()) > 32                                # more in-edges than any register array of the kernels is long
    # the mailbox is the edge list grouped by destination in edge-id order
    for n in (0, int(g.deg_in.argmax()), g.N - 1):
        assert g.mail[n][g.mail[n] >= 0].tolist() == (g.dst == n).nonzero()[:, 0].tolist()


def test_molecule_batch_is_the_ordinary_case():
    f = MP.graph_facts(MP.graph("mol"))
    print(f"\nmolecule batch: {f}", end="")
    assert f["zero_in"] == 0 and f["zero_out"] == 0 and f["duplicates"] == 0 and f["self_loops"] == 0 and f["directed_only"] == 0
    assert 2 <= f["max_in"] <= 9 and f["N"] < MP.TOPOLOGY_FACTS["N"]


# ---------------------------------------------------------------------------- tables
def test_ids_are_unique():
    i = ids(MP.ALL)
    assert len(i) == len(set(i)), sorted(x for x in i if i.count(x) > 1)


@pytest.mark.parametrize("row", MP.ALL, ids=ids(MP.ALL))
def test_row_takes_the_branch_it_names_and_states_its_hazard(row):
    assert MP.OPS[row.op].predicate(row.p) == row.branch
    assert row.hazard


@pytest.mark.parametrize("name", sorted(MP.OPS))
def test_rows_cover_every_kernel_instance(name):
    op = MP.OPS[name]
    seen = {b for r in op.cases for b in r.branch.split(" | ")}
    assert seen == op.branches, f"{name}: not reached {sorted(op.branches - seen)}, not declared {sorted(seen - op.branches)}"
    assert {r.p["graph"] for r in op.cases} == {"topo", "mol"}


def test_the_kernels_the_grid_was_written_for_are_all_in_the_tables():
    seen = {b for r in MP.ALL for b in r.branch.split(" | ")}
    want = {"k_pna_aggregate", "k_pna_aggregate_bwd", "k_pna_aggregate_gather", "k_edge_attention", "k_edge_attention strided",
            "k_edge_attention_bwd_dst", "k_edge_attention_bwd_src", "k_gat_aggregate_wave<1>", "k_gat_aggregate_wave<2>", "k_gat_bwd_dst<64>",
            "k_gat_bwd_src<64>", "k_gat_bwd_dst<128>", "k_gat_bwd_src<128>", "k_edge_rows_sum plan", "k_edge_rows_sum flipped plan"}
    assert want <= seen, sorted(want - seen)


def test_the_tables_hold_the_shapes_the_grid_was_written_for():
    def have(rows, *keys):
        return {tuple(r.p[k] for k in keys) for r in rows if r.p["graph"] == "topo"}
    assert have(MP.PNA, "C", "hself") == {(C, h) for C in (1, 14, 70) for h in (True, False)}
    assert any(r.p["ldm"] and r.p["ldm"] > r.p["C"] for r in MP.PNA) and any(r.p["ties"] for r in MP.PNA)
    assert {(0, None), (4, None)} <= have(MP.PNA_GATHER, "tower", "qe_layer") and any(r.p["tower"] and r.p["qe_layer"] is not None for r in MP.PNA_GATHER)
    assert have(MP.EDGE_ATTENTION, "H", "dk", "scale", "layer") >= ({(H, dk, s, None) for H, dk in MP.HEAD_SHAPES for s in (1, 3)} |
                                                                    {(H, dk, 1, 0) for H, dk in MP.HEAD_SHAPES} |
                                                                    {(H, dk, 3, MP.L_FUSED - 1) for H, dk in MP.HEAD_SHAPES})
    assert set(MP.HEAD_SHAPES) == {(4, 6), (2, 32), (3, 1), (8, 8)} and MP.L_FUSED == 3
    assert have(MP.GAT, "H", "C", "relu", "bias") == {(H, C, r, b) for H, C in ((4, 12), (3, 64), (2, 65), (1, 128), (3, 1))
                                                      for r in (True, False) for b in (True, False)}
    assert have(MP.GATHER_ROWS, "C", "side") == {(C, s) for C in (1, 10, 70) for s in ("dst", "src")}


# ---------------------------------------------------------------------------- every row
@pytest.mark.parametrize("row", MP.ALL, ids=ids(MP.ALL))
def test_float32_restatement_forward_is_within_rel_of_float64(row):
    (o32, g32), (o64, g64) = MP.references(row)
    _, aux = MP.inputs(row)
    assert set(g32) == set(g64) == set(aux["cots"])
    for i, (a32, a64) in enumerate(zip(o32, o64)):
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and bool(torch.isfinite(a64).all())
        if row.op in ("pna", "pna_gather"):          # the std columns cancel in fp32: held to the bound derived for them, the rest to REL
            std, bound = MP.pna_std(row)
            assert bool(((a32.double() - a64)[:, std].abs() <= bound).all()), f"{row.id} std columns"
            a32, a64 = a32[:, ~std], a64[:, ~std]
        scale = a64.abs().max().item()
        err = (a32.double() - a64).abs().max().item()
        assert err <= PU.REL * scale, f"{row.id} output {i}: |cpu32 - f64| {err / scale:.2e} of max|f64| {scale:.3e}"
    for name in g64:
        for a32, a64 in zip(g32[name], g64[name]):
            assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and bool(torch.isfinite(a64).all()) and bool(torch.isfinite(a32).all())


@pytest.mark.parametrize("row", MP.PNA, ids=ids(MP.PNA))
def test_pna_extrema_are_clear_of_the_runner_up_or_exactly_tied(row):
    p = row.p
    (msg, *_), aux = MP.inputs(row)
    g = aux["g"]
    m = MP.pna_margins(g, msg)
    print(f"\n{row.id}: {m}", end="")
    assert m["gap_max"] >= AC.MARGIN and m["gap_min"] >= AC.MARGIN
    c0 = aux["c0"]
    assert torch.equal(aux["wide"][:, c0:c0 + p["C"]], msg) and aux["wide"].shape[1] == (p["ldm"] or p["C"])
    if not p["ties"]:
        assert m["ties_max"] == 0 and m["ties_min"] == 0
        return
    assert m["ties_max"] >= 20 and m["ties_min"] >= 20
    groups = MP.tie_groups(g)
    assert len(groups) >= 8 and max(len(x) for x in groups) == 13             # the duplicate edges, and a third of the hub's 39 in-edges
    for grp in groups:
        assert bool((msg[grp] == msg[grp[0]]).all())               # bit-identical in fp32
    # the float64 reference routes a tied maximum to the FIRST in-edge in edge order, whole — what the kernel's `v > mx` does
    hub = int(g.deg_in.argmax())
    first, *rest = groups[-1]
    dmsg = MP.references(row)[1][1]["std-free"][0]
    W = MP.pna_width(p["C"], p["hself"])
    cot = aux["cots"]["std-free"][0][hub]
    off = p["C"] if p["hself"] else 0
    D = float(g.deg_in[hub])
    amp, att = torch.log(torch.tensor(D + 1, dtype=AC.F64)) / MP.AVG_LOG, MP.AVG_LOG / torch.log(torch.tensor(D + 1, dtype=AC.F64))
    da = lambda a, c: cot[off + a * p["C"] + c] + cot[off + (4 + a) * p["C"] + c] * amp + cot[off + (8 + a) * p["C"] + c] * att   # noqa: E731
    assert len(cot) == W
    for c in range(0, p["C"], 3):                                  # channels where the shared row is the hub's maximum
        assert abs(float(dmsg[first, c]) - float(da(0, c) / D + da(1, c))) <= 1e-12 * (1 + abs(float(da(1, c))))
        for e in rest:
            assert abs(float(dmsg[e, c]) - float(da(0, c) / D)) <= 1e-12


@pytest.mark.parametrize("row", MP.PNA, ids=ids(MP.PNA))
def test_pna_cotangents_split_the_std_blocks(row):
    p = row.p
    _, aux = MP.inputs(row)
    std = MP.std_columns(p["C"], p["hself"])
    free, only = aux["cots"]["std-free"][0], aux["cots"]["std-only"][0]
    assert int(std.sum()) == 3 * p["C"]
    assert not bool(free[:, std].any()) and bool((free[:, ~std] != 0).all())
    assert not bool(only[:, ~std].any()) and bool((only[:, std] != 0).all())
    # the std blocks are where the restatement's columns are sqrt(relu(E[x^2] - E[x]^2) + 1e-5): at least sqrt(1e-5) on a node with in-edges
    out = MP.references(row)[1][0][0]
    has = aux["g"].deg_in > 0
    assert bool((out[has][:, std][:, :p["C"]] >= 1e-5 ** 0.5 * (1 - 1e-12)).all()) and not bool(out[~has][:, std].any())


@pytest.mark.parametrize("row", MP.PNA_GATHER, ids=ids(MP.PNA_GATHER))
def test_pna_gather_layout(row):
    p = row.p
    leaves, aux = MP.inputs(row)
    C, it = p["C"], p["tower"]
    assert aux["qe_all"].shape[1] == (1 if p["qe_layer"] is None else MP.L_FUSED) * C
    lay = p["qe_layer"] or 0
    assert torch.equal(aux["qe_all"][:, lay * C:(lay + 1) * C], leaves[1])
    out = MP.references(row)[1][0][0]
    std, bound = MP.pna_std(row)
    assert int(std.sum()) == 3 * C and bound.shape == (aux["g"].N, 3 * C)
    # the std columns are where the restatement has sqrt(relu(E[x^2] - E[x]^2) + 1e-5) times a scaler that is 1 for a third of them
    has = aux["g"].deg_in > 0
    assert bool((out[has][:, std] > 0).all()) and int((out[has][:, std] < 1e-5 ** 0.5 * (1 - 1e-12)).sum()) <= int(has.sum()) * C
    if it:          # tower t owns 13 * it contiguous columns, its own it channels of hself first
        assert C % it == 0
        for t in range(C // it):
            assert torch.equal(out[:, t * 13 * it:t * 13 * it + it], leaves[2].double()[:, t * it:(t + 1) * it])
    else:
        assert torch.equal(out[:, :C], leaves[2].double())


@pytest.mark.parametrize("row", MP.EDGE_ATTENTION, ids=ids(MP.EDGE_ATTENTION))
def test_attention_scores_are_off_the_clamp_and_the_clamp_is_exercised(row):
    p = row.p
    (Q, K, V, Ee), aux = MP.inputs(row)
    margin, share = MP.clamp_stats(aux["g"], p["H"], Q, K, Ee)
    print(f"\n{row.id}: {100 * share:.2f} % of the scores clamped, nearest to +-5 at {margin:.2e} rms", end="")
    assert margin >= AC.MARGIN
    if p["scale"] == 3:
        assert share >= 0.05
    else:
        assert p["scale"] == 1 and share <= 0.01
    assert aux["other"].shape == (aux["g"].E, MP.L_FUSED * p["H"] * p["dk"])


@pytest.mark.parametrize("row", MP.GAT, ids=ids(MP.GAT))
def test_gat_logits_are_off_the_kink_and_the_relu_decisions_carry_no_cotangent(row):
    p = row.p
    leaves, aux = MP.inputs(row)
    g = aux["g"]
    feat, al, ar = (t.double() for t in leaves[:3])
    b = leaves[3].double() if p["bias"] else None
    pre, out = MP.gat_parts(g, p["H"], p["relu"], feat, al, ar, b)
    m = MP.logit_margin(pre)
    share = aux["near"].double().mean().item()
    print(f"\n{row.id}: seed {aux['seed']} (try {aux['seed'] - MP.GAT_SEED0 - 1000 * (p['H'] * 131 + p['C']) + 1} of {MP.GAT_TRIES}), "
          f"min |logit| {m:.2e} rms, cotangent zeroed on {100 * share:.3f} % of the outputs", end="")
    assert m >= AC.MARGIN
    cot = aux["cots"][""][0]
    if p["relu"]:
        rms = out.pow(2).mean().sqrt()
        near = (out.abs() < AC.MARGIN * rms) & (out != 0)
        assert torch.equal(near, aux["near"]) and not bool(cot[near].any()) and bool((cot[~near] != 0).all())
        assert share <= 0.01
        # exact zeros before the ReLU are the nodes without in-edges of a row without bias, nothing else
        zero_rows = (out == 0).all(1)
        assert bool((out == 0).sum() == zero_rows.sum() * out.shape[1])
        assert torch.equal(zero_rows, (g.deg_in == 0) if not p["bias"] else torch.zeros(g.N, dtype=torch.bool))
    else:
        assert share == 0 and bool((cot != 0).all())
    # a node without in-edges gets the bias
    lone = g.deg_in == 0
    if bool(lone.any()):
        want = b if p["bias"] else torch.zeros(p["H"] * p["C"], dtype=AC.F64)
        assert torch.equal(out[lone], want[None, :].expand(int(lone.sum()), -1))


@pytest.mark.parametrize("row", MP.GATHER_ROWS, ids=ids(MP.GATHER_ROWS))
def test_gather_rows_adjoint_is_the_degree_weighted_sum(row):
    p = row.p
    _, aux = MP.inputs(row)
    g = aux["g"]
    dh = MP.references(row)[1][1][""][0]
    deg = g.deg_in if p["side"] == "dst" else g.deg_out
    assert not bool(dh[deg == 0].any()) and bool((dh[deg > 0] != 0).all())


# ---------------------------------------------------------------------------- the restatements against the oracle's
def test_restatements_agree_with_the_oracle_where_the_oracle_is_defined():
    """oracle.dgl_nets restates the same ops for the nets' goldens (scatter-based: no rule for ties, no node without in-edges in its
    fixtures): in float64, on rows without ties, the two restatements are the same function."""
    from oracle import dgl_nets as ON
    for row in MP.PNA:
        if row.p["ties"] or row.p["hself"]:
            continue
        (msg,), aux = MP.inputs(row)
        g = aux["g"]
        ref = ON.pna_aggregate(msg.double(), g.dst, g.N, MP.AVG_LOG)
        has = g.deg_in > 0
        assert (MP.references(row)[1][0][0] - ref)[has].abs().max().item() <= 1e-12 * ref.abs().max().item(), row.id
    for row in MP.GAT:
        p = row.p
        if not (p["relu"] and p["bias"]):
            continue
        (feat, al, ar, b), aux = MP.inputs(row)
        g = aux["g"]
        sd = {"l.fc.weight": torch.eye(p["H"] * p["C"], dtype=AC.F64), "l.attn_l": al.double(), "l.attn_r": ar.double(), "l.bias": b.double()}
        ref = ON.gat_conv(sd, "l", g.src, g.dst, feat.double(), p["H"]).flatten(1)
        has = g.deg_in > 0
        assert (MP.references(row)[1][0][0] - ref)[has].abs().max().item() <= 1e-12 * ref.abs().max().item(), row.id
