"""Shared by tests/test_signinv_dropout_cpu.py and tests/test_signinv_dropout_gpu.py: the dropout sites of the DGL tree's sign-invariant
encoders restated from the reference (layers/deepsigns.py, layers/gnns.py, layers/mlp.py), the host-side path predicate of
sn_affine_dropout_f32 restated from csrc/dropout.hip, and the case tables.  Philox and keep_mask are tests/dropout_cases.py's.
Pure numpy: no GPU, no torch.

    site = SITE0 + ordinal of the F.dropout / nn.Dropout call within ONE forward of the encoder module:
           enc(g, x) first, then enc(g, -x), then rho; a call with p = 0 is no site and takes no ordinal

  gin / masked_gin   enc = GIN (gnns.py:102-114): layer 0's MLP hidden site (mlp.py:51, [N, k, hidden]); then per layer i >= 1 the inter-layer
                     site in front of its BatchNorm (gnns.py:105, [N, k, hidden]) and its MLP hidden site: 2L - 1 per call;
                     rho = MLP(.., L): L - 1 hidden sites on [N, hidden]                                                   5L - 3
  gcn                enc = GCN (gnns.py:33-45): the inter-layer site in front of every layer i >= 1: L - 1 per call; rho L - 1   3L - 3
  transformer        SetTransformerEncoder is built with dropouth = dropouta = 0: no site; rho = MLP(.., 4): 3                  3
"""
import numpy as np

import dropout_cases as DC

SITE0 = 0x53490000          # SN_SIGNINV_DROP_SITE

ENCODER_CASES = ["ds_dropout_gin_h8_c4_l3_k4", "ds_dropout_gin_h19_c3_l4_k5", "ds_dropout_masked_gin_h8_c4_l3_k6",
                 "ds_dropout_masked_gin_h7_c5_l4_k5", "ds_dropout_gcn_h8_c4_l3_k4", "ds_dropout_gcn_h19_c21_l4_k5",
                 "ds_dropout_transformer_h16_l3_k4", "ds_dropout_transformer_h14_l3_k5"]
NET_CASES = ["ds_dropout_net_gatedgcn_gin_add", "ds_dropout_net_transformer_masked_gin_concat"]
NET_SIGN_INV_LAYERS = 3     # (make_dropout_deepsigns.NET_COMMON)
NET_PHI_OUT = 4
CLASSES = {"gin": "GINDeepSigns", "masked_gin": "MaskedGINDeepSigns", "gcn": "GCNDeepSigns", "transformer": "TransformerDeepSigns"}


# name -> (net class, its parameters beyond NET_COMMON): make_dropout_deepsigns.NETS restated
NET_COMMON = dict(num_atom_type=28, num_bond_type=4, batch_norm=True, residual=True, edge_feat=True,
                  pe_init="lap_pe", lap_method="sign_inv", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4,
                  sign_inv_layers=NET_SIGN_INV_LAYERS, sign_inv_activation="relu", phi_out_dim=NET_PHI_OUT)
NETS = {
    "ds_dropout_net_gatedgcn_gin_add": ("GatedGCNNet", "gatedgcn", dict(hidden_dim=12, out_dim=12, L=2, pos_enc_dim=4, readout="mean",
                                                                         sign_inv_net="gin", pe_aggregate="add")),
    "ds_dropout_net_transformer_masked_gin_concat": ("TransformerNet", "transformer",
                                                     dict(hidden_dim=16, out_dim=16, L=2, pos_enc_dim=5, n_heads=4, full_graph=False,
                                                          readout="sum", layer_norm=True, sign_inv_net="masked_gin",
                                                          pe_aggregate="concat")),
}


def net_params(name, device, dropout):
    cls, family, extra = NETS[name]
    return cls, family, dict(NET_COMMON, **extra, device=device, dropout=dropout, in_feat_dropout=dropout)


def site_count(kind, L):
    return {"gin": 5 * L - 3, "masked_gin": 5 * L - 3, "gcn": 3 * L - 3, "transformer": 3}[kind]


def site_table(kind, N, hidden, L, k):
    """[(site, R, C, post_bn)] of one forward, in call order: the logical row-major shape [R, C] of the reference tensor and whether a
    BatchNorm directly precedes the dropout (use_bn = True, as get_sign_inv_net builds every encoder) — the sites that are one launch
    with the BatchNorm apply."""
    out = []
    if kind in ("gin", "masked_gin"):
        for _ in (0, 1):
            out.append((N * k, hidden, True))                 # layer 0: MLP hidden
            for _i in range(1, L):
                out.append((N * k, hidden, False))            # in front of layer i's BatchNorm
                out.append((N * k, hidden, True))             # layer i: MLP hidden
        out += [(N, hidden, True)] * (L - 1)
    elif kind == "gcn":
        for _ in (0, 1):
            out += [(N * k, hidden, False)] * (L - 1)
        out += [(N, hidden, True)] * (L - 1)
    elif kind == "transformer":
        out += [(N, hidden, True)] * 3
    else:
        raise KeyError(kind)
    assert len(out) == site_count(kind, L)
    return [(SITE0 + s, R, C, bn) for s, (R, C, bn) in enumerate(out)]


def fused_sites(kind, L):
    """How many sites of one forward directly follow a BatchNorm: 3L - 1 for the GIN encoders, rho's alone otherwise."""
    return sum(1 for t in site_table(kind, 1, 1, L, 1) if t[3])


def masks(table, p, seed, step):
    return [DC.keep_mask(R, C, p, seed, step, site) for site, R, C, _ in table]


def unpack(bits, shape):
    n = int(shape[0]) * int(shape[1])
    return np.unpackbits(np.asarray(bits))[:n].reshape(int(shape[0]), int(shape[1])).astype(bool)


# ----------------------------------------------------------------------------- dispatch of sn_affine_dropout_f32, restated
MAX_BLOCKS = DC.MAX_BLOCKS


def path(C, ldx, ldy, base, x_ptr, y_ptr, scale_ptr=0, shift_ptr=0):
    """'row' / 'flat' / 'scalar': the kernel the host picks (pointers as byte addresses; 0 for scale / shift = NULL)."""
    aligned = x_ptr % 16 == 0 and y_ptr % 16 == 0 and base % 4 == 0
    if aligned and C % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and scale_ptr % 16 == 0 and shift_ptr % 16 == 0:
        return "row"
    if aligned and ldx == C and ldy == C:
        return "flat"
    return "scalar"


def n_groups(R, C, base, which):
    total = R * C
    if total == 0:
        return 0
    return {"row": total // 4, "flat": (total + 3) // 4, "scalar": ((base + total - 1) >> 2) - (base >> 2) + 1}[which]


# (C, ldx, ldy, base, x, y, scale, shift) -> path: every clause of each predicate falsified alone
PATH_TABLE = [
    ((68, 68, 68, 0, 0, 0, 0, 0), "row"),
    ((68, 72, 76, 8, 16, 32, 48, 64), "row"),                # strided rows stay on the row path
    ((67, 67, 67, 0, 0, 0, 0, 0), "flat"),                   # C % 4 != 0, contiguous
    ((68, 68, 68, 0, 0, 0, 4, 0), "flat"),                   # scale not 16-byte aligned, contiguous
    ((68, 68, 68, 0, 0, 0, 0, 4), "flat"),                   # shift likewise
    ((68, 70, 72, 0, 0, 0, 0, 0), "scalar"),                 # ldx % 4 != 0 (and not contiguous)
    ((68, 72, 70, 0, 0, 0, 0, 0), "scalar"),                 # ldy % 4 != 0
    ((68, 72, 72, 0, 0, 0, 4, 0), "scalar"),                 # scale misaligned and strided
    ((68, 68, 68, 3, 0, 0, 0, 0), "scalar"),                 # base % 4 != 0
    ((68, 68, 68, 0, 4, 0, 0, 0), "scalar"),                 # x 4 bytes off
    ((68, 68, 68, 0, 0, 4, 0, 0), "scalar"),                 # y 4 bytes off
    ((67, 67, 67, 2, 0, 0, 0, 0), "scalar"),                 # flat: base % 4 != 0
    ((67, 67, 67, 0, 8, 0, 0, 0), "scalar"),                 # flat: x misaligned
    ((67, 67, 67, 0, 0, 12, 0, 0), "scalar"),                # flat: y misaligned
    ((67, 68, 67, 0, 0, 0, 0, 0), "scalar"),                 # flat: ldx != C
    ((67, 67, 71, 0, 0, 0, 0, 0), "scalar"),                 # flat: ldy != C
    ((1, 1, 1, 0, 0, 0, 0, 0), "flat"),
    ((4, 4, 4, 1 << 34, 0, 0, 0, 0), "row"),
]

# ----------------------------------------------------------------------------- kernel cases of the GPU test
SHAPES = [(1, 1, None), (3, 5, None), (7, 4, None), (37 * 3, 67, None), (33, 77, None), (5, 68, 72), (0, 8, None)]
PS = [0.1, 0.5, 0.9]
BASES = [0, 3, (1 << 34) - 6]
K_MASK = 3                   # rows are (node, slot) with 3 slots; nvalid cycles through 0..3
SEED, STEP, SITE = 0x0FED_CBA9_8765_4321, 17, SITE0 + 5
BIG = (2049, 1024)           # 2049 * 256 row groups > MAX_BLOCKS * 256: the grid's second pass
BIG_FLAT = (2049, 1025)      # the same on the flat path (an odd width)


def nvalid_for(R, K=K_MASK):
    """int32 [ceil(R / K)]: 0, 1, 2, 3, 0, ... valid slots per node."""
    return (np.arange((R + K - 1) // K) % (K + 1)).astype(np.int32)


def rowvalid(R, nvalid, K=K_MASK):
    r = np.arange(R)
    return (r % K) < nvalid[r // K] if R else np.zeros(0, bool)
