"""readout='max' (DESIGN.md §4.6a): the shape table of the kernel tests, the float64 restatement of sn_segment_max_f32 /
sn_segment_max_bwd_f32 with their tie, NaN and empty-graph rules, and the fixture helpers shared by tests/test_readout_max_cpu.py and
tests/test_readout_max_gpu.py."""
import json

import torch

import golden_util as G

# segment sizes {0, 1, 2, 15, 16, 17, 64, 65, 300, 2100}: 0 in first, middle and last position; 2100 is past the eight-deep unroll at
# every row-lane count (8 x 256 rows at C = 1)
SIZE_LISTS = [[0, 1, 2, 15, 16, 0, 17, 64, 65, 300, 0], [2100, 0, 17]]
# scalar and vector paths, every column-lane count, a second blockIdx.y chunk (260); 77 and 95 are shipped out_dim values
WIDTHS = [1, 3, 4, 64, 77, 95, 128, 260]
TIE_SIZES = [17, 65, 300]

FIXTURES = ["readout_max_gin", "readout_max_gatedgcn", "readout_max_pna", "readout_max_transformer", "readout_max_gat",
            "readout_max_gatedgcn_signinv", "readout_max_transformer_full"]
CLS = {"gin": "GINNet", "gatedgcn": "GatedGCNNet", "pna": "PNANet", "transformer": "TransformerNet", "gat": "GATNet"}
MIN_GAP = 1e-3          # 100 x the 1e-5 forward tolerance: below it a float32 rounding could hand the gradient to another node


def graph_ptr(sizes):
    return torch.tensor([0] + list(sizes), dtype=torch.int64).cumsum(0).to(torch.int32)


def segment_max_ref(x, sizes):
    """-> (out [B, C] float64, arg [B, C] int32): per graph and channel the maximum of the graph's rows and the LOWEST row that attains
    it; a NaN among the rows gives NaN and the first NaN row; a graph without rows gives 0 and -1."""
    x = x.detach().cpu().double()
    C = x.shape[1]
    out = torch.zeros(len(sizes), C, dtype=torch.float64)
    arg = torch.full((len(sizes), C), -1, dtype=torch.int64)
    r = 0
    for b, n in enumerate(sizes):
        if n == 0:
            continue
        blk = x[r:r + n]
        rows = torch.arange(n).reshape(n, 1).expand(n, C)
        nan = torch.isnan(blk)
        clean = torch.where(nan, torch.full_like(blk, float("-inf")), blk)
        m = clean.max(0).values
        first_max = torch.where(clean == m, rows, torch.full_like(rows, n)).min(0).values
        first_nan = torch.where(nan, rows, torch.full_like(rows, n)).min(0).values
        has_nan = nan.any(0)
        out[b] = torch.where(has_nan, torch.full_like(m, float("nan")), m)
        arg[b] = r + torch.where(has_nan, first_nan, first_max)
        r += n
    return out, arg.to(torch.int32)


def segment_max_bwd_ref(dy, arg, sizes, N):
    """dx [N, C] float64: dy[g, c] at row arg[g, c], zero at every other row."""
    dy = dy.detach().cpu().double()
    dx = torch.zeros(N, dy.shape[1], dtype=torch.float64)
    cols = torch.arange(dy.shape[1])
    for b, n in enumerate(sizes):
        if n:
            dx[arg[b].long(), cols] = dy[b]
    return dx


def grid_input(sizes, C, seed):
    """[N, C] float32 multiples of 2^-8 drawn from a range wide enough that most maxima are unique and a few tie."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4096, 4097, (sum(sizes), C), generator=g).float() / 256.0


# ----------------------------------------------------------------------------- the fixtures (tests/golden/make_readout_max.py)
def fixture(name):
    return G.load(name)


def net_params(fx, device="cpu", **over):
    p = json.loads(str(fx.meta["net_params"]))
    p.update(device=device, **over)
    return p


def build(name, device="cpu", module=None, **over):
    """(fixture, the readout_models net — or `module`'s — with the fixture's parameters and state_dict)"""
    from signnet_basisnet_amd import readout_models
    fx = fixture(name)
    net = getattr(module or readout_models, CLS[str(fx.meta["net"])])(net_params(fx, device, **over))
    net.load_state_dict(fx.sd, strict=True)
    return fx, net.to(device)
