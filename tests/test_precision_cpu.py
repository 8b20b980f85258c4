"""Matmul precision of the fused eval stages, the parts that need no GPU: the Python surface (`matmul_precision`), the C ABI names,
and the CPU emulation of the three product sets (tests/precision_emulation.py) held against its derived bounds."""
import os
import re

import pytest
import torch

import precision_emulation as PE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC_ENTRY_POINTS = ("sn_phi_fused_prec_f32", "sn_rho_fused_prec_f32", "sn_deepsigns_phi_prec_f32", "sn_mlp_chain_prec_f32")


def _modules():
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd.pyg import SignNetGNN
    return [SignNetGNN(None, None, 64, 1, 2, 2, variant="gine", max_k=8),
            SignNetGNN(6, 4, 108, 12, 2, 2, variant="alchemy"),
            DS.GINDeepSigns(1, 64, 4, 8, 16, use_bn=True, dropout=0.0),
            DS.MaskedGINDeepSigns(1, 67, 67, 8, 37, None, use_bn=True, dropout=0.0)]


def test_matmul_precision_property():
    for m in _modules():
        assert m.matmul_precision == "highest", type(m).__name__
        for name in ("high", "medium", "highest"):
            m.matmul_precision = name
            assert m.matmul_precision == name
        for bad in ("bf16", "HIGH", "", None, 1):
            with pytest.raises(ValueError):
                m.matmul_precision = bad
            assert m.matmul_precision == "highest", "a refused value leaves the mode as it was"


def test_matmul_precision_is_not_module_state():
    """Constructor signatures stay the reference's and the option is not a parameter or buffer: state_dicts are unchanged."""
    for m in _modules():
        keys = list(m.state_dict().keys())
        m.matmul_precision = "medium"
        assert list(m.state_dict().keys()) == keys


def test_reduced_mode_is_refused_at_other_widths():
    """The reduced modes are built for the shipped widths; elsewhere they are refused, never replaced by another mode."""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd.pyg import SignNetGNN
    for m in (SignNetGNN(None, None, 32, 1, 2, 2, variant="gine", max_k=8), SignNetGNN(None, None, 96, 1, 2, 2, variant="gine"),
              DS.GINDeepSigns(1, 40, 4, 8, 8, use_bn=True, dropout=0.0), DS.GINDeepSigns(1, 112, 4, 8, 8, use_bn=True, dropout=0.0)):
        for name in ("high", "medium"):
            with pytest.raises(ValueError, match="16-channel tiles"):
                m.matmul_precision = name
        m.matmul_precision = "highest"
        assert m.matmul_precision == "highest"


def test_prec_entry_points_are_declared_and_bound():
    """Header and ctypes table carry the four *_prec_f32 names (tests/test_abi.py then holds the two lists to each other); each takes
    its neighbour's arguments with `int precision` in front of the stream."""
    import ctypes as C
    from signnet_basisnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "signnet_hip.h")).read()
    for name in PREC_ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/signnet_hip.h"
        assert re.search(r"int\s+precision\s*,\s*void\s*\*\s*stream\s*$", m.group(1).strip()), f"{name}: ..., int precision, void* stream)"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        base = _lib.SIGNATURES[name.replace("_prec_f32", "_f32")]
        assert _lib.SIGNATURES[name] == base[:-1] + [C.c_int, base[-1]]
    assert re.search(r"#define\s+SN_ABI_VERSION\s+3\b", hdr), "the ABI version is 3 since the in-launch finishes of the training links were removed"
    for k, v in (("HIGHEST", 0), ("HIGH", 1), ("MEDIUM", 2)):
        assert re.search(rf"#define\s+SN_PREC_{k}\s+{v}\b", hdr)
    from signnet_basisnet_amd import fused
    assert fused.PRECISIONS == {"highest": 0, "high": 1, "medium": 2}


def test_planes_are_an_exact_bf16_split():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g) * torch.logspace(-6, 6, 4096)
    h, m, l = PE.planes(x)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    for p in (h, m, l):
        assert torch.equal(p.to(torch.bfloat16).float(), p), "every plane is a bf16 value"
    hn, mn, ln = PE.planes(-x)
    assert torch.equal(hn, -h) and torch.equal(mn, -m) and torch.equal(ln, -l), "truncation is symmetric in the sign"
    assert bool(((x - h).abs() < 2.0 ** -7 * x.abs()).all()) and bool((l.abs() < 2.0 ** -15 * x.abs()).all())


def test_emulation_meets_its_derived_bounds():
    """[512, 128] x [128, 128], seeded: every mode within its derived bound of the float64 product, elementwise; errors strictly ordered."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(512, 128, generator=g)
    w = torch.randn(128, 128, generator=g) / 128 ** 0.5
    y64 = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    worst = {}
    for mode in PE.MODES:
        e = (PE.emu_mm(x, w, mode) - y64).abs() / mag
        worst[mode] = e.max().item()
        print(f"emu_mm {mode}: worst |err| / mag = {worst[mode]:.3e} (bound {PE.C_MODE[mode]:.3e})")
        assert bool((e <= PE.C_MODE[mode]).all()), (mode, worst[mode])
    assert PE.C_MODE == {"highest": 2.0 ** -21, "high": 2.0 ** -13, "medium": 2.0 ** -6 + 2.0 ** -14}
    assert worst["highest"] < worst["high"] < worst["medium"]
