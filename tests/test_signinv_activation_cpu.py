"""CPU: `--sign_inv_activation tanh | elu`.  The float64 restatements of tests/signinv_activation_cases.py — and
oracle.dgl_deepsigns for the two GIN encoders — reproduce every tests/golden/ds_act_*.npz fixture (the reference's own modules); the new
classes refuse what the reference refuses, with its exceptions, and the old ones what they refused before; state_dict keys, the drop-in
table and runner flag, the header's constants and the host-side argument checks of the two entry points."""
import functools
import os
import re

import pytest
import torch

import golden_util as G
import signinv_activation_cases as AC
from parity_util import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_REL = 1e-9          # a float64 restatement against the reference's float64 rerun: different summation orders only


@functools.lru_cache(maxsize=None)
def fixture(name):
    return G.load(name)


def _grad_close(got, fx, what):
    """Every gradient against the reference's float64 rerun; a gradient that is zero in exact arithmetic (a bias in front of a train-mode
    BatchNorm: ~1e-18 in float64) is measured against the model's largest gradient entry, as the generator's margin is."""
    g64 = {k[len("grad64/"):]: v for k, v in fx.out.items() if k.startswith("grad64/")}
    assert set(got) == set(g64), sorted(set(got) ^ set(g64))
    top = max(float(v.abs().max()) for v in g64.values())
    for k in sorted(g64):
        scale = float(g64[k].abs().max())
        if scale < 1e-9 * top:
            scale = top
        err = float((got[k].double() - g64[k]).abs().max())
        assert err <= F64_REL * scale, f"{what}: d {k}: {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("name", AC.ENCODER_CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    fx = fixture(name)
    assert float(fx.meta["margin"]) <= 1e-5, "the generator refuses a fixture whose own float32 run is farther than 1e-5 from float64"
    y = AC.module_ref(fx, torch.float64)
    close(y, fx.out["eval/y"], f"{name}: eval y")
    buffers = {}
    yt = AC.module_ref(fx, torch.float64, training=True, buffers=buffers)
    close(yt, fx.out["train/y"], f"{name}: train y")
    close(yt, fx.out["train/y64"], f"{name}: train y (float64)", rel=F64_REL)
    n = 0
    for key, ref in fx.out.items():
        if key.startswith("train/buffers/"):
            k = key[len("train/buffers/"):]
            n += 1
            if k.endswith("num_batches_tracked"):
                assert int(buffers[k]) == int(ref), k
            else:
                close(buffers[k], ref, f"{name}: {k}")
    assert n
    _, grads = AC.module_ref(fx, torch.float64, training=True, grads=True)
    _grad_close(grads, fx, name)
    # and the float32 restatement lies where the reference's float32 run lies
    close(AC.module_ref(fx, torch.float32, training=True), fx.out["train/y"], f"{name}: train y (float32 restatement)", ref64=fx.out["train/y64"])


@pytest.mark.parametrize("name", AC.ENCODER_CASES[:2])
def test_oracle_reproduces_the_gin_fixtures(name):
    from oracle import dgl_deepsigns as OD
    fx = fixture(name)
    p = AC.params(fx)
    ei = fx.inp["edge_index"]
    x = fx.inp["pos_enc"].double().unsqueeze(-1)

    def run(sd, training):
        if p.kind == "gin":
            return OD.gin_deepsigns(sd, ei[0], ei[1], x, p.layers, p.k, activation=p.act, training=training)
        return OD.masked_gin_deepsigns(sd, ei[0], ei[1], fx.inp["sizes"], x, p.layers, p.k, activation=p.act, training=training)
    sd = AC._sd(fx, torch.float64, False)
    close(run(sd, False), fx.out["eval/y"], f"{name}: oracle eval y")
    close(run(sd, True), fx.out["train/y"], f"{name}: oracle train y")
    close(run(sd, True), fx.out["train/y64"], f"{name}: oracle train y (float64)", rel=F64_REL)
    sd = AC._sd(fx, torch.float64, True)
    (run(sd, True) * fx.inp["cotangent"].double()).sum().backward()
    _grad_close({k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}, fx, f"{name}: oracle")


def test_float64_restatement_reproduces_the_net_fixture():
    fx = fixture(AC.NET_CASE)
    assert float(fx.meta["margin"]) <= 1e-5
    close(AC.net_ref(fx, torch.float64), fx.out["eval/y"], "net: eval y")
    yt, grads = AC.net_ref(fx, torch.float64, training=True, grads=True)
    close(yt, fx.out["train/y"], "net: train y")
    close(yt, fx.out["train/y64"], "net: train y (float64)", rel=F64_REL)
    _grad_close(grads, fx, "net")
    assert any(k.startswith("sign_inv_net.") for k in grads)


# ----------------------------------------------------------------------------- refusals
def _args(kind, device="cpu"):
    return (1, 8, 4, 3, 4) + ((device,) if kind == "masked_gin" else ())


@pytest.mark.parametrize("kind", list(AC.CLASSES))
def test_base_classes_refuse_as_before(kind):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import dropout_signinv as S
    for mod in (DS, S):
        for act in ("tanh", "elu", "swish"):
            with pytest.raises(ValueError, match="HIP path: only relu"):
                getattr(mod, AC.CLASSES[kind])(*_args(kind), use_bn=True, dropout=0.0, activation=act)
        assert getattr(mod, AC.CLASSES[kind])._signinv_activations == ("relu",)
    for act in ("tanh", "elu"):
        with pytest.raises(ValueError, match="HIP path: only relu"):
            DS.MLP(4, 8, 4, 3, use_bn=True, activation=act)
    with pytest.raises(ValueError, match="HIP path: only relu"):
        DS.GCN(1, 8, 4, 3, activation="tanh")
    params = dict(sign_inv_net=kind, hidden_dim=8, phi_out_dim=4, sign_inv_layers=3, pos_enc_dim=4, dropout=0.0, sign_inv_activation="tanh",
                  device="cpu")
    for factory in (DS.get_sign_inv_net, S.get_sign_inv_net):
        with pytest.raises(ValueError, match="HIP path: only relu"):
            factory(params)


@pytest.mark.parametrize("kind", list(AC.CLASSES))
def test_new_classes_accept_and_refuse_what_the_reference_does(kind):
    """layers/gnns.py:13 looks the name up in {'relu', 'tanh'} before any MLP exists (KeyError with the name); layers/mlp.py:23-30 raises
    ValueError('Invalid activation')."""
    from signnet_basisnet_amd import activation_signinv as A
    cls = getattr(A, AC.CLASSES[kind])
    for act in AC.ACCEPTED[kind]:
        m = cls(*_args(kind), use_bn=True, dropout=0.0, activation=act)
        assert m._act == (None if act == "relu" else act) and m.rho.activation == act
    for act, exc in AC.REFUSED[kind].items():
        with pytest.raises(exc) as e:
            cls(*_args(kind), use_bn=True, dropout=0.0, activation=act)
        assert e.type is exc
        assert e.value.args == ((act,) if exc is KeyError else ("Invalid activation",))
        params = dict(sign_inv_net=kind, hidden_dim=8, phi_out_dim=4, sign_inv_layers=3, pos_enc_dim=4, dropout=0.0,
                      sign_inv_activation=act, device="cpu")
        with pytest.raises(exc):
            A.get_sign_inv_net(params)
    if kind in ("gcn", "transformer"):          # what stays refused (the GIN encoders never hand use_ln on, as in the reference)
        with pytest.raises(ValueError, match="HIP path"):
            cls(*_args(kind), use_bn=True, use_ln=True, dropout=0.0, activation="tanh")
    with pytest.raises(ValueError, match="Invalid sign inv net"):
        A.get_sign_inv_net(dict(sign_inv_net="deepsets", hidden_dim=8, phi_out_dim=4, sign_inv_layers=3, pos_enc_dim=4, dropout=0.0,
                                sign_inv_activation="tanh", device="cpu"))


@pytest.mark.parametrize("kind", ["gin", "masked_gin"])
def test_reduced_matmul_precision_is_refused_for_a_non_relu_gin_encoder(kind):
    from signnet_basisnet_amd import activation_signinv as A
    m = getattr(A, AC.CLASSES[kind])(*((1, 64, 4, 3, 4) + (("cpu",) if kind == "masked_gin" else ())), use_bn=True, dropout=0.0,
                                     activation="tanh")
    m.matmul_precision = "highest"
    for name in ("high", "medium"):
        with pytest.raises(ValueError, match="tanh encoder"):
            m.matmul_precision = name
    assert m.matmul_precision == "highest"
    r = getattr(A, AC.CLASSES[kind])(*((1, 64, 4, 3, 4) + (("cpu",) if kind == "masked_gin" else ())), use_bn=True, dropout=0.0,
                                     activation="relu")
    r.matmul_precision = "high"            # relu through the new class: the base class's switch
    assert r.matmul_precision == "high"


# ----------------------------------------------------------------------------- parameters, class chain
@pytest.mark.parametrize("name", AC.ENCODER_CASES)
def test_state_dict_keys_are_the_references(name):
    from signnet_basisnet_amd import dropout_signinv as S
    fx = fixture(name)
    m = AC.build(fx)                                            # (a strict load)
    assert list(m.state_dict().keys()) == [str(k) for k in fx.meta["sd_keys"]]
    base = AC.build(fx, module=S, activation="relu")
    assert list(base.state_dict().keys()) == list(m.state_dict().keys())
    assert [tuple(v.shape) for v in base.state_dict().values()] == [tuple(v.shape) for v in m.state_dict().values()]


@pytest.mark.parametrize("kind", list(AC.CLASSES))
def test_relu_through_the_new_factory_is_the_dropout_signinv_class(kind):
    from signnet_basisnet_amd import activation_signinv as A
    from signnet_basisnet_amd import dropout_signinv as S
    params = dict(sign_inv_net=kind, hidden_dim=8, phi_out_dim=4, sign_inv_layers=3, pos_enc_dim=4, dropout=0.0, sign_inv_activation="relu",
                  device="cpu")
    m = A.get_sign_inv_net(params)
    cls = type(m)
    assert cls is getattr(A, AC.CLASSES[kind]) and cls.__mro__[1] is getattr(S, AC.CLASSES[kind])
    assert {k for k in vars(cls) if not k.startswith("__")} == {"_signinv_activations"}, "the subclass differs in one class attribute"
    assert cls._signinv_activations == AC.ACCEPTED[kind] and m._act is None and m._signinv_dropout


def test_the_five_nets_build_their_encoder_with_the_new_factory():
    from signnet_basisnet_amd import activation_signinv as A
    from signnet_basisnet_amd import readout_models
    fx = fixture(AC.NET_CASE)
    assert set(A.NETS) == set(readout_models.NETS)
    for cls in A.NETS.values():
        assert issubclass(cls, getattr(readout_models, cls.__name__)) and cls._sign_inv_factory is A.get_sign_inv_net
    net = A.GatedGCNNet(AC.net_params(fx, "cpu"))
    assert type(net.sign_inv_net) is A.GINDeepSigns and net.sign_inv_net._act == "tanh"
    net.load_state_dict(fx.sd, strict=True)
    assert list(net.state_dict().keys()) == [str(k) for k in fx.meta["sd_keys"]]
    with pytest.raises(ValueError, match="HIP path: only relu"):
        readout_models.GatedGCNNet(AC.net_params(fx, "cpu"))


# ----------------------------------------------------------------------------- the drop-in
_NAMES = ["nets.ZINC_graph_regression." + m for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net", "sign_inv_net")]


def _resolve(finder, name):
    import importlib
    spec = finder.find_spec(name)
    assert spec is not None, name
    return importlib.import_module(spec.origin)


def test_dropin_resolves_the_new_names_only_with_the_flag():
    from signnet_basisnet_amd import activation_signinv as A
    from signnet_basisnet_amd import dgl_deepsigns, dropin, readout_models
    pkg = "signnet_basisnet_amd.dropin"
    assert dropin.AliasFinder("graphprediction").table == dropin.ALIASES["graphprediction"]
    mx = dropin.AliasFinder("graphprediction", max_readout=True).table
    assert not any("activation" in v for v in mx.values())
    act = dropin.AliasFinder("graphprediction", sign_inv_activation=True).table
    assert all(act[n] == pkg + ".signinv_activation_nets" for n in _NAMES) and act["layers.deepsigns"] == pkg + ".signinv_activation_layers"
    assert set(act) == set(mx)
    for tree in ("alchemy", "gine_pyg", "learningfilters"):
        assert dropin.AliasFinder(tree, sign_inv_activation=True).table == dropin.AliasFinder(tree, max_readout=True).table
    dropin.uninstall("graphprediction")
    try:
        f = dropin.install("graphprediction", max_readout=True)
        assert _resolve(f, _NAMES[1]).GatedGCNNet is readout_models.GatedGCNNet
        assert dropin.install("graphprediction", sign_inv_activation=True) is f          # extends the installed finder in place
        for n, cls in zip(_NAMES, ("GINNet", "GatedGCNNet", "PNANet", "TransformerNet", "GATNet")):
            assert getattr(_resolve(f, n), cls) is getattr(A, cls)
        assert _resolve(f, _NAMES[5]).get_sign_inv_net is A.get_sign_inv_net
        layers = _resolve(f, "layers.deepsigns")
        assert layers.GINDeepSigns is A.GINDeepSigns and layers.TransformerDeepSigns is A.TransformerDeepSigns and layers.MLP is dgl_deepsigns.MLP
        dropin.install("graphprediction", max_readout=True)                      # a later call with less takes nothing away
        assert _resolve(f, _NAMES[0]).GINNet is A.GINNet
        assert f.find_spec("nets.ZINC_graph_regression.load_net") is None and f.find_spec("layers.mlp") is None
    finally:
        dropin.uninstall("graphprediction")


def test_runner_flag(monkeypatch, tmp_path):
    import sys
    from signnet_basisnet_amd import dropin
    from signnet_basisnet_amd.dropin import run
    seen = {}
    monkeypatch.setattr(run, "install", lambda tree, **kw: seen.update(tree=tree, **kw))
    script = tmp_path / "main_ZINC_graph_regression.py"
    script.write_text("import sys\nARGS = list(sys.argv)\n")
    argv, path = list(sys.argv), list(sys.path)
    try:
        run.main(["--sign-inv-activation", str(script), "--sign_inv_activation", "tanh"])
    finally:
        sys.argv[:] = argv
        sys.path[:] = path
    assert seen == dict(tree="graphprediction", baselines=False, gnn_types=False, feature_dropout=True, sign_inv_dropout=True,
                        max_readout=True, sign_inv_activation=True)
    assert "--sign-inv-activation" in run.__doc__ and "SIGN_INV_ACTIVATION_OVERRIDES" in dropin.install.__doc__
    with pytest.raises(SystemExit, match=r"\[--sign-inv-activation\]"):
        run.main([])


# ----------------------------------------------------------------------------- header and C ABI
def test_header_constants_and_declarations():
    hdr = open(os.path.join(ROOT, "include", "signnet_hip.h")).read()
    assert re.search(r"^#define SN_ACT_TANH 1\b", hdr, re.M) and re.search(r"^#define SN_ACT_ELU\s+2\b", hdr, re.M)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint sn_act_affine_f32\(", code) and re.search(r"\bint sn_act_affine_bwd_f32\(", code)
    from signnet_basisnet_amd import ops
    assert (ops.ACT_TANH, ops.ACT_ELU) == (1, 2) == (AC.ACT_CODES["tanh"], AC.ACT_CODES["elu"]) and ops.ACTIVATIONS == AC.ACT_CODES


def test_argument_errors_are_returned_before_any_launch():
    """The checks run on the host: callable without a GPU (16 stands for any non-NULL, 16-byte aligned address)."""
    from signnet_basisnet_amd import _lib
    L = _lib.lib()
    one = 16
    fwd, bwd = L.sn_act_affine_f32, L.sn_act_affine_bwd_f32
    for act in (0, 3, -1):
        assert fwd(one, 4, 2, 4, None, 0, act, None, None, one, 4, None) == -1 and b"unknown activation" in L.sn_last_error()
        assert bwd(one, 4, one, 4, 2, 4, None, 0, act, one, 4, None) == -1 and b"unknown activation" in L.sn_last_error()
    assert fwd(one, 4, 2, 4, None, 0, 1, one, None, one, 4, None) == -1 and b"scale and shift go together" in L.sn_last_error()
    assert fwd(one, 4, 2, 4, None, 0, 2, None, one, one, 4, None) == -1 and b"scale and shift go together" in L.sn_last_error()
    assert fwd(None, 4, 2, 4, None, 0, 1, None, None, one, 4, None) == -1 and b"sn_act_affine_f32" in L.sn_last_error()
    assert fwd(one, 3, 2, 4, None, 0, 1, None, None, one, 4, None) == -1                     # ldx < C
    assert fwd(one, 4, 2, 4, one, 0, 1, None, None, one, 4, None) == -1 and b"nvalid needs K > 0" in L.sn_last_error()
    assert fwd(one + 2, 4, 2, 4, None, 0, 1, None, None, one, 4, None) == -1 and b"misaligned" in L.sn_last_error()
    assert bwd(one, 4, None, 4, 2, 4, None, 0, 1, one, 4, None) == -1 and b"sn_act_affine_bwd_f32" in L.sn_last_error()
    assert bwd(one, 4, one, 4, 2, 4, None, 0, 1, one, 3, None) == -1                        # lddx < C
    assert fwd(one, 4, 0, 4, None, 0, 1, None, None, one, 4, None) == 0 and bwd(one, 4, one, 4, 0, 4, None, 0, 2, one, 4, None) == 0   # R = 0
    from signnet_basisnet_amd import ops
    with pytest.raises(ValueError, match="activation must be one of"):
        ops.act_affine(torch.zeros(2, 4), "relu")
    with pytest.raises(ValueError, match="scale and shift go together"):
        ops.act_affine(torch.zeros(2, 4), "tanh", scale=torch.ones(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.act_affine(torch.zeros(2, 4), "tanh")


def test_path_predicate_table():
    """Every clause of the two vector conditions of csrc/activation.hip falsified alone."""
    P = AC.path
    assert P(68, (68, 68), (0, 0), (0, 0)) == "row" and P(68, (72, 76), (16, 32), (48, 64)) == "row"
    assert P(67, (67, 67), (0, 0), (0, 0)) == "flat"                      # C % 4 != 0, contiguous
    assert P(68, (68, 68), (0, 0), (4, 0)) == "flat" and P(68, (68, 68), (0, 0), (0, 8)) == "flat"      # scale / shift off a 16-byte boundary
    assert P(68, (69, 72), (0, 0), (0, 0)) == "scalar" and P(68, (72, 70), (0, 0), (0, 0)) == "scalar"  # one ld % 4 != 0
    assert P(68, (68, 68), (4, 0), (0, 0)) == "scalar" and P(68, (68, 68), (0, 4), (0, 0)) == "scalar"  # one pointer 4 bytes off
    assert P(67, (68, 67), (0, 0), (0, 0)) == "scalar" and P(67, (67, 67), (0, 12), (0, 0)) == "scalar"
    assert P(64, (64, 64, 64), (0, 0, 0)) == "row" and P(64, (64, 65, 64), (0, 0, 0)) == "scalar" and P(95, (95, 95, 95), (0, 0, 0)) == "flat"
