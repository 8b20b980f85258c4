"""The drop-in runner's --attn-dropout switch and SignNetGNN.attn_dropout_source, as far as they go without a GPU."""
import pytest


def test_runner_switch_sets_the_source_of_new_models(monkeypatch):
    from signnet_basisnet_amd.dropin import run
    from signnet_basisnet_amd.pyg import SignNetGNN
    monkeypatch.setattr(SignNetGNN, "DEFAULT_ATTN_DROPOUT_SOURCE", "generator")
    assert SignNetGNN(None, None, 16, 1, 1, 1, variant="gine", max_k=4).attn_dropout_source == "generator"
    with pytest.raises(SystemExit, match="usage"):              # (no script: the options are parsed, nothing runs)
        run.main(["--attn-dropout=counter"])
    m = SignNetGNN(None, None, 16, 1, 1, 1, variant="gine", max_k=4)
    assert m.attn_dropout_source == "counter" and m._dropout_active()
    assert not any("dropout" in k or "_sn_" in k for k in m.state_dict())
    with pytest.raises(SystemExit, match="generator"):
        run.main(["--attn-dropout=philox", "main_alchemy.py"])


def test_source_property():
    from signnet_basisnet_amd.pyg import SignNetGNN
    m = SignNetGNN(None, None, 16, 1, 1, 1, variant="gine", max_k=4)
    assert m.attn_dropout_source == "generator" and not m._dropout_active()
    m.attn_dropout_source = "counter"
    assert m._dropout_active()
    m.attn_dropout = 0.0
    assert not m._dropout_active()
    with pytest.raises(ValueError, match="attn_dropout_source"):
        m.attn_dropout_source = "torch"
    assert m.attn_dropout_source == "counter"
