"""CPU: NeuMF construction, flags and bookkeeping against the reference's (tests/golden/neumf_*.npz)."""
import pytest
import torch

from conftest import load_golden

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd.neumf import ModelFlag, NeuMF, get_sparsity_and_param


def _build(cfg=None):
    g = load_golden("neumf_model")
    torch.manual_seed(2023)
    return NeuMF(int(g["num_user"]), int(g["num_item"]), emb_size=int(g["emb_size"]), hidden_sizes=[int(h) for h in g["hidden"]],
                 p_dropout=0, embedding_config=cfg), g


def test_exported_from_the_package():
    assert pkg.NeuMF is NeuMF and pkg.ModelFlag is ModelFlag
    assert [f.value for f in ModelFlag] == [1, 2, 3]


def test_seeded_construction_matches_the_reference_parameters_and_key_order():
    model, g = _build()
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for k, v in sd.items():
        assert torch.equal(v, g.t("param/" + k)), k


def test_seeded_qr_construction_matches_the_reference():
    model, _ = _build({"name": "qr", "operation": "mult", "divider": 3})
    g = load_golden("neumf_qr")
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for k, v in sd.items():
        assert torch.equal(v, g.t("param/" + k)), k


def test_flags_get_embs_and_sparsity():
    model, g = _build()
    assert model.flag == ModelFlag.NMF and model.mlp_flag() and model.gmf_flag()
    assert [n for n, _ in model.get_embs()] == ["mlp-user", "mlp-item", "gmf-user", "gmf-item"]
    assert model.get_embs()[0][1] is model._mlp.user_emb_table
    sp, n = get_sparsity_and_param(model)
    assert n == int(g["n_params"]) and sp == pytest.approx(float(g["sparsity"]), abs=0)
    model.flag = ModelFlag.GMF
    assert not model.mlp_flag()
    assert [n for n, _ in model.get_embs()] == ["gmf-user", "gmf-item"]
    sp, n = get_sparsity_and_param(model)
    assert n == int(g["n_params_gmf"]) and sp == pytest.approx(float(g["sparsity_gmf"]), abs=0)
    model.flag = ModelFlag.MLP
    assert [n for n, _ in model.get_embs()] == ["mlp-user", "mlp-item"]
    assert (model.num_user, model.num_item) == (int(g["num_user"]), int(g["num_item"]))


def test_update_weight_scales_the_two_heads():
    model, g = _build()
    model.update_weight(0.25)
    assert torch.allclose(model._gmf.gmf_fc.weight, g.t("param/_gmf.gmf_fc.weight") * 0.75)
    assert torch.allclose(model._gmf.gmf_fc.bias, g.t("param/_gmf.gmf_fc.bias") * 0.75)
    assert torch.allclose(model._mlp.mlp_fc.weight, g.t("param/_mlp.mlp_fc.weight") * 0.25)
    assert torch.allclose(model._mlp.mlp_fc.bias, g.t("param/_mlp.mlp_fc.bias") * 0.25)


def test_checkpoint_round_trip(tmp_path):
    model, _ = _build()
    model.update_weight(0.5)
    path = tmp_path / "nmf.pth"
    torch.save(model.state_dict(), path)
    other = NeuMF(model.num_user, model.num_item, emb_size=16, hidden_sizes=[16, 8])
    other.load_state_dict(torch.load(path))
    for (ka, va), (kb, vb) in zip(model.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_clear_cache_resets_the_cached_tables():
    model, _ = _build()
    model._gmf._user_emb = model._mlp._item_emb = torch.zeros(1)
    model.clear_cache()
    assert all(getattr(p, a) is None for p in (model._gmf, model._mlp) for a in ("_user_emb", "_item_emb"))


def test_cpu_tensors_raise_the_library_error():
    model, _ = _build()
    users, items = torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
    for flag in (ModelFlag.NMF, ModelFlag.GMF, ModelFlag.MLP):
        model.flag = flag
        with pytest.raises(pkg.MI355XLibraryError):
            model(users, items)
    with pytest.raises(pkg.MI355XLibraryError):
        model.score_all_items(users)


def test_hccf_stays_refused():
    with pytest.raises(Exception):
        pkg.get_graph_model(3, 3, {"name": "hccf"})
