"""The host side of the training flow (flowcompare_amd/train_flow.py): the layer plan parsed from `flow.transforms` and the
activation budget that decides which layers keep their activations.  CPU modules only: no library, no kernel."""
import dataclasses

import pytest
import torch

import flowcompare_amd as fa
from conftest import Fixture
from flowcompare_amd import modules as M
from flowcompare_amd import train_flow as TF

COUPLING = {"RationalQuadraticSplineCoupling": M.RationalQuadraticSplineCoupling, "AffineCoupling": M.AffineCoupling,
            "ExponentialCoupling": M.ExponentialCoupling}
PERMUTER = {"LinearLU": M.LinearLU, "random_permute": M.Permuter, "FullCombiner": M.FullCombiner, "ExponentialCombiner": M.ExponentialCombiner}


def _flow(name):
    cfg = dict(Fixture(name).cfg)
    return cfg, fa.initialize_flow(cfg, device="cpu", mode="test")["flow"]


@pytest.mark.parametrize("name", ["e2e_tiny_spline_relu", "e2e_tiny_cif", "e2e_tiny_global_extra", "e2e_tiny_random_permute",
                                  "e2e_tiny_FullCombiner", "e2e_tiny_expcoupling", "e2e_tiny_identity_aug"])
def test_plan_mirrors_the_config(name):
    cfg, flow = _flow(name)
    augmenter, layers = TF.plan_layers(flow, cfg["using_extra_context"])
    cif = cfg["latent_dim"] < cfg["cif_latent_dim"]
    assert augmenter == ("attention" if cfg["latent_dim"] > cfg["input_dim"] else "identity")
    assert len(layers) == cfg["n_flow_layers"]
    for lay in layers:
        assert lay.cif == cif and type(lay.block) is (M.CIFblock if cif else M.PreConditionApplier)
        assert lay.block in list(flow.transforms)
        inner = lay.block.flow if cif else lay.block
        assert lay.pre_conditioner is inner.pre_conditioner and lay.coupling is inner.transform
        assert type(lay.coupling) is COUPLING[cfg["flow_type"]]
        assert type(lay.pre_conditioner) is (M.CouplingPreconditionerGlobal if cfg["global"] else M.CouplingPreconditionerAttn)
    for lay in layers[:-1]:
        assert type(lay.actnorm) is (M.ActNormBijectionCloud if cfg["act_norm"] else type(None))
        assert type(lay.permuter) is PERMUTER[cfg["permuter_type"]]
    assert layers[-1].actnorm is None and layers[-1].permuter is None
    # every module of flow.transforms sits in the plan exactly once, in order
    flat = [flow.transforms[0]] + [m for lay in layers for m in (lay.block, lay.actnorm, lay.permuter) if m is not None]
    assert len(flat) == len(flow.transforms) and all(a is b for a, b in zip(flat, flow.transforms))
    # noise sites: the augmenter's draw, then one per CIF layer
    assert (augmenter == "attention") + sum(lay.cif for lay in layers) == len(flow.noise_shapes(1, 1))
    with pytest.raises(dataclasses.FrozenInstanceError):
        layers[0].block = None


def _initialised_flags(flow):
    return [float(m.initialized) for m in flow.modules() if isinstance(m, M.ActNormBijectionCloud)]


def test_identity_between_two_layers_is_refused():
    cfg, flow = _flow("e2e_tiny_spline_relu")
    flow.train()
    before = _initialised_flags(flow)
    assert type(flow.transforms[1]) is M.PreConditionApplier and type(flow.transforms[2]) is M.ActNormBijectionCloud
    flow.transforms.insert(2, torch.nn.Identity())                  # behind layer 0's coupling, in front of its ActNorm
    with pytest.raises(NotImplementedError, match=r"^training path: transform Identity between layers$"):
        TF.plan_layers(flow, False)
    del flow.transforms[2]
    TF.plan_layers(flow, False)
    assert type(flow.transforms[4]) is M.PreConditionApplier
    flow.transforms.insert(4, torch.nn.Identity())                  # behind layer 0's permuter: where layer 1's block should stand
    with pytest.raises(NotImplementedError, match=r"^training path: transform Identity$"):
        TF.plan_layers(flow, False)
    # flow_log_prob refuses it too, before it touches a tensor (these are not even on a device) or an ActNorm layer
    with pytest.raises(NotImplementedError, match=r"^training path: transform Identity$"):
        TF.flow_log_prob(flow, torch.zeros(1, 4, cfg["input_dim"]), torch.zeros(1, 4, cfg["input_embedding_dim"]))
    assert _initialised_flags(flow) == before


def test_unknown_coupling_is_refused():
    _, flow = _flow("e2e_tiny_spline_relu")
    flow.transforms[1].transform = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match=r"^training path: coupling Identity$"):
        TF.plan_layers(flow, False)


def test_unknown_augmenter_is_refused():
    _, flow = _flow("e2e_tiny_spline_relu")
    flow.transforms[0] = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match=r"^training path: augmenter Identity$"):
        TF.plan_layers(flow, False)


def test_cif_with_extra_context_is_refused():
    _, flow = _flow("e2e_tiny_cif")
    TF.plan_layers(flow, False)
    with pytest.raises(Exception, match=r"^Not implemented extra context with cif$") as err:
        TF.plan_layers(flow, True)
    assert type(err.value) is Exception


# ---------------------------------------------------------------- the activation budget on synthetic growth figures
CUDA = torch.device("cuda", 0)                       # never touched: with an explicit budget the constructor asks the device nothing


def _drive(budget, growths):
    """flow_log_prob's loop without the layers: ask, and after a kept layer hand over the measured growth where one is measured."""
    kept = []
    for grown in growths:
        kept.append(budget.keep_next())
        if kept[-1] and budget.budget > 0:
            budget.record(grown)
    return kept


def test_without_checkpointing_every_layer_is_kept_and_nothing_is_recorded():
    b = TF.ActivationBudget(False, CUDA, 10)
    assert _drive(b, [4, 4, 4, 4]) == [True] * 4
    assert (b.budget, b.kept_bytes, b.layer_bytes, b.n_kept, b.n_ckpt) == (0, 0, None, 0, 0)
    with torch.no_grad():                                           # no graph, nothing to recompute
        b = TF.ActivationBudget(True, CUDA, 10)
    assert _drive(b, [4, 4, 4]) == [True] * 3 and (b.budget, b.n_kept, b.n_ckpt) == (0, 0, 0)


def test_budget_zero_checkpoints_every_layer():
    b = TF.ActivationBudget(True, CUDA, 0)
    assert _drive(b, [4, 4, 4]) == [False] * 3
    assert (b.budget, b.kept_bytes, b.layer_bytes, b.n_kept, b.n_ckpt) == (0, 0, None, 0, 3)
    b = TF.ActivationBudget(True, torch.device("cpu"), 10)         # not a CUDA input: budget 0
    assert _drive(b, [4, 4]) == [False] * 2 and b.budget == 0


def test_budget_ten_with_growths_of_four_checkpoints_the_third_layer():
    b = TF.ActivationBudget(True, CUDA, 10)
    assert _drive(b, [4, 4, 4, 4]) == [True, True, False, False]
    assert (b.budget, b.kept_bytes, b.layer_bytes, b.n_kept, b.n_ckpt) == (10, 8, 4, 2, 2)


def test_layer_bytes_is_the_largest_growth_seen_not_the_last():
    b = TF.ActivationBudget(True, CUDA, 16)
    assert _drive(b, [2, 6, 3]) == [True, True, True] and b.layer_bytes == 6 and b.kept_bytes == 11
    assert not b.keep_next()                                        # 11 + 6 > 16, though 11 + 3 (the last growth) would fit
    b = TF.ActivationBudget(True, CUDA, 16)
    assert _drive(b, [2, 3, 3]) == [True, True, True] and b.layer_bytes == 3 and b.keep_next()


def test_budget_one_keeps_exactly_the_first_layer():
    b = TF.ActivationBudget(True, CUDA, 1)
    assert _drive(b, [4, 4, 4]) == [True, False, False]
    assert (b.kept_bytes, b.layer_bytes, b.n_kept, b.n_ckpt) == (4, 4, 1, 2)


def test_the_argument_goes_before_the_module_level_budget(monkeypatch):
    monkeypatch.setattr(TF, "ACTIVATION_BUDGET_BYTES", 7)
    assert TF.ActivationBudget(True, CUDA).budget == 7
    assert TF.ActivationBudget(True, CUDA, 3).budget == 3
    assert TF.ActivationBudget(True, CUDA, 0).budget == 0
