"""Fine-tuning with frozen BatchNorm statistics, host side: freeze_batchnorm / unfreeze_batchnorm on a model that never
touches the GPU, the optimizer_hparams switch, the new C entries, and the refusal that is gone."""
import os
import re

import pytest
import torch

from common import LMAX2, build_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = {"allowed_species": [13, 29, 79], "average_num_neighbors": 18.0}
ADAM = {"class_path": "torch.optim.Adam", "init_args": {"lr": 0.01, "weight_decay": 0.00001}}


def _bns(model):
    from matten_amd.nn.utils import _IrrepBatchNorm

    bns = [m for m in model.modules() if isinstance(m, _IrrepBatchNorm)]
    assert len(bns) == LMAX2["num_layers"]
    return bns


def test_freeze_batchnorm_survives_model_train_and_is_undone_by_unfreeze():
    from matten_amd.model import freeze_batchnorm, unfreeze_batchnorm

    _, model = build_pair(LMAX2, DS, device=None)
    before = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.train()
    assert all(bn.training for bn in _bns(model))
    assert freeze_batchnorm(model) is model
    assert not any(bn.training for bn in _bns(model))
    model.train()                       # what a trainer does at the start of every epoch
    assert model.training and not any(bn.training for bn in _bns(model))
    others = [m for m in model.modules() if m not in _bns(model)]
    assert all(m.training for m in others)          # mixed mode: everything else trains
    assert all(bn.weight.requires_grad and bn.bias.requires_grad for bn in _bns(model))
    model.eval()
    model.train()
    assert not any(bn.training for bn in _bns(model))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == before
    assert unfreeze_batchnorm(model) is model
    assert all(bn.training for bn in _bns(model))
    model.eval()
    assert not any(bn.training for bn in _bns(model))
    model.train()
    assert all(bn.training for bn in _bns(model))


def test_freeze_affine_sets_and_restores_requires_grad():
    from matten_amd.model import freeze_batchnorm, unfreeze_batchnorm

    _, model = build_pair(LMAX2, DS, device=None)
    bns = _bns(model)
    bns[1].bias.requires_grad_(False)   # a flag the user set stays the user's
    n_all = sum(1 for p in model.parameters() if p.requires_grad)
    freeze_batchnorm(model, freeze_affine=True)
    freeze_batchnorm(model, freeze_affine=True)   # twice: the remembered flags are the original ones
    assert not any(bn.weight.requires_grad or bn.bias.requires_grad for bn in bns)
    assert sum(1 for p in model.parameters() if p.requires_grad) == n_all - (2 * len(bns) - 1)
    unfreeze_batchnorm(model)
    assert all(bn.weight.requires_grad for bn in bns)
    assert [bn.bias.requires_grad for bn in bns] == [True, False, True]
    # unfreezing in eval mode leaves the modules in eval mode
    freeze_batchnorm(model.train())
    unfreeze_batchnorm(model.eval())
    assert not any(bn.training for bn in bns)


def test_alias_import_path_resolves():
    import matten.model
    import matten_amd.model

    assert matten.model.freeze_batchnorm is matten_amd.model.freeze_batchnorm
    assert matten.model.unfreeze_batchnorm is matten_amd.model.unfreeze_batchnorm


@pytest.mark.parametrize("value,affine", [(None, None), (True, False), ("statistics", False), ("affine", True)])
def test_configure_optimizers_honours_freeze_batchnorm(value, affine):
    from matten_amd.model_factory.task import TensorRegressionTask
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    hp = dict(ADAM) if value is None else dict(ADAM, freeze_batchnorm=value)
    model = ScalarTensorModel(tasks=TensorRegressionTask(name="elastic_tensor_full"), backbone_hparams=dict(LMAX2),
                              dataset_hparams=DS, optimizer_hparams=hp)
    n_params = sum(1 for _ in model.parameters())
    cfg = model.configure_optimizers()
    opt = cfg["optimizer"] if isinstance(cfg, dict) else cfg
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == 0.01
    model.train()
    n_opt = sum(len(g["params"]) for g in opt.param_groups)
    if value is None:                     # absent: today's behaviour
        assert all(bn.training for bn in _bns(model)) and n_opt == n_params
        return
    assert not any(bn.training for bn in _bns(model))
    assert all(bn.weight.requires_grad != affine and bn.bias.requires_grad != affine for bn in _bns(model))
    assert n_opt == n_params - (2 * len(_bns(model)) if affine else 0)


def test_configure_optimizers_refuses_an_unknown_freeze_mode():
    from matten_amd.model_factory.task import TensorRegressionTask
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    model = ScalarTensorModel(tasks=TensorRegressionTask(name="elastic_tensor_full"), backbone_hparams=dict(LMAX2),
                              dataset_hparams=DS, optimizer_hparams=dict(ADAM, freeze_batchnorm="running"))
    with pytest.raises(ValueError, match="freeze_batchnorm"):
        model.configure_optimizers()


def test_eval_adjoint_entries_are_declared_bound_and_exported():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    lib = _lib.load()
    for name in ("matten_gate_bn_eval_bwd", "matten_norm_act_bn_eval_bwd", "matten_bn_eval_bwd_scratch_floats"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION >= 46 and lib.matten_abi_version() == _lib.ABI_VERSION
    # one float2 record per (16-row block, column)
    assert lib.matten_bn_eval_bwd_scratch_floats(37, 10) == 2 * 3 * 10
    assert lib.matten_bn_eval_bwd_scratch_floats(0, 10) == 0


def test_the_refusal_is_gone_from_the_package():
    hits = []
    for d, _, files in os.walk(os.path.join(ROOT, "matten_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")) and "call model.train()" in open(os.path.join(d, f), errors="replace").read():
                hits.append(os.path.join(d, f))
    assert not hits, hits
