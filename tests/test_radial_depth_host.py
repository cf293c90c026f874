"""Radial networks of 1 to 4 hidden layers (the reference's invariant_layers) on the host: the validator's envelope, model
construction with the reference's state_dict names, and the fp16-range bound of the last hidden layer's features."""
import numpy as np
import pytest
import torch

from common import ATOMIC, LMAX2, PAPER, build_pair

DS = {"allowed_species": [13, 29, 79], "average_num_neighbors": 18.0}


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_validate_hparams_accepts_one_to_four_radial_layers(layers):
    from matten_amd.model_factory.utils import validate_hparams

    validate_hparams(dict(PAPER, invariant_layers=layers), DS)


@pytest.mark.parametrize("layers", [0, 5])
def test_validate_hparams_refuses_other_depths(layers):
    from matten_amd.model_factory.utils import UnsupportedConfig, validate_hparams

    with pytest.raises(UnsupportedConfig, match="invariant_layers"):
        validate_hparams(dict(PAPER, invariant_layers=layers), DS)


def test_validate_hparams_still_refuses_other_widths():
    from matten_amd.model_factory.utils import UnsupportedConfig, validate_hparams

    with pytest.raises(UnsupportedConfig, match="invariant_neurons") as ei:
        validate_hparams(dict(PAPER, invariant_layers=3, invariant_neurons=64), DS)
    assert "invariant_layers=3" not in str(ei.value)   # the depth itself is fine


@pytest.mark.parametrize("layers", [1, 3, 4])
@pytest.mark.parametrize("atomic", [False, True])
def test_models_build_with_the_reference_state_dict_at_any_depth(layers, atomic):
    hp = dict(ATOMIC if atomic else LMAX2, invariant_layers=layers)
    ref, model = build_pair(hp, DS, device=None, atomic=atomic)
    sd, want = model.state_dict(), ref.state_dict()
    extra = {k for k in want if k.endswith(("output_mask", "tp.tp.weight"))}
    assert set(sd) == set(want) - extra
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in want.items() if k in sd}
    mlps = [m for m in model.modules() if type(m).__name__ == "RadialMLP"]
    assert mlps and all(m.n_mid == layers - 1 and len(m.weights()) == layers + 1 for m in mlps)
    assert all(f"layer{layers}" in dict(m.named_children()) and f"layer{layers + 1}" not in dict(m.named_children())
               for m in mlps)
    # the middle layers are 32 -> 32, the last one reads 32 features
    assert all(tuple(m.weights()[-1].shape)[0] == 32 and all(tuple(w.shape) == (32, 32) for w in m.weights()[1:-1])
               for m in mlps)


def test_radial_mlp_shapes_outside_the_envelope_are_refused():
    from matten_amd.nn.utils import RadialMLP

    RadialMLP([8, 32, 48])
    RadialMLP([8, 32, 32, 32, 32, 48])
    for hs in ([8, 48], [8] + 5 * [32] + [48], [8, 32, 64, 48], [8, 64, 48]):
        with pytest.raises(NotImplementedError, match="invariant_layers"):
            RadialMLP(hs)


def _last_hidden_fp64(mlp, r, r_start, r_end):
    """the last hidden layer's features h_L[E, 32] the hidden-layer kernels split into fp16 pieces, in fp64"""
    from oracle.e3nn_lite.math import soft_one_hot_linspace

    nb = mlp.hs[0]
    ws = [w.detach().double() for w in mlp.weights()]
    x = soft_one_hot_linspace(r, r_start, r_end, nb, "bessel", True) * nb**0.5
    h = torch.nn.functional.silu(x @ (ws[0] / nb**0.5))
    for w in ws[1:-1]:
        h = torch.nn.functional.silu(h @ (w * (mlp.act_cst / 32**0.5)))
    return h


@pytest.mark.parametrize("layers", [1, 3, 4])
@pytest.mark.parametrize("blow_up", [1.0, 1e3])
def test_fp16_scale_bounds_the_last_hidden_layer(layers, blow_up):
    """RadialMLP._fp16_scale bounds |h_L| by P(c) n0 prod_i n_i over the middle layers: for every edge length of a dense
    fp64 sweep of [start, end], |h_L| * s < 2^15, with normally scaled and with 10^3 x larger weights."""
    from matten_amd.nn.utils import RadialMLP

    torch.manual_seed(layers)
    r_start, r_end, nb = 0.0, 5.0, 8
    mlp = RadialMLP([nb] + layers * [32] + [48])
    with torch.no_grad():
        for w in mlp.weights()[:-1]:
            w.mul_(blow_up)
    r = torch.linspace(r_start, r_end, 20001, dtype=torch.float64)[1:]   # (the basis is 0 at r = start, the formula 0/0)
    h = _last_hidden_fp64(mlp, r, r_start, r_end)
    s, inv = (float(v) for v in mlp.h_scale(r_start, r_end))
    assert s > 0 and np.log2(s) == int(np.log2(s)) and inv == 1.0 / s
    assert float(h.abs().max()) * s < 2.0**15
    if blow_up == 1.0:
        assert s == 1.0          # a normally scaled MLP is not scaled at all
    elif layers > 1:
        assert s < 1.0           # (one hidden layer of 10^3 x weights stays inside the range)
