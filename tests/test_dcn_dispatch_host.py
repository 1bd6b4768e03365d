"""CPU: the yardstick behind tests/test_dcn_dispatch_gpu.py.  For every head and model case of tests/dcn_dispatch_helpers.py
the oracle in stock float32 already lies inside the tolerance the GPU test applies against the float64 oracle, and no ReLU
pre-activation of a model case is near its kink — so a GPU failure there is the kernels', not the tolerance's.

Measured here (max over the tensors of a case of |float32 - float64| / tolerance; 1.0 would be the edge):
  DCNHead      d22-three-pass 0.006, d15-three-pass 0.011, d1028-three-pass-panel 0.002, d1030-three-pass-general 0.002,
               d24-panel-off 0.006, view case 0.005
  DCN_MixHead  d22-r16-no-fused-expert 0.006, E9-gate-by-gemm 0.007, d18-r48 0.003, d16-r5 0.004, L0 0, r16-panel-off and
               d40-r16-deterministic 0.006, d22-r8-deterministic 0.007, view case 0.006
  models       (train / eval) dcn_mix-nf5 0.005 / 0.001, dcn_mix-nf6 0.004 / 0.001, dcnv2-stacked-nf5 0.012 / 0.003,
               dcnv2-parallel-nf5 0.002 / 0.002; the nearest ReLU pre-activation of any case is 6.4e-4 from 0
(the worst tensor is the output / the logits in every case but d18-r48, where it is a bias gradient).  The assertions leave
half of each tolerance to the kernels: a case whose float32 evaluation needs more than that gets another seed or scale."""
import pytest
import torch

import dcn_dispatch_helpers as dh

HEADS = sorted(set(dh.DCN_HEAD_CASES.values()) | set(dh.MIX_HEAD_CASES.values()) | {dh.VIEW_DCN, dh.VIEW_MIX})


@pytest.mark.parametrize("dims", HEADS, ids=["x".join(map(str, d)) for d in HEADS])
def test_float32_oracle_of_a_head_case_is_inside_the_contract(dims):
    key, ratio = dh.head_worst(dh.head_eval(dims, torch.float32), dh.head_reference(dims))
    print(f"head {dims}: float32 vs float64 worst {key} at {ratio:.3f} of the tolerance")
    assert ratio <= 0.5, f"{dims}: {key} of the float32 oracle is at {ratio:.3f} of the tolerance: no room left for the kernels"


@pytest.mark.parametrize("dims", [dh.VIEW_DCN, dh.VIEW_MIX], ids=["dcn", "mix"])
def test_float32_oracle_with_an_upstream_gradient_of_ones(dims):
    head, X, _ = dh.head_problem(dims)
    key, ratio = dh.head_worst(dh.head_eval(dims, torch.float32, G=torch.ones_like(X)), dh.head_reference_ones(dims))
    print(f"head {dims} (sum): float32 vs float64 worst {key} at {ratio:.3f} of the tolerance")
    assert ratio <= 0.5


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", sorted(dh.MODEL_CASES))
def test_float32_oracle_of_a_model_case_is_inside_the_tolerance_and_off_the_kinks(name, training):
    ref = dh.model_reference(name, training)
    got = dh.model_eval(name, training, torch.float32)
    nearest = min(float(z.abs().min()) for z in ref["pre"])
    key, ratio = dh.model_worst(got, ref)
    print(f"model {name} training={training}: float32 vs float64 worst {key} at {ratio:.3f}; nearest pre-activation {nearest:.2e}")
    assert len(ref["pre"]) == dh.MODEL_CASES[name][2]
    assert nearest > dh.KINK, f"{name}: a ReLU pre-activation {nearest:.2e} from its kink: pick another seed"
    assert ratio <= 0.5, f"{name}: {key} of the float32 oracle is at {ratio:.3f} of the tolerance"
    assert abs(float(got["loss"]) - float(ref["loss"])) <= 1e-5
