"""LCMKernel without a device: the dense branch against tests/lcm_ref.py, the constructor's checks, the parameter layout and the native rule."""
import pytest
import torch

from tests.lcm_ref import lcm_matrix, task_covar


def _kernel(g, dtype, T=3):
    k = g.kernels.LCMKernel([g.kernels.ScaleKernel(g.kernels.RBFKernel(ard_num_dims=2)), g.kernels.MaternKernel(nu=1.5)], num_tasks=T, rank=1).to(dtype)
    k.covar_module_list[0].data_covar_module.base_kernel.lengthscale = torch.tensor([[0.6, 1.1]])
    k.covar_module_list[0].data_covar_module.outputscale = 1.7
    k.covar_module_list[1].data_covar_module.lengthscale = 0.8
    gen = torch.Generator().manual_seed(0)
    for mt in k.covar_module_list:
        with torch.no_grad():
            mt.task_covar_module.covar_factor.copy_(torch.randn(T, 1, generator=gen))
        mt.task_covar_module.var = torch.rand(T, generator=gen) + 0.2
    return k


def _members(k):
    a, b = k.covar_module_list
    return [(None, a.data_covar_module.base_kernel.lengthscale.detach().reshape(-1), a.data_covar_module.outputscale.detach(),
             task_covar(a.task_covar_module.covar_factor.detach(), a.task_covar_module.var.detach())),
            (1.5, b.data_covar_module.lengthscale.detach().reshape(-1), 1.0, task_covar(b.task_covar_module.covar_factor.detach(), b.task_covar_module.var.detach()))]


@pytest.mark.parametrize("dtype,bound", [(torch.float64, 1e-12), (torch.float32, 1e-5)])
def test_dense_branch_against_reference(dtype, bound):
    import gpytorch_amd as g

    gen = torch.Generator().manual_seed(1)
    x1, x2 = torch.rand(7, 2, generator=gen, dtype=torch.float64), torch.rand(5, 2, generator=gen, dtype=torch.float64)
    k = _kernel(g, dtype)
    ref = lcm_matrix(x1, x2, _members(k))
    got = g.to_dense(k(x1.to(dtype), x2.to(dtype))).detach().double()
    assert got.shape == (21, 15) and k.num_outputs_per_input(x1, x2) == 3
    assert float((got - ref).abs().max() / ref.abs().max()) < bound


def test_constructor_errors_and_state_dict():
    import gpytorch_amd as g

    with pytest.raises(ValueError, match="At least one base kernel"):
        g.kernels.LCMKernel([], num_tasks=2)
    with pytest.raises(ValueError, match="must only contain Kernel objects"):
        g.kernels.LCMKernel([g.kernels.RBFKernel(), "rbf"], num_tasks=2)
    with pytest.raises(ValueError):
        g.kernels.LCMKernel([g.kernels.RBFKernel(), g.kernels.RBFKernel()], num_tasks=2, rank=[1])
    keys = set(_kernel(g, torch.float32).state_dict())
    assert {"covar_module_list.0.task_covar_module.covar_factor", "covar_module_list.0.task_covar_module.raw_var",
            "covar_module_list.0.data_covar_module.raw_outputscale", "covar_module_list.0.data_covar_module.base_kernel.raw_lengthscale",
            "covar_module_list.1.task_covar_module.covar_factor", "covar_module_list.1.task_covar_module.raw_var",
            "covar_module_list.1.data_covar_module.raw_lengthscale"} <= keys


def test_native_rule():
    import gpytorch_amd as g

    K = g.kernels
    x = torch.rand(6, 2)
    assert K.lcm_native(_kernel(g, torch.float32), x)
    refused = {
        "float64": (_kernel(g, torch.float64), x.double()),
        "d = 5": (K.LCMKernel([K.RBFKernel()], num_tasks=2), torch.rand(6, 5)),
        "Q = 5": (K.LCMKernel([K.RBFKernel() for _ in range(5)], num_tasks=2), x),
        "T = 9": (K.LCMKernel([K.RBFKernel()], num_tasks=9), x),
        "RQ base": (K.LCMKernel([K.RQKernel()], num_tasks=2), x),
        "active_dims": (K.LCMKernel([K.RBFKernel(active_dims=[0])], num_tasks=2), x),
        "batch": (_kernel(g, torch.float32), torch.rand(3, 6, 2)),
    }
    for why, (k, xx) in refused.items():
        assert not K.lcm_native(k, xx), why
