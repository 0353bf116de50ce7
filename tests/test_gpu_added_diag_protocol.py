"""GPU: the five structured "K + diagonal" operators (sum of kernels, Hadamard and Kronecker multitask, derivative observations, grid
interpolation) are ONE protocol -- ``operators.StructuredAddedDiagLinearOperator`` with a handful of hooks filled in.  This asserts the protocol,
not new numerics: the operator algebra every subclass inherits, and one solve per operator on the CG branch against its own dense float64 matrix.

Shapes: n = 131 points (no multiple of 4 or 128), T = 2 tasks, d = 2, a 16-node grid per axis.  The solve bound is the one each operator's own
test asserts at ``cg_tolerance(1e-4)``: 2e-3 for the sum, the Kronecker and the Hadamard operator (tests/test_gpu_structured.py:
``test_sum_operator_preconditioner``, ``test_kronecker_operator_preconditioner_with_per_task_noise``, ``test_hadamard_operator_preconditioner``),
and 2e-3 for the mean-cache solve behind ``e_mu`` of tests/test_gpu_rbfgrad.py ``test_gp_posterior`` and tests/test_gpu_ski.py
``test_model_posterior``."""
import pytest
import torch

from tests.util import rel_err

pytestmark = pytest.mark.gpu

N, T, D, GRID = 131, 2, 2, 16
SOLVE_TOL = 2e-3


def _inputs(dev):
    gen = torch.Generator().manual_seed(0)
    x = (0.01 + 0.98 * torch.rand(N, D, generator=gen)).to(dev)
    tasks = torch.randint(0, T, (N,), generator=gen).to(dev)
    return x, tasks


def _index_kernel(g, dev):
    kt = g.kernels.IndexKernel(num_tasks=T, rank=1).to(dev)
    with torch.no_grad():
        kt.covar_factor.copy_(torch.tensor([[0.9], [-0.4]]))
    kt.var = torch.tensor([0.3, 0.5])
    return kt


def _build(name, g, dev):
    """(the added-diagonal operator on parameters that require grad, its class)."""
    from gpytorch_amd.composite import SumFusedAddedDiagLinearOperator
    from gpytorch_amd.derivative import RBFGradFusedAddedDiagLinearOperator
    from gpytorch_amd.hadamard import HadamardFusedAddedDiagLinearOperator
    from gpytorch_amd.multitask import KroneckerFusedAddedDiagLinearOperator, TaskNoiseDiagLinearOperator
    from gpytorch_amd.ski import SKIFusedAddedDiagLinearOperator

    x, tasks = _inputs(dev)
    noise = torch.tensor([0.1], device=dev, requires_grad=True)
    if name == "sum":
        kern = (g.kernels.ScaleKernel(g.kernels.RBFKernel()) + g.kernels.ScaleKernel(g.kernels.MaternKernel(nu=2.5))).to(dev)
        ka, kb = kern.kernels
        ka.base_kernel.lengthscale, ka.outputscale = 0.25, 1.1
        kb.base_kernel.lengthscale, kb.outputscale = 0.9, 0.4
        return kern(x).evaluate_kernel().add_diagonal(noise), SumFusedAddedDiagLinearOperator
    if name == "hadamard":
        kx = g.kernels.RBFKernel().to(dev)
        kx.lengthscale = 0.35
        return kx(x).evaluate_kernel().mul(_index_kernel(g, dev)(tasks)).add_diagonal(noise), HadamardFusedAddedDiagLinearOperator
    if name == "kronecker":
        kern = g.kernels.MultitaskKernel(g.kernels.RBFKernel(), num_tasks=T, rank=1).to(dev)
        kern.data_covar_module.lengthscale = 0.35
        with torch.no_grad():
            kern.task_covar_module.covar_factor.copy_(torch.tensor([[0.9], [-0.4]]))
        kern.task_covar_module.var = torch.tensor([0.3, 0.5])
        tn = torch.tensor([0.05, 0.1], device=dev, requires_grad=True)
        return kern(x).evaluate_kernel() + TaskNoiseDiagLinearOperator(tn, N), KroneckerFusedAddedDiagLinearOperator
    if name == "grad":
        kern = g.kernels.ScaleKernel(g.kernels.RBFKernelGrad()).to(dev)
        kern.base_kernel.lengthscale, kern.outputscale = 0.35, 1.3
        return kern(x).evaluate_kernel().add_diagonal(noise), RBFGradFusedAddedDiagLinearOperator
    kern = g.kernels.ScaleKernel(g.kernels.GridInterpolationKernel(g.kernels.RBFKernel(), grid_size=[GRID] * D, grid_bounds=[(0.0, 1.0)] * D)).to(dev)
    kern.base_kernel.base_kernel.lengthscale, kern.outputscale = 0.3, 1.3
    return kern(x).evaluate_kernel().add_diagonal(noise), SKIFusedAddedDiagLinearOperator


@pytest.mark.parametrize("name", ["sum", "hadamard", "kronecker", "grad", "ski"])
def test_added_diag_protocol(name, dev):
    import gpytorch_amd as g
    from gpytorch_amd.operators import DiagLinearOperator, StructuredAddedDiagLinearOperator

    S = g.settings
    op, cls = _build(name, g, dev)
    assert type(op) is cls and isinstance(op, StructuredAddedDiagLinearOperator)
    assert op.requires_grad
    n = op.shape[-1]
    gen = torch.Generator().manual_seed(1)
    # + a diagonal: the same class, the vector merged into noise_vec
    v = (0.01 + 0.02 * torch.rand(n, generator=gen)).to(dev)
    assert v.unique().numel() > 1
    op1 = op + DiagLinearOperator(v)
    assert type(op1) is cls and op1.noise_vec is not None and torch.equal(op1.noise_vec, v)
    op2 = op1 + DiagLinearOperator(v)
    assert type(op2) is cls and torch.equal(op2.noise_vec, v + v)
    assert torch.allclose(op2._diag_total(), op._diag_total() + 2 * v, rtol=1e-6, atol=0)
    assert torch.allclose(op2.diagonal(), op.diagonal() + 2 * v, rtol=1e-6, atol=0)
    # detach(): nothing left on the autograd path, the vector included
    vg = v.clone().requires_grad_(True)
    att = op + DiagLinearOperator(vg)
    assert att.noise_vec.requires_grad and att.requires_grad
    det = att.detach()
    assert type(det) is cls and not det.requires_grad and not det.noise_vec.requires_grad
    assert not det._diag_total().requires_grad and not det.to_dense().requires_grad
    # the log-determinant alone on the CG branch: an empty inv_quad
    with S.max_cholesky_size(0), S.cg_tolerance(1e-4), S.min_preconditioning_size(100), S.num_trace_samples(16):
        torch.manual_seed(0)
        iq, ld = op.inv_quad_logdet(None, logdet=True, reduce_inv_quad=False)
    assert iq.shape == (0,) and ld.numel() == 1 and bool(torch.isfinite(ld).all())
    # solve on the CG branch (row-built preconditioner on) against the operator's own dense matrix in float64, without and with a vector diagonal
    y = torch.randn(n, 1, generator=gen).to(dev)
    for which, o in (("scalar", op), ("vector", op1)):
        with torch.no_grad():
            ref = torch.linalg.solve(o.to_dense().double(), y.double())
            with S.max_cholesky_size(0), S.cg_tolerance(1e-4), S.min_preconditioning_size(100):
                sol = o.solve(y)
        err = rel_err(sol, ref)
        print("solve", name, which, n, err)
        assert sol.shape == (n, 1) and err < SOLVE_TOL, (name, which, err)
