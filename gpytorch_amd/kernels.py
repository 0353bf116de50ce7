"""Kernel modules of the hot path: ``RBFKernel``, ``MaternKernel``, ``ScaleKernel`` (+ the ``Kernel``
base they share).  Same constructor arguments, parameter names (``raw_lengthscale``,
``raw_outputscale``), constraints and call semantics as ``gpytorch/kernels/kernel.py:84-589``,
``rbf_kernel.py``, ``matern_kernel.py``, ``scale_kernel.py`` -- but ``forward`` returns a matrix-free
:class:`~gpytorch_amd.operators.FusedKernelLinearOperator`, exactly like the in-tree precedent
``gpytorch/kernels/keops/rbf_kernel.py:44-55`` returns a ``KernelLinearOperator``.
"""
from __future__ import annotations

import math

import torch

from . import backend as B
from .functions import KernelSpec
from .module import Interval, Module, Positive
from .module import AttrGetter, AttrSetter
from .operators import BatchLinearOperator, FusedKernelLinearOperator, LinearOperator


class Kernel(Module):
    has_lengthscale = False

    def __init__(self, ard_num_dims=None, batch_shape=torch.Size([]), active_dims=None, lengthscale_prior=None,
                 lengthscale_constraint=None, eps=1e-6, **kwargs):
        super().__init__()
        self._batch_shape = torch.Size(batch_shape)
        if active_dims is not None and not torch.is_tensor(active_dims):
            active_dims = torch.tensor(active_dims, dtype=torch.long)
        self.register_buffer("active_dims", active_dims)
        self.ard_num_dims = ard_num_dims
        self.eps = eps
        if self.has_lengthscale:
            n_ls = 1 if ard_num_dims is None else ard_num_dims
            self.register_parameter("raw_lengthscale", torch.nn.Parameter(torch.zeros(*self._batch_shape, 1, n_ls)))
            self.register_constraint("raw_lengthscale", Positive() if lengthscale_constraint is None else lengthscale_constraint)
            if lengthscale_prior is not None:
                self.register_prior("lengthscale_prior", lengthscale_prior, AttrGetter("lengthscale"), AttrSetter("_set_lengthscale"))

    @property
    def batch_shape(self):
        return self._batch_shape

    @property
    def dtype(self):
        """kernel.py:276-285."""
        if self.has_lengthscale:
            return self.lengthscale.dtype
        dtypes = {p.dtype for p in self.parameters()}
        if len(dtypes) > 1:
            raise RuntimeError(f"The kernel's parameters have multiple dtypes: {dtypes}.")
        return dtypes.pop() if dtypes else torch.get_default_dtype()

    @property
    def device(self):
        devices = {p.device for p in self.parameters()}
        if len(devices) > 1:
            raise RuntimeError(f"The kernel's parameters are on multiple devices: {devices}.")
        return devices.pop() if devices else torch.device("cpu")

    def named_sub_kernels(self):
        """Directly held member kernels (``kernel.py:405-414``; the list-holding compositions override ``__getitem__`` / ``expand_batch`` themselves)."""
        for name, module in self.named_children():
            if isinstance(module, Kernel):
                yield name, module

    def _batch_parameters(self):
        """Own parameters and those buffers that carry the batch shape (``active_dims`` is a buffer WITHOUT it)."""
        yield from self.named_parameters(recurse=False)
        nb = len(self._batch_shape)
        for name, buf in self.named_buffers(recurse=False):
            if buf is not None and name != "active_dims" and buf.dim() > nb and buf.shape[:nb] == self._batch_shape:
                yield name, buf

    def __getitem__(self, index):
        """``kernel.py:556-590``: the kernel of the indexed batch members -- every batch-shaped parameter indexed, the batch shape shortened by the
        dimensions the index removed, member kernels indexed the same way."""
        if len(self._batch_shape) == 0:
            return self
        import copy

        new = copy.deepcopy(self)
        index = index if isinstance(index, tuple) else (index,)
        for name, old in self._batch_parameters():
            t = getattr(new, name)
            t.data = t.data[index]
            new._batch_shape = t.shape[: len(self._batch_shape) - (old.dim() - t.dim())]
        for name, sub in self.named_sub_kernels():
            setattr(new, name, sub[index])
        return new

    def expand_batch(self, *sizes):
        """``kernel.py:354-403``: the same kernel with its parameters expanded to a larger batch shape."""
        if len(sizes) == 1 and hasattr(sizes[0], "__iter__"):
            new_shape = torch.Size(sizes[0])
        elif all(isinstance(v, int) for v in sizes):
            new_shape = torch.Size(sizes)
        else:
            raise RuntimeError(f"Invalid arguments {sizes} to expand_batch.")
        if new_shape == self._batch_shape:
            return self
        try:
            torch.broadcast_shapes(new_shape, self._batch_shape)
        except RuntimeError:
            raise RuntimeError(f"Cannot expand a kernel with batch shape {self._batch_shape} to new shape {new_shape}")
        import copy

        new = copy.deepcopy(self)
        nb = len(self._batch_shape)
        for name, old in self._batch_parameters():
            getattr(new, name).data = old.data.expand(*new_shape, *old.shape[nb:]).clone()
        new._batch_shape = new_shape
        for name, sub in self.named_sub_kernels():
            setattr(new, name, sub.expand_batch(new_shape))
        return new

    @property
    def lengthscale(self):
        return self._get_transformed("raw_lengthscale") if self.has_lengthscale else None

    @lengthscale.setter
    def lengthscale(self, value):
        self._set_lengthscale(value)

    def _set_lengthscale(self, value):
        if not self.has_lengthscale:
            raise RuntimeError("Kernel has no lengthscale.")
        self._set_transformed("raw_lengthscale", value)

    @property
    def is_stationary(self):
        return self.has_lengthscale

    def forward(self, x1, x2, diag=False, **params):
        raise NotImplementedError

    def __call__(self, x1, x2=None, diag=False, last_dim_is_batch=False, **params):
        """``kernel.py:454-534``: select active dims, promote 1-D inputs to [n, 1], default x2 = x1; leading dimensions of
        the inputs (and the kernel's ``batch_shape``) are batch dimensions (``kernel.py:163-208``)."""
        x1_, x2_ = x1, (None if x2 is x1 else x2)
        in_forward = last_dim_is_batch and getattr(self, "dims_as_batch_in_forward", False)
        if last_dim_is_batch and not in_forward:  # kernel.py:336-338: every input dimension becomes its own batch member, [..., d, n, 1]
            x1_ = x1_.transpose(-1, -2).unsqueeze(-1)
            x2_ = None if x2_ is None else x2_.transpose(-1, -2).unsqueeze(-1)
        if x1_.dim() == 1:
            x1_ = x1_.unsqueeze(1)
        if x2_ is not None and x2_.dim() == 1:
            x2_ = x2_.unsqueeze(1)
        if self.active_dims is not None:
            x1_ = x1_.index_select(-1, self.active_dims)
            if x2_ is not None:
                x2_ = x2_.index_select(-1, self.active_dims)
        if x2_ is None:
            x2_ = x1_
        elif x1_.shape[-1] != x2_.shape[-1]:
            raise RuntimeError("x1_ and x2_ must have the same number of dimensions!")
        if self.ard_num_dims is not None and self.ard_num_dims != x1_.shape[-1]:
            raise RuntimeError(f"Expected the input to have {self.ard_num_dims} dimensionality (based on ard_num_dims). Got {x1_.shape[-1]}.")
        if in_forward:      # (the stationary families scale by their per-dimension lengthscales first, as the reference's forward does)
            params["last_dim_is_batch"] = True
        return self.forward(x1_, x2_, diag=diag, **params)

    @property
    def prediction_strategy(self):
        from .models import DefaultPredictionStrategy

        return DefaultPredictionStrategy

    # ---- composition (kernels/kernel.py:563-589: ``+`` -> AdditiveKernel, ``*`` -> ProductKernel)
    def __add__(self, other):
        kernels = list(self.kernels) if isinstance(self, AdditiveKernel) else [self]
        kernels += list(other.kernels) if isinstance(other, AdditiveKernel) else [other]
        return AdditiveKernel(*kernels)

    def __mul__(self, other):
        kernels = list(self.kernels) if isinstance(self, ProductKernel) else [self]
        kernels += list(other.kernels) if isinstance(other, ProductKernel) else [other]
        return ProductKernel(*kernels)

    def _select(self, x):
        """Promote 1-D inputs and apply ``active_dims`` (the input handling of ``__call__``)."""
        x = x.unsqueeze(1) if x.dim() == 1 else x
        return x if self.active_dims is None else x.index_select(-1, self.active_dims)

    def rbf_features(self, x):
        """phi(x) with  k(x, x') = exp(-1/2 |phi(x) - phi(x')|^2)  for kernels of the squared-exponential family (RBF: x / l;
        Periodic: (cos, sin)(2 pi x / p) / sqrt(l); their products: concatenation), or None.  It lets compositions run on the
        fused RBF kernels: hyper-parameters reach the objective through phi, whose gradient is the fused input gradient."""
        return None


class _StationaryFused(Kernel):
    has_lengthscale = True
    kind = None

    def _shift(self, x1):
        # stationary kernel: any common shift is exact; centring keeps |z| small, which the Gram-form
        # generation kernel needs (the reference's sq_dist centres for the same reason, kernel.py:29-30)
        return x1.detach().mean(dim=-2)

    def _make_spec(self, x1, b=None, batch=None, num_dims=None):
        """Non-tensor description of the operator for batch member ``b`` (families with a shape parameter add it here).  ``num_dims``: the
        width of the whole input where the members are its single dimensions (``last_dim_is_batch``), else None."""
        return KernelSpec(self.kind, self._shift(x1))

    dims_as_batch_in_forward = True

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        # float32 with d <= 16: fused MFMA / VALU kernels; float64 or d > 16: generic path (backend.kv_chunked)
        ls = self.lengthscale
        same = x2 is x1
        nd = None
        if last_dim_is_batch:
            # rbf_kernel.py:78-81 + kernel.py:336-338 (deprecated in the reference, kept): the inputs are divided by the lengthscale of THEIR
            # dimension, then every dimension becomes a batch member [..., d, n, 1] -- so the lengthscales move to the batch with them
            nd = x1.shape[-1]
            x1 = x1.transpose(-1, -2).unsqueeze(-1)
            x2 = x1 if same else x2.transpose(-1, -2).unsqueeze(-1)
            ls = ls.expand(*ls.shape[:-1], nd).transpose(-1, -2).unsqueeze(-1)
        batch = torch.broadcast_shapes(x1.shape[:-2], x2.shape[:-2], ls.shape[:-2])
        if not batch:
            op = FusedKernelLinearOperator(x1, x2, self._make_spec(x1, num_dims=nd), ls)
            return op.diagonal() if diag else op
        # batch mode: one fused operator per batch member (inputs and lengthscales broadcast against each other)
        x1b = x1.expand(*batch, *x1.shape[-2:]).reshape(-1, *x1.shape[-2:])
        x2b = x1b if same else x2.expand(*batch, *x2.shape[-2:]).reshape(-1, *x2.shape[-2:])
        lsb = ls.expand(*batch, *ls.shape[-2:]).reshape(-1, *ls.shape[-2:])
        ops = []
        for b in range(x1b.shape[0]):
            xa = x1b[b]
            xb = xa if same else x2b[b]
            if nd is None:
                spec = self._make_spec(xa, b, batch)
            else:               # (shape parameters belong to the kernel's own batch: the dimension index is the last batch dimension)
                spec = self._make_spec(xa, b // nd, batch[:-1], num_dims=nd) if len(batch) > 1 else self._make_spec(xa, num_dims=nd)
            ops.append(FusedKernelLinearOperator(xa, xb, spec, lsb[b]))
        op = BatchLinearOperator(ops, batch)
        return op.diagonal() if diag else op


class RBFKernel(_StationaryFused):
    r"""k(x, x') = exp(-1/2 (x - x')^T Theta^-2 (x - x'))  (``gpytorch/kernels/rbf_kernel.py:14-85``)."""

    kind = "rbf"

    def rbf_features(self, x):
        return self._select(x) / self.lengthscale


def _unit_lengthscale(x):
    return torch.ones(1, 1, device=x.device, dtype=x.dtype)


def _feature_operator(f1, f2, same):
    """exp(-1/2 |f1_i - f2_j|^2) as a fused RBF operator with unit lengthscale over feature clouds (batch-aware)."""
    if f1.dim() == 2:
        f2 = f1 if same else f2
        return FusedKernelLinearOperator(f1, f2, KernelSpec("rbf", f1.detach().mean(dim=-2)), _unit_lengthscale(f1))
    batch = torch.broadcast_shapes(f1.shape[:-2], f2.shape[:-2])
    f1b = f1.expand(*batch, *f1.shape[-2:]).reshape(-1, *f1.shape[-2:])
    f2b = f1b if same else f2.expand(*batch, *f2.shape[-2:]).reshape(-1, *f2.shape[-2:])
    ops = [_feature_operator(f1b[b], f1b[b] if same else f2b[b], same) for b in range(f1b.shape[0])]
    return BatchLinearOperator(ops, batch)


def _feature_diag(f1, f2):
    """k(x1_i, x2_i) = exp(-1/2 |phi(x1_i) - phi(x2_i)|^2): the ``diag=True`` value for two DIFFERENT equally long inputs (kernels/kernel.py:318-330
    evaluates the elementwise diagonal, not the all-ones diagonal of K(x, x))."""
    return (f1 - f2).pow(2).sum(-1).mul(-0.5).exp()


def _cat_features(fs):
    """Feature maps of the members of a product side by side; members with and without a batch shape broadcast against each other."""
    batch = torch.broadcast_shapes(*[f.shape[:-1] for f in fs])
    return torch.cat([f.expand(*batch, f.shape[-1]) for f in fs], dim=-1)


class PeriodicKernel(Kernel):
    r"""k(x, x') = exp(-2 sum_q sin^2(pi (x_q - x'_q) / p_q) / l_q)   (``gpytorch/kernels/periodic_kernel.py:14-142``, the
    KeOps twin ``kernels/keops/periodic_kernel.py``).  Since sin^2(a - b) = (1 - cos 2(a - b)) / 2, the exponent is
    -1/2 |phi(x) - phi(x')|^2 with phi_q = (cos, sin)(2 pi x_q / p_q) / sqrt(l_q): a fused RBF operator over 2 d features
    (d <= 8 on the fused float32 kernels)."""

    has_lengthscale = True

    def __init__(self, period_length_prior=None, period_length_constraint=None, **kwargs):
        super().__init__(**kwargs)
        n_p = 1 if self.ard_num_dims is None else self.ard_num_dims
        self.register_parameter("raw_period_length", torch.nn.Parameter(torch.zeros(*self._batch_shape, 1, n_p)))
        self.register_constraint("raw_period_length", Positive() if period_length_constraint is None else period_length_constraint)
        if period_length_prior is not None:
            self.register_prior("period_length_prior", period_length_prior, AttrGetter("period_length"), AttrSetter("_set_period_length"))

    @property
    def period_length(self):
        return self._get_transformed("raw_period_length")

    @period_length.setter
    def period_length(self, value):
        self._set_period_length(value)

    def _set_period_length(self, value):
        self._set_transformed("raw_period_length", value)

    def rbf_features(self, x):
        x = self._select(x)
        a = x * (2.0 * math.pi / self.period_length)
        return torch.cat([a.cos(), a.sin()], dim=-1) / torch.cat([self.lengthscale.sqrt().expand_as(a[..., :1, :])] * 2, dim=-1)

    def forward(self, x1, x2, diag=False, **params):
        same = x2 is x1
        if diag:
            if same or (x1.shape == x2.shape and torch.equal(x1, x2)):
                return torch.ones(x1.shape[:-1], device=x1.device, dtype=x1.dtype)
            return _feature_diag(self.rbf_features(x1), self.rbf_features(x2))
        f1 = self.rbf_features(x1)
        return _feature_operator(f1, f1 if same else self.rbf_features(x2), same)

    def __call__(self, x1, x2=None, diag=False, **params):
        # active_dims are applied inside rbf_features (so that products can concatenate members with different active_dims)
        x2 = x1 if x2 is None else x2
        return self.forward(x1, x2, diag=diag, **params)


class MaternKernel(_StationaryFused):
    r"""Matern nu in {1/2, 3/2, 5/2} (``gpytorch/kernels/matern_kernel.py:14-110``); inputs are centred by
    the mean of x1 first, as the reference does (``matern_kernel.py:94-97``)."""

    def __init__(self, nu: float = 2.5, **kwargs):
        if nu not in {0.5, 1.5, 2.5}:
            raise RuntimeError("nu expected to be 0.5, 1.5, or 2.5")
        super().__init__(**kwargs)
        self.nu = nu

    @property
    def kind(self):
        return B.NU_TO_KIND[self.nu]

    def _shift(self, x1):
        return x1.detach().mean(dim=-2)


class RQKernel(_StationaryFused):
    r"""k(x, x') = (1 + (x - x')^T Theta^-2 (x - x') / (2 alpha))^-alpha   (``gpytorch/kernels/rq_kernel.py:14-86``).  A native
    covariance family of the fused float32 kernels (``KIND_RQ``: one ``v_log_f32`` + one ``v_exp_f32`` per pair) and of the float64 / d > 16
    generic path; alpha is a learnable shape parameter whose gradient comes out of the same derivative pass as the lengthscales'."""

    kind = "rq"

    def __init__(self, alpha_constraint=None, **kwargs):
        super().__init__(**kwargs)
        self.register_parameter("raw_alpha", torch.nn.Parameter(torch.zeros(*self._batch_shape, 1)))
        self.register_constraint("raw_alpha", Positive() if alpha_constraint is None else alpha_constraint)

    @property
    def alpha(self):
        return self._get_transformed("raw_alpha")

    @alpha.setter
    def alpha(self, value):
        self._set_transformed("raw_alpha", value)

    def _make_spec(self, x1, b=None, batch=None, num_dims=None):
        a = self.alpha
        if b is not None:
            a = a.expand(*batch, 1).reshape(-1, 1)[b]
        return KernelSpec("rq", self._shift(x1), param=a)


def pp_dense(r, code: int):
    """The piecewise-polynomial covariance of the distances ``r`` (in lengthscales) for the shape code 4 j + q, in autograd-visible torch ops (the
    small dense branches that differentiate through torch; the arithmetic of csrc/common.hpp PPShape)."""
    j, q = code >> 2, code & 3
    c2 = {2: B.pp_q2_c2(j), 3: (6 * j * j + 36 * j + 45) / 15.0}.get(q, 0.0)   # q = 2: the coefficient the reference executes
    c3 = (j ** 3 + 9 * j * j + 23 * j + 15) / 15.0 if q == 3 else 0.0
    c1 = float(j + q) if q else 0.0
    return (1.0 - r).clamp_min(0.0).pow(j + q) * (1.0 + r * (c1 + r * (c2 + r * c3)))


class PiecewisePolynomialKernel(_StationaryFused):
    r"""k(x, x') = max(1 - r, 0)^(j+q) P_q(r) with r = |Theta^-1 (x - x')|, q in {0, 1, 2, 3} and j = floor(D / 2) + q + 1
    (``gpytorch/kernels/piecewise_polynomial_kernel.py:11-28, 98-121``; Wendland's functions, Rasmussen & Williams eq. 4.21): EXACTLY zero beyond one
    lengthscale.  A native covariance family of the fused kernels (``KIND_PP``) whose products skip the tiles that hold nothing but zeros
    (``settings.compact_support_culling``: exact, on by default).

    P_2's quadratic coefficient is the one the reference's code evaluates, ``(j + 4 j + 3) / 3`` -- its docstring and the book say
    ``(j^2 + 4 j + 3) / 3``.  This library reproduces the reference's outputs; the coefficient lives in one named function per language
    (``pp_q2_c2`` in ``csrc/common.hpp`` for the kernels, ``backend.pp_q2_c2`` for the dense torch branch) for the day upstream changes it.

    D is the number of input dimensions after ``active_dims``; under ``last_dim_is_batch`` it is the original last dimension, as the reference
    computes it.  q and j are plain numbers: the kernel has no parameter beyond the lengthscale."""

    kind = "pp"

    def __init__(self, q: int = 2, **kwargs):
        super().__init__(**kwargs)
        if q not in {0, 1, 2, 3}:
            raise ValueError("q expected to be 0, 1, 2 or 3")
        self.q = q

    def shape_code(self, num_dims: int) -> int:
        """4 j + q for ``num_dims`` input dimensions: what the native layer receives as ``kparam``."""
        return B.pp_code(num_dims, self.q)

    def _make_spec(self, x1, b=None, batch=None, num_dims=None):
        # (dimensions as batch members: every member is one-dimensional, j keeps the dimension count of the whole input)
        return KernelSpec("pp", self._shift(x1), code=self.shape_code(x1.shape[-1] if num_dims is None else num_dims))


class ScaleKernel(Kernel):
    r"""K_scaled = outputscale * K_orig  (``gpytorch/kernels/scale_kernel.py:20-124``)."""

    def __init__(self, base_kernel, outputscale_prior=None, outputscale_constraint=None, **kwargs):
        if base_kernel.active_dims is not None:
            kwargs["active_dims"] = base_kernel.active_dims
        super().__init__(**kwargs)
        self.base_kernel = base_kernel
        self.register_parameter("raw_outputscale", torch.nn.Parameter(torch.zeros(self._batch_shape)))
        self.register_constraint("raw_outputscale", Positive() if outputscale_constraint is None else outputscale_constraint)
        if outputscale_prior is not None:
            self.register_prior("outputscale_prior", outputscale_prior, AttrGetter("outputscale"), AttrSetter("_set_outputscale"))

    @property
    def is_stationary(self):
        return self.base_kernel.is_stationary

    @property
    def outputscale(self):
        return self._get_transformed("raw_outputscale")

    @outputscale.setter
    def outputscale(self, value):
        self._set_outputscale(value)

    def _set_outputscale(self, value):
        self._set_transformed("raw_outputscale", value)

    def __call__(self, x1, x2=None, diag=False, **params):
        # active_dims were inherited from the base kernel: let the base kernel apply them once
        return self.forward(x1, x2, diag=diag, **params)

    def forward(self, x1, x2, diag=False, **params):
        orig = self.base_kernel(x1, x2, diag=diag, **params)
        os_ = self.outputscale
        if params.get("last_dim_is_batch", False):      # scale_kernel.py:110-112: the input dimensions became the LAST batch dimension
            os_ = os_.unsqueeze(-1)
        if diag:
            return orig * os_.unsqueeze(-1)
        if isinstance(orig, LinearOperator):  # scale_kernel.py:117-118: outputscale.view(*batch, 1, 1)
            return orig.mul(os_.reshape(1) if os_.numel() == 1 and not orig.batch_shape else os_)
        return orig * os_.reshape(*os_.shape, 1, 1)

    @property
    def prediction_strategy(self):
        return self.base_kernel.prediction_strategy


class MultiDeviceKernel(Kernel):
    r"""Constructor-compatible stand-in for ``gpytorch.kernels.MultiDeviceKernel`` (``kernels/multi_device_kernel.py:14-92``).

    The reference scatters row chunks of x1 over ``device_ids`` inside ONE process (``DataParallel``: module replicas re-created on
    every forward, peer copies of V on every product) and concatenates dense chunks.  Here multi-GPU means one process per GPU
    (``torchrun``; RCCL): the wrapped kernel returns the same fused operator as without the wrapper, and the operator shards its
    work at solve time -- probe columns of the MLL over ``settings.sharding.probe_group``, the few-column posterior solves by rows
    over ``settings.sharding.row_group`` (``distributed.py``).  Constructing this kernel in a process group of more than one rank
    installs the automatic layout policy over WORLD (``settings.sharding("auto")``, unless a sharding scope is already set): the closest
    equivalent of "allocate the covariance on these devices" -- the user names devices, never a probe-share x row-block grid; in a single
    process with several ``device_ids`` it warns once and runs on the inputs' device.
    The wrapped kernel is registered as ``module`` (the name ``DataParallel`` uses), so state-dict keys match the reference's."""

    def __init__(self, base_kernel, device_ids, output_device=None, create_cuda_context=True, **kwargs):
        super().__init__(**kwargs)
        self.module = base_kernel
        self.device_ids = list(device_ids)
        self.output_device = output_device if output_device is not None else (self.device_ids[0] if self.device_ids else None)
        import torch.distributed as dist

        from . import settings

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # process-global, like every setting here (and like the reference's settings): said out loud once, undone by `release()`.  The user of
            # the reference's MultiDeviceKernel names devices, not a layout: the "auto" policy of settings.sharding takes that role -- every MLL
            # evaluation picks its probe-share x row-block grid from (n, probes) (distributed.choose_grid), the posterior solves are row-sharded over WORLD
            import warnings

            self._installed = []
            if not settings.sharding._auto and settings.sharding._probe_group is None and settings.sharding._row_group is None \
                    and settings.sharding._mll_row_group is None:
                settings.sharding._auto = True
                self._installed = ["auto"]
                warnings.warn("gpytorch_amd.kernels.MultiDeviceKernel installed the WORLD process group with the automatic layout policy "
                              "(settings.sharding('auto')) for EVERY model of this process; MultiDeviceKernel.release() (or a settings.sharding(...) "
                              "scope) undoes it.", RuntimeWarning)
        elif len(self.device_ids) > 1:
            import warnings

            warnings.warn("gpytorch_amd.kernels.MultiDeviceKernel: multi-GPU runs are one process per GPU (torchrun + settings.sharding); "
                          "this single process evaluates the kernel on the device of its inputs.", RuntimeWarning)

    def release(self):
        """Take back the process groups this constructor installed in ``settings.sharding`` (no-op if it installed none)."""
        from . import settings

        if getattr(self, "_installed", []):
            settings.sharding._auto = False
        self._installed = []

    @property
    def base_kernel(self):
        return self.module

    @property
    def is_stationary(self):
        return self.module.is_stationary

    def __call__(self, x1, x2=None, diag=False, **params):
        return self.forward(x1, x2, diag=diag, **params)     # (the wrapped kernel applies its own active_dims)

    def forward(self, x1, x2, diag=False, **params):
        return self.module(x1, x2, diag=diag, **params)

    def num_outputs_per_input(self, x1, x2):
        f = getattr(self.module, "num_outputs_per_input", None)
        return 1 if f is None else f(x1, x2)

    @property
    def prediction_strategy(self):
        return self.module.prediction_strategy


def _index_members(kernel, index):
    """``kernel.py:626-631`` / ``:684-688``: a sum / product of kernels indexes every member."""
    import copy

    new = copy.deepcopy(kernel)
    for i, member in enumerate(kernel.kernels):
        new.kernels[i] = member[index]
    return new


class AdditiveKernel(Kernel):
    """K = sum_i K_i (``kernels/kernel.py:592-632``): the members stay matrix-free; their sum is a
    :class:`~gpytorch_amd.operators.SumFusedLinearOperator` whose products, solves and log-determinants add the members'
    fused products."""

    def __init__(self, *kernels):
        super().__init__()
        self.kernels = torch.nn.ModuleList(kernels)

    @property
    def is_stationary(self):
        return all(k.is_stationary for k in self.kernels)

    def __getitem__(self, index):
        return _index_members(self, index)

    def __call__(self, x1, x2=None, diag=False, **params):
        return self.forward(x1, x1 if x2 is None else x2, diag=diag, **params)

    def forward(self, x1, x2, diag=False, **params):
        from .composite import SumFusedLinearOperator

        terms = [k(x1, x2, diag=diag, **params) for k in self.kernels]
        if diag:
            return sum(terms[1:], terms[0])
        return SumFusedLinearOperator.of(terms)


def _se_family(kernel):
    """(feature function, outputscale or None) if ``kernel`` is a product of squared-exponential-family members, else None."""
    if isinstance(kernel, ScaleKernel):
        inner = _se_family(kernel.base_kernel)
        if inner is None:
            return None
        return inner[0], (kernel.outputscale if inner[1] is None else kernel.outputscale * inner[1])
    if isinstance(kernel, ProductKernel):
        parts = [_se_family(k) for k in kernel.kernels]
        if any(p is None for p in parts):
            return None
        scale = None
        for _, sc in parts:
            if sc is not None:
                scale = sc if scale is None else scale * sc
        return (lambda x, parts=parts: _cat_features([f(x) for f, _ in parts])), scale
    if kernel.rbf_features.__func__ is not Kernel.rbf_features:
        return kernel.rbf_features, None
    return None


def stationary_dense(kind: str, d2):
    """RBF / Matern covariance of the squared scaled distances ``d2`` (x / lengthscale, no family constant folded in) in autograd-visible torch ops."""
    if kind == "rbf":
        return torch.exp(-0.5 * d2)
    nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind]
    r = (d2 + 1e-20).sqrt() * (2 * nu) ** 0.5
    e = torch.exp(-r)
    return e if nu == 0.5 else ((1 + r) * e if nu == 1.5 else (1 + r + r * r / 3) * e)


class ProductFactors:
    """What ``product_factors`` recognised: the two members in CANONICAL order (A: the lower family id, for equal families the fewer columns), the
    code K_A + 4 K_B + 16 D_A, and the product of the outputscales of every peeled ScaleKernel (None: no ScaleKernel)."""

    def __init__(self, a, b, da: int, db: int, scale):
        self.a, self.b, self.da, self.db, self.scale = a, b, da, db, scale
        self.ka, self.kb = B.KIND_IDS[a.kind], B.KIND_IDS[b.kind]
        self.code = B.prod_code(self.ka, self.kb, da)

    def gather(self, x):
        """The cloud the fused operator sees: the columns of A, then the columns of B (gathered, not partitioned: the groups may overlap)."""
        return torch.cat([self.a._select(x), self.b._select(x)], dim=-1)

    def lengthscale(self):
        """One lengthscale per gathered column, [1, D_A + D_B]; differentiable, so the per-dimension gradient of the fused operator reaches each
        member's ``raw_lengthscale`` through autograd (a single lengthscale receives the sum over its columns)."""
        return torch.cat([self.a.lengthscale.expand(1, self.da), self.b.lengthscale.expand(1, self.db)], dim=-1)


def _product_leaves(kernel):
    """Nested ProductKernels flattened and ScaleKernels peeled: (leaf kernels, list of outputscales), or None where a wrapper carries a batch shape."""
    if isinstance(kernel, ScaleKernel):
        if len(kernel.batch_shape):
            return None
        inner = _product_leaves(kernel.base_kernel)
        return None if inner is None else (inner[0], inner[1] + [kernel.outputscale])
    if isinstance(kernel, ProductKernel):
        leaves, scales = [], []
        for k in kernel.kernels:
            inner = _product_leaves(k)
            if inner is None:
                return None
            leaves += inner[0]
            scales += inner[1]
        return leaves, scales
    return [kernel], []


def product_factors(kernel, x1, x2=None, last_dim_is_batch=False):
    """The matrix-free form of a product of two stationary families, or None.  Pure: it looks at the kernel's structure and at the shapes and
    dtypes of the inputs, never at the device.

    Accepted: after flattening nested ``ProductKernel``s and peeling ``ScaleKernel``s (their outputscales multiply into one), exactly two members,
    each an ``RBFKernel`` or a ``MaternKernel``, not both RBF; no batch shape on any kernel or input; no ``last_dim_is_batch``; float32 inputs; each
    member sees 1..3 columns after its ``active_dims`` (the two groups may overlap or coincide).  Products of the squared-exponential family keep
    their own path (``_se_family`` comes first)."""
    if last_dim_is_batch or _se_family(kernel) is not None:
        return None
    flat = _product_leaves(kernel)
    if flat is None or len(flat[0]) != 2:
        return None
    leaves, scales = flat
    if any(type(k) not in (RBFKernel, MaternKernel) or len(k.batch_shape) for k in leaves) or all(type(k) is RBFKernel for k in leaves):
        return None
    x2 = x1 if x2 is None else x2
    if x1.dim() > 2 or x2.dim() > 2 or x1.dtype != torch.float32 or x2.dtype != torch.float32:
        return None
    width = 1 if x1.dim() == 1 else x1.shape[-1]
    if (1 if x2.dim() == 1 else x2.shape[-1]) != width:
        return None
    dims = []
    for k in leaves:
        nd = width if k.active_dims is None else int(k.active_dims.numel())
        if k.active_dims is not None and (int(k.active_dims.max()) >= width or int(k.active_dims.min()) < -width):
            return None      # (the member's own call raises the index error)
        if not 1 <= nd <= B.PROD_MAX_FACTOR_DIM or (k.ard_num_dims is not None and k.ard_num_dims != nd):
            return None
        dims.append(nd)
    order = sorted((0, 1), key=lambda i: (B.KIND_IDS[leaves[i].kind], dims[i]))   # (stable: full ties keep the user's order, the code is the same)
    scale = None
    for sc in scales:
        scale = sc if scale is None else scale * sc
    return ProductFactors(leaves[order[0]], leaves[order[1]], dims[order[0]], dims[order[1]], scale)


def sm_dense(x1, x2, weights, means, scales, diag=False, last_dim_is_batch=False):
    """The spectral-mixture covariance as the reference executes it (``gpytorch/kernels/spectral_mixture_kernel.py:309-354``: the sum over the mixtures
    BEFORE the product over the dimensions) in autograd-visible torch ops, any dtype, any batch shape: x1 [..., n, d], x2 [..., m, d], weights [..., Q],
    means / scales [..., Q, 1, d].  Returns [..., n, m] ([..., n] with ``diag``); with ``last_dim_is_batch`` the per-dimension factors as the last batch
    dimension, [..., d, n, m] ([..., d, n]), as the reference's permute leaves them."""
    x1_, x2_ = x1.unsqueeze(-3), x2.unsqueeze(-3)                    # [..., 1, n, d]
    if diag:
        tau, sc, mu = x1_ - x2_, scales, means                       # [..., 1, n, d]; [..., Q, 1, d]
    else:
        tau, sc, mu = x1_.unsqueeze(-2) - x2_.unsqueeze(-3), scales.unsqueeze(-2), means.unsqueeze(-2)   # [..., 1, n, m, d]; [..., Q, 1, 1, d]
    res = torch.exp(-2.0 * math.pi ** 2 * (tau * sc).square()) * torch.cos(2.0 * math.pi * tau * mu)
    w = weights.reshape(*weights.shape, 1, 1)
    res = (res * (w if diag else w.unsqueeze(-2))).sum(-3 if diag else -4)     # [..., n, d] / [..., n, m, d]
    if last_dim_is_batch:
        return res.movedim(-1, -2) if diag else res.movedim(-1, -3)
    return res.prod(-1)


def sm_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free (native ``"sm"``) form applies to this call of a ``SpectralMixtureKernel``.  Pure: it looks at the kernel's shapes and dtypes and
    at those of the inputs, never at the device.  All of: float32 parameters and inputs; no batch shape on the kernel or the inputs; no
    ``last_dim_is_batch``; (Q, d) inside the native envelope (``backend.sm_envelope_ok``: d <= 3, Q <= 8 at d = 1, Q <= 4 at d = 2, 3).  Everything else
    takes the dense branch (``sm_dense`` under plain autograd)."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() > 2 or x2.dim() > 2:
        return False
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or kernel.raw_mixture_weights.dtype != torch.float32:
        return False
    d = 1 if x1.dim() == 1 else x1.shape[-1]
    return d == kernel.ard_num_dims and B.sm_envelope_ok(kernel.num_mixtures, d)


class SpectralMixtureKernel(Kernel):
    r"""k(x, x') = prod_j sum_q w_q exp(-2 pi^2 sigma_qj^2 tau_j^2) cos(2 pi mu_qj tau_j), tau = x - x'
    (``gpytorch/kernels/spectral_mixture_kernel.py:24-354``, AS EXECUTED: the sum over mixtures comes before the product over dimensions; for d = 1 this
    is Wilson & Adams' kernel).  Parameter names, shapes, default ``Positive()`` constraints, setters and ``initialize_from_data`` are the reference's;
    ``initialize_from_data_empspect`` (scikit-learn) is not provided.

    float32, no batches, (Q, d) within d <= 3, Q <= 8 (d = 1) / Q <= 4 (d = 2, 3): ONE matrix-free operator of the native family ``"sm"``
    (``sm_native`` has the rule; csrc/kv_directsm.hpp the kernel) -- the reference materialises a Q x n x m x d tensor.  The operator evaluates
    k / Wsum^d, Wsum = sum_q w_q; Wsum^d rides in its outputscale slot and theta = [w | mu | sigma] in its learnable-parameter slot, both differentiable.
    Anything else -- float64, batches, ``last_dim_is_batch``, ``diag=True`` of two different inputs, larger Q d -- is formed densely by ``sm_dense``."""

    is_stationary = True
    dims_as_batch_in_forward = True   # (``last_dim_is_batch`` is handled by forward, as in the reference)

    def __init__(self, num_mixtures=None, ard_num_dims=1, batch_shape=torch.Size([]), mixture_scales_prior=None, mixture_scales_constraint=None,
                 mixture_means_prior=None, mixture_means_constraint=None, mixture_weights_prior=None, mixture_weights_constraint=None, **kwargs):
        if num_mixtures is None:
            raise RuntimeError("num_mixtures is a required argument")
        if mixture_means_prior is not None or mixture_scales_prior is not None or mixture_weights_prior is not None:
            import warnings

            warnings.warn("Priors not implemented for SpectralMixtureKernel")
        super().__init__(ard_num_dims=ard_num_dims, batch_shape=batch_shape, **kwargs)   # (this kernel does not use the default lengthscale)
        self.num_mixtures = num_mixtures
        self.register_parameter("raw_mixture_weights", torch.nn.Parameter(torch.zeros(*self._batch_shape, num_mixtures)))
        ms_shape = torch.Size([*self._batch_shape, num_mixtures, 1, self.ard_num_dims])
        self.register_parameter("raw_mixture_means", torch.nn.Parameter(torch.zeros(ms_shape)))
        self.register_parameter("raw_mixture_scales", torch.nn.Parameter(torch.zeros(ms_shape)))
        self.register_constraint("raw_mixture_scales", Positive() if mixture_scales_constraint is None else mixture_scales_constraint)
        self.register_constraint("raw_mixture_means", Positive() if mixture_means_constraint is None else mixture_means_constraint)
        self.register_constraint("raw_mixture_weights", Positive() if mixture_weights_constraint is None else mixture_weights_constraint)

    @property
    def mixture_scales(self):
        return self._get_transformed("raw_mixture_scales")

    @mixture_scales.setter
    def mixture_scales(self, value):
        self._set_mixture_scales(value)

    def _set_mixture_scales(self, value):
        self._set_transformed("raw_mixture_scales", value)

    @property
    def mixture_means(self):
        return self._get_transformed("raw_mixture_means")

    @mixture_means.setter
    def mixture_means(self, value):
        self._set_mixture_means(value)

    def _set_mixture_means(self, value):
        self._set_transformed("raw_mixture_means", value)

    @property
    def mixture_weights(self):
        return self._get_transformed("raw_mixture_weights")

    @mixture_weights.setter
    def mixture_weights(self, value):
        self._set_mixture_weights(value)

    def _set_mixture_weights(self, value):
        self._set_transformed("raw_mixture_weights", value)

    def initialize_from_data(self, train_x, train_y, **kwargs):
        """``spectral_mixture_kernel.py:219-269``: scales ~ 1 / |N(0, max_dist^2)|, means ~ U(0, 0.5 / min_dist), weights = std(y) / Q."""
        with torch.no_grad():
            if not torch.is_tensor(train_x) or not torch.is_tensor(train_y):
                raise RuntimeError("train_x and train_y should be tensors")
            if train_x.ndimension() == 1:
                train_x = train_x.unsqueeze(-1)
            if self.active_dims is not None:
                train_x = train_x[..., self.active_dims]
            train_x_sort = train_x.sort(dim=-2)[0]
            max_dist = train_x_sort[..., -1, :] - train_x_sort[..., 0, :]
            dists = train_x_sort[..., 1:, :] - train_x_sort[..., :-1, :]
            dists = torch.where(dists.eq(0.0), torch.tensor(1.0e10, dtype=train_x.dtype, device=train_x.device), dists)   # (no zero minimum distance)
            min_dist = dists.sort(dim=-2)[0][..., 0, :]
            # a singleton data dimension (-2) and one for the mixtures (-3); then compress what corresponds to singletons of the parameters
            min_dist, max_dist = min_dist.unsqueeze(-2).unsqueeze(-3), max_dist.unsqueeze(-2).unsqueeze(-3)
            dim = -3
            while -dim <= min_dist.dim():
                if -dim > self.raw_mixture_scales.dim():
                    min_dist, max_dist = min_dist.min(dim=dim)[0], max_dist.max(dim=dim)[0]
                elif self.raw_mixture_scales.size(dim) == 1:
                    min_dist, max_dist = min_dist.min(dim=dim, keepdim=True)[0], max_dist.max(dim=dim, keepdim=True)[0]
                    dim -= 1
                else:
                    dim -= 1
            self.mixture_scales = torch.randn_like(self.raw_mixture_scales).mul_(max_dist).abs_().reciprocal_()
            self.mixture_means = torch.rand_like(self.raw_mixture_means).mul_(0.5).div(min_dist)
            self.mixture_weights = train_y.std().div(self.num_mixtures)

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        num_dims = x1.shape[-1]
        if not num_dims == self.ard_num_dims:
            raise RuntimeError("The SpectralMixtureKernel expected the input to have {} dimensionality (based on the ard_num_dims argument). Got {}."
                               .format(self.ard_num_dims, num_dims))
        w, mu, sigma = self.mixture_weights, self.mixture_means, self.mixture_scales
        same = x2 is x1
        if sm_native(self, x1, x2, last_dim_is_batch) and not (diag and not same):
            scale = w.sum() ** num_dims
            if diag:   # k(x, x) = Wsum^d: no launch
                return torch.ones(x1.shape[0], device=x1.device, dtype=x1.dtype) * scale
            spec = KernelSpec("sm", x1.detach().mean(dim=-2), param=B.sm_theta(w, mu, sigma))
            ones = torch.ones(1, num_dims, device=x1.device, dtype=x1.dtype)   # the lengthscale slot: ones, no gradient
            return FusedKernelLinearOperator(x1, x2, spec, ones, scale.reshape(1))
        from .operators import DenseLinearOperator

        res = sm_dense(x1, x2, w, mu, sigma, diag=diag, last_dim_is_batch=last_dim_is_batch)
        return res if diag else DenseLinearOperator(res)


def rbfgrad_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free form (``derivative.RBFGradFusedLinearOperator``) applies to this call of an ``RBFKernelGrad``.  All of: float32 parameters and
    inputs; inputs on the device, without ``requires_grad``; no batch shape on the kernel or the inputs; no ``last_dim_is_batch``; 1..4 input
    dimensions (``backend.RBFGRAD_MAX_DIM``).  Everything else -- float64 models, batches, d > 4, gradients with respect to the inputs, host tensors --
    takes the dense branch (``derivative.rbfgrad_dense`` under plain autograd)."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() > 2 or x2.dim() > 2:
        return False
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or kernel.raw_lengthscale.dtype != torch.float32:
        return False
    if x1.requires_grad or x2.requires_grad or x1.device.type != "cuda" or x2.device.type != "cuda":
        return False
    d = 1 if x1.dim() == 1 else x1.shape[-1]
    return 1 <= d <= B.RBFGRAD_MAX_DIM


class RBFKernelGrad(_StationaryFused):
    r"""The RBF kernel over function values and their gradients (``gpytorch/kernels/rbf_kernel_grad.py:14-118``): for n points in d dimensions
    an n (d + 1) x n (d + 1) covariance in the multitask ordering -- row i (d + 1) + a is the value (a = 0) or the a-th partial derivative of
    point i.  Used with ``means.ConstantMeanGrad``, ``MultitaskMultivariateNormal`` and ``MultitaskGaussianLikelihood(num_tasks=d + 1)``.

    float32 on the device, d <= 4, no batches, inputs without ``requires_grad``: ONE matrix-free operator (``rbfgrad_native`` has the rule;
    csrc/kv_rbfgrad.hpp the kernel) -- the reference materialises the matrix.  Anything else is formed densely by ``derivative.rbfgrad_dense``.
    ``diag=True`` is the reference's: value entries 1, derivative entries 1 / l_a^2, and an error unless x1 == x2.

    (Derived from the stationary base, not from ``RBFKernel``: the rules by which ``ProductKernel`` recognises squared-exponential members and
    two-factor products look at ``RBFKernel`` and must not take a kernel whose matrix has d + 1 rows per point.)"""

    kind = "rbf"
    dims_as_batch_in_forward = False   # (``last_dim_is_batch``: the base class turns the dimensions into batch members, as the reference does)

    def forward(self, x1, x2, diag=False, **params):
        from .derivative import RBFGradFusedLinearOperator, rbfgrad_dense

        if diag:
            return rbfgrad_dense(x1, x2, self.lengthscale, diag=True)
        if rbfgrad_native(self, x1, x2, params.get("last_dim_is_batch", False)):
            return RBFGradFusedLinearOperator(x1, x2, self.lengthscale)
        from .operators import DenseLinearOperator

        return DenseLinearOperator(rbfgrad_dense(x1, x2, self.lengthscale))

    def num_outputs_per_input(self, x1, x2):
        return x1.size(-1) + 1


def matern52grad_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free form (``derivative.Matern52GradFusedLinearOperator``) applies to this call of a ``Matern52KernelGrad``: the conditions of
    ``rbfgrad_native`` -- float32 parameters and inputs; inputs on the device, without ``requires_grad``; no batch; 1..4 input dimensions.
    Everything else takes the dense branch (``derivative.matern52grad_dense`` under plain autograd)."""
    return rbfgrad_native(kernel, x1, x2, last_dim_is_batch)


class Matern52KernelGrad(_StationaryFused):
    r"""The Matern-5/2 kernel over function values and their gradients (``gpytorch/kernels/matern52_kernel_grad.py:16-196``): the twin of
    ``RBFKernelGrad`` for priors that are twice, not infinitely, differentiable -- same n (d + 1) x n (d + 1) multitask ordering, same companions
    (``means.ConstantMeanGrad``, ``MultitaskMultivariateNormal``, ``MultitaskGaussianLikelihood(num_tasks=d + 1)``).  A ``nu`` keyword is accepted
    and dropped, as in the reference: nu is 2.5.

    float32 on the device, d <= 4, no batches, inputs without ``requires_grad``: ONE matrix-free operator (``matern52grad_native`` has the rule;
    csrc/kv_rbfgrad.hpp, family KRG_M52, the kernel) -- the reference materialises the matrix.  Anything else is formed densely by
    ``derivative.matern52grad_dense``.  ``diag=True`` is the reference's: value entries 1, derivative entries (5/3) / l_a^2, and an error unless
    x1 == x2.

    (Derived from the stationary base, not from ``MaternKernel``, for the reason ``RBFKernelGrad`` is not an ``RBFKernel``: the rules that recognise
    Matern members of products must not take a kernel whose matrix has d + 1 rows per point.)"""

    kind = "matern52"
    nu = 2.5
    dims_as_batch_in_forward = False

    def __init__(self, **kwargs):
        kwargs.pop("nu", None)
        super().__init__(**kwargs)

    def forward(self, x1, x2, diag=False, **params):
        from .derivative import Matern52GradFusedLinearOperator, matern52grad_dense

        if diag:
            return matern52grad_dense(x1, x2, self.lengthscale, diag=True)
        if matern52grad_native(self, x1, x2, params.get("last_dim_is_batch", False)):
            return Matern52GradFusedLinearOperator(x1, x2, self.lengthscale)
        from .operators import DenseLinearOperator

        return DenseLinearOperator(matern52grad_dense(x1, x2, self.lengthscale))

    def num_outputs_per_input(self, x1, x2):
        return x1.size(-1) + 1


def rbfgradgrad_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free form (``derivative.RBFGradGradFusedLinearOperator``) applies to this call of an ``RBFKernelGradGrad``: the conditions of
    ``rbfgrad_native`` -- float32 parameters and inputs; inputs on the device, without ``requires_grad``; no batch; 1..4 input dimensions.
    Everything else takes the dense branch (``derivative.rbfgradgrad_dense`` under plain autograd)."""
    return rbfgrad_native(kernel, x1, x2, last_dim_is_batch)


class RBFKernelGradGrad(_StationaryFused):
    r"""The RBF kernel over function values, their gradients and their non-mixed second derivatives (``gpytorch/kernels/rbf_kernel_gradgrad.py:14-169``):
    for n points in d dimensions an n (2 d + 1) x n (2 d + 1) covariance in the multitask ordering -- row i (2 d + 1) + c is the value (c = 0), the
    c-th partial derivative (1 <= c <= d) or the second derivative d2/dx_{c-d}^2 (c > d) of point i: curvature and Laplacian data, PDE-constrained
    regression.  Used with ``means.ConstantMeanGradGrad``, ``MultitaskMultivariateNormal`` and ``MultitaskGaussianLikelihood(num_tasks=2 d + 1)``.

    float32 on the device, d <= 4, no batches, inputs without ``requires_grad``: ONE matrix-free operator (``rbfgradgrad_native`` has the rule;
    csrc/kv_rbfgradgrad.hpp the kernel) -- the reference materialises the matrix, and its ``forward`` fails for n1 != n2; here the rectangular
    train x test block is the same formula.  Anything else is formed densely by ``derivative.rbfgradgrad_dense``.  ``diag=True`` is the
    reference's: 1, 1 / l_a^2, 3 / l_a^4, and an error unless x1 == x2.

    (Derived from the stationary base, not from ``RBFKernel``, for the reason ``RBFKernelGrad`` gives: the rules that recognise squared-exponential
    members of products must not take a kernel whose matrix has 2 d + 1 rows per point.)"""

    kind = "rbf"
    dims_as_batch_in_forward = False

    def forward(self, x1, x2, diag=False, **params):
        from .derivative import RBFGradGradFusedLinearOperator, rbfgradgrad_dense

        if diag:
            return rbfgradgrad_dense(x1, x2, self.lengthscale, diag=True)
        if rbfgradgrad_native(self, x1, x2, params.get("last_dim_is_batch", False)):
            return RBFGradGradFusedLinearOperator(x1, x2, self.lengthscale)
        from .operators import DenseLinearOperator

        return DenseLinearOperator(rbfgradgrad_dense(x1, x2, self.lengthscale))

    def num_outputs_per_input(self, x1, x2):
        return 2 * x1.size(-1) + 1


class ProductKernel(Kernel):
    """K = prod_i K_i elementwise (``kernels/kernel.py:634-688``).  Two forms are matrix-free:

    * products of squared-exponential-family members (RBF, Periodic, their ScaleKernels): ONE fused RBF operator over the concatenated feature
      maps -- exact, at most 16 feature dimensions;
    * otherwise, the product of exactly TWO members, each an ``RBFKernel`` or ``MaternKernel`` (ScaleKernels peeled, nested products flattened), on
      float32 inputs without batch dimensions, each member seeing 1..3 columns after its ``active_dims`` (overlapping groups are fine: the columns
      are gathered): ONE fused operator of the native product family (``spec.kind == "prod"``; ``product_factors`` has the rule) over the cloud
      ``[x[:, dims_A] | x[:, dims_B]]``.  Hyper-parameter gradients reach both members' lengthscales and every outputscale; gradients with respect
      to the inputs are not provided.

    Any other product -- Periodic / RQ / piecewise-polynomial members next to a Matern, three or more non-SE factors, float64, batches, more than
    three columns in a factor, ``last_dim_is_batch`` -- is formed densely (the reference, too, densifies whenever x1 != x2) and is meant for small
    problems."""

    def __init__(self, *kernels):
        super().__init__()
        self.kernels = torch.nn.ModuleList(kernels)

    @property
    def is_stationary(self):
        return all(k.is_stationary for k in self.kernels)

    def __getitem__(self, index):
        return _index_members(self, index)

    def __call__(self, x1, x2=None, diag=False, **params):
        return self.forward(x1, x1 if x2 is None else x2, diag=diag, **params)

    def forward(self, x1, x2, diag=False, **params):
        fam = _se_family(self)
        if fam is not None:
            feat, scale = fam
            same = x2 is x1
            if diag:
                if same or (x1.shape == x2.shape and torch.equal(x1, x2)):
                    one = torch.ones(x1.shape[:-1] if x1.dim() > 1 else x1.shape, device=x1.device, dtype=x1.dtype)
                else:     # two different inputs: the elementwise diagonal (test/kernels/test_additive_and_product_kernels.py:127-157)
                    one = _feature_diag(feat(x1), feat(x2))
                return one if scale is None else one * scale.unsqueeze(-1)
            f1 = feat(x1)
            if f1.shape[-1] <= B.MAX_INPUT_DIM or f1.dtype == torch.float64:
                op = _feature_operator(f1, f1 if same else feat(x2), same)
                return op if scale is None else op.mul(scale.reshape(1) if scale.numel() == 1 and not op.batch_shape else scale)
        pf = None if fam is not None else product_factors(self, x1, x2, params.get("last_dim_is_batch", False))
        same = x2 is x1
        if pf is not None and not (diag and not same):   # (the diagonal of two different inputs: the members' elementwise diagonals, below)
            if diag:
                one = torch.ones(x1.shape[:1], device=x1.device, dtype=x1.dtype)
                return one if pf.scale is None else one * pf.scale.reshape(())
            g1 = pf.gather(x1)
            g2 = g1 if same else pf.gather(x2)
            spec = KernelSpec("prod", g1.detach().mean(dim=-2), code=pf.code)
            return FusedKernelLinearOperator(g1, g2, spec, pf.lengthscale(), None if pf.scale is None else pf.scale.reshape(1))
        from .operators import DenseLinearOperator, to_dense

        res = None
        for k in self.kernels:
            term = k(x1, x2, diag=diag, **params)
            term = term if diag else to_dense(term)
            res = term if res is None else res * term
        return res if diag else DenseLinearOperator(res)


def _additive_base(kernel):
    """(base, outputscale or None) of an ``AdditiveStructureKernel`` whose base kernel is exactly an ``RBFKernel`` or a ``MaternKernel``, optionally
    inside ONE ``ScaleKernel`` without batch shape (peeled: its outputscale is returned); None for anything else."""
    base, scale = kernel.base_kernel, None
    if type(base) is ScaleKernel:
        if len(base.batch_shape):
            return None
        base, scale = base.base_kernel, base.outputscale
    if type(base) not in (RBFKernel, MaternKernel) or len(base.batch_shape) or base.active_dims is not None:
        return None
    return base, scale


def additive_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free (native ``"add"``) form applies to this call of an ``AdditiveStructureKernel``.  Pure: it looks at the kernel's structure and at
    the shapes and dtypes of the inputs, never at the device.  All of: float32 parameters and inputs; no batch shape on the kernel or the inputs; no
    ``last_dim_is_batch``; 2 <= d <= 8 and d == ``num_dims``; the base kernel exactly an ``RBFKernel`` or a ``MaternKernel``, optionally inside one
    ``ScaleKernel`` with an unbatched outputscale; a lengthscale shaped [1, 1] or [1, d]; inputs without ``requires_grad`` (the native family has no
    input gradients).  Everything else takes the dense branch (``additive_dense`` under plain autograd)."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return False
    found = _additive_base(kernel)
    if found is None:
        return False
    base, scale = found
    ls = base.raw_lengthscale
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or ls.dtype != torch.float32 or (scale is not None and scale.dtype != torch.float32):
        return False
    if x1.requires_grad or x2.requires_grad:
        return False
    d = x1.shape[-1]
    if not (B.ADD_MIN_DIM <= d <= B.ADD_MAX_DIM and d == kernel.num_dims and x2.shape[-1] == d):
        return False
    return tuple(ls.shape) in ((1, 1), (1, d))


def _ski_additive_base(kernel):
    """(grid kernel, outer outputscale or None) of an ``AdditiveStructureKernel`` over a ``GridInterpolationKernel`` with ``num_dims == 1``, bare or
    inside ONE unbatched ``ScaleKernel``; None for anything else."""
    base, scale = kernel.base_kernel, None
    if type(base) is ScaleKernel:
        if len(base.batch_shape):
            return None
        base, scale = base.base_kernel, base.outputscale
    if type(base) is not GridInterpolationKernel or base.num_dims != 1 or base.active_dims is not None:
        return None
    return base, scale


def ski_additive_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free additive KISS-GP form (ONE ``ski.SKIFusedLinearOperator`` on the concatenation of d one-dimensional axes) applies to this call
    of an ``AdditiveStructureKernel``.  All of: the base is a ``GridInterpolationKernel`` with ``num_dims == 1``, bare or inside ONE unbatched
    ``ScaleKernel`` (its outputscale becomes the operator's ``scale``); ``ski.columns_native`` of the grid kernel's base kernel, with one
    lengthscale or d of them (a Periodic base only with ONE lengthscale and period); float32 inputs and grid, on the device, without
    ``requires_grad`` and without a batch shape; no ``last_dim_is_batch``; 2 <= d <= 16 and d == ``num_dims`` of the additive kernel; at least 4
    grid nodes (fewer is a ``ValueError`` at construction) and at most 2^24 in all.  Everything else takes ``additive_dense``."""
    from .ski import _innermost, columns_native

    x2 = x1 if x2 is None else x2
    found = _ski_additive_base(kernel)
    if found is None or last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return False
    gk, scale = found
    if not columns_native(gk.base_kernel):
        return False
    axis = gk.grid[0]
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or axis.dtype != torch.float32 or (scale is not None and scale.dtype != torch.float32):
        return False
    if x1.requires_grad or x2.requires_grad or x1.device.type != "cuda" or x2.device.type != "cuda":
        return False
    d, m = x1.shape[-1], int(axis.numel())
    if not (B.SKI_ADD_MIN_DIM <= d <= B.SKI_ADD_MAX_DIM and d == kernel.num_dims and x2.shape[-1] == d and m >= 4 and d * m <= B.SKI_MAX_NODES):
        return False
    inner = _innermost(gk.base_kernel)
    k = inner.lengthscale.numel()
    if type(inner) is PeriodicKernel:
        return k == 1 and inner.period_length.numel() == 1
    return k in (1, d)


def _gram_sq_dist(x1, x2, same):
    """Squared distances as the reference forms them (``gpytorch/kernels/kernel.py:26-49``): x1 centred, the quadratic expansion as ONE matrix product
    of [-2 x1 | |x1|^2 | 1] with [x2 | 1 | |x2|^2], clamped at zero; identical inputs that need no gradient share the operands and get an exactly zero
    diagonal.  ``additive_dense`` restates it so that the dense branch returns the reference's VALUES, rounding included, in every dtype."""
    adjustment = x1.mean(-2, keepdim=True)
    x1 = x1 - adjustment
    x1_norm = x1.pow(2).sum(dim=-1, keepdim=True)
    x1_pad = torch.ones_like(x1_norm)
    shared = same and not x1.requires_grad and not x2.requires_grad
    if shared:
        x2, x2_norm, x2_pad = x1, x1_norm, x1_pad
    else:
        x2 = x2 - adjustment
        x2_norm = x2.pow(2).sum(dim=-1, keepdim=True)
        x2_pad = torch.ones_like(x2_norm)
    res = torch.cat([-2.0 * x1, x1_norm, x1_pad], dim=-1).matmul(torch.cat([x2, x2_pad, x2_norm], dim=-1).transpose(-2, -1))
    if shared:
        res.diagonal(dim1=-2, dim2=-1).fill_(0)
    return res.clamp_min(0)


def _ref_dist(x1, x2, same):
    """Distances as the reference forms them (``kernel.py:52-60``): ``torch.cdist`` clamped at 1e-15 for two inputs, the square root of the
    Gram-trick squared distance clamped at 1e-30 for one."""
    if not same:
        return torch.cdist(x1, x2).clamp_min(1e-15)
    return _gram_sq_dist(x1, x2, True).clamp_min(1e-30).sqrt()


def additive_dense(base_kernel, x1, x2, diag=False, **params):
    """sum_q k'(x1[..., q], x2[..., q]): the reference's arithmetic (``gpytorch/kernels/additive_structure_kernel.py:62-68``: the base kernel under
    ``last_dim_is_batch=True``, summed over the dimension batch) in autograd-visible torch ops, any dtype, any batch shape, any device.  Returns
    [..., n, m] ([..., n] with ``diag``).  RBF / Matern bases (bare or under ScaleKernels) are evaluated here as the reference evaluates them
    (``rbf_kernel.py:68-85``, ``matern_kernel.py:85-110`` through ``Kernel.covar_dist``): inputs divided by the lengthscale of their dimension
    (Matern: centred by the mean of x1 first), every dimension a batch member [..., d, n, 1], the reference's own distance arithmetic
    (``_gram_sq_dist`` / ``_ref_dist``) -- so the values are the reference's to rounding, in float32 as in float64.  Any other base kernel is called
    with ``last_dim_is_batch=True`` and whatever it returns is summed."""
    terms, scales = _dimension_terms(base_kernel, x1, x2, diag=diag, **params)
    res = terms.sum(-2 if diag else -3)
    for sc in scales:                                            # [...]: one outputscale per batch member
        res = res * (sc.unsqueeze(-1) if diag else sc.reshape(*sc.shape, 1, 1))
    return res


def _dimension_terms(base_kernel, x1, x2, diag=False, **params):
    """(terms, scales): the d one-dimensional covariances k'(x1[..., q], x2[..., q]) as the dimension batch [..., d, n, m] ([..., d, n] with
    ``diag``) in the reference's arithmetic (see ``additive_dense``), and the outputscales of the peeled ScaleKernels, NOT yet applied (an empty list
    for a base kernel that is called as a whole: what it returns carries them).  Shared by ``additive_dense`` and ``ng_dense``."""
    base, scales = base_kernel, []
    while type(base) is ScaleKernel:
        scales.append(base.outputscale)
        base = base.base_kernel
    if type(base) in (RBFKernel, MaternKernel) and base.active_dims is None:
        ls = base.lengthscale                                        # [..., 1, 1 or d]
        rbf = base.kind == "rbf"
        if not rbf:
            mean = x1.mean(dim=-2, keepdim=True)
            x1, x2 = x1 - mean, x2 - mean
        t1, t2 = (x1 / ls).transpose(-1, -2).unsqueeze(-1), (x2 / ls).transpose(-1, -2).unsqueeze(-1)   # [..., d, n, 1]
        same = t1.shape == t2.shape and bool(torch.equal(t1, t2))
        if diag:      # covar_dist: zeros for identical inputs, else the norm of the elementwise difference
            r = torch.zeros(*t1.shape[:-1], dtype=t1.dtype, device=t1.device) if same else torch.linalg.norm(t1 - t2, dim=-1)
            sq = None if not rbf else (r if same else r.pow(2))
        elif rbf:
            sq = _gram_sq_dist(t1, t2, same)
        else:
            r = _ref_dist(t1, t2, same)
        if rbf:
            terms = sq.div(-2.0).exp()
        else:
            e = torch.exp(-math.sqrt(base.nu * 2) * r)
            if base.nu == 0.5:
                terms = e
            elif base.nu == 1.5:
                terms = (math.sqrt(3) * r).add(1) * e
            else:
                terms = (math.sqrt(5) * r).add(1).add(5.0 / 3.0 * r ** 2) * e
        return terms, scales
    from .operators import to_dense

    res = base_kernel(x1, x2, diag=diag, last_dim_is_batch=True, **params)
    return (res if diag else to_dense(res)), []


class AdditiveStructureKernel(Kernel):
    r"""k(x, x') = sum_{q<d} k'(x_q, x'_q): first-order additive structure over the input dimensions
    (``gpytorch/kernels/additive_structure_kernel.py:10-74``; constructor arguments, the ``DeprecationWarning``, the ``last_dim_is_batch`` error,
    ``is_stationary``, ``prediction_strategy`` and ``num_outputs_per_input`` are the reference's).  The reference calls the base kernel with
    ``last_dim_is_batch=True`` and sums a d x n x m tensor.

    float32, no batches, 2 <= d <= 8 == ``num_dims``, the base kernel an ``RBFKernel`` or ``MaternKernel`` (one or d lengthscales), bare or inside one
    ``ScaleKernel``: ONE matrix-free operator of the native family ``"add"`` (``additive_native`` has the rule; csrc/kv_directadd.hpp the kernel) --
    d one-dimensional covariances per pair, summed in registers, contracted once.  The operator evaluates the MEAN of the d terms (unit diagonal);
    d times the inner outputscale rides in its outputscale slot, differentiable, and the lengthscale travels expanded to [1, d], so a single
    lengthscale receives the sum of the per-dimension gradients.  Gradients with respect to the inputs are not provided on this path.
    Anything else -- float64, batches, d > 8, other base kernels, inputs that require grad, ``diag=True`` of two different inputs -- is formed
    densely by ``additive_dense``.  d = 1 is the base kernel's own operator.

    Over a ``GridInterpolationKernel`` with ``num_dims == 1`` (additive KISS-GP, 2 <= d <= 16; ``ski_additive_native`` has the rule): ONE
    ``ski.SKIFusedLinearOperator`` on the concatenation of d copies of the grid axis, K = scale W_add blockdiag(T_q) W_add^T, 4 d taps per point
    (csrc/kv_ski_add.hpp)."""

    def __init__(self, base_kernel, num_dims, active_dims=None):
        import warnings

        warnings.warn("AdditiveStructureKernel is deprecated, and will be removed in GPyTorch 2.0. "
                      'Please refer to the "Kernels with Additive or Product Structure" tutorial '
                      "in the GPyTorch docs for how to implement GPs with additive structure.", DeprecationWarning)
        super().__init__(active_dims=active_dims)
        self.base_kernel = base_kernel
        self.num_dims = num_dims

    @property
    def is_stationary(self):
        return self.base_kernel.is_stationary

    dims_as_batch_in_forward = True   # (``last_dim_is_batch`` reaches forward, which refuses it as the reference does)

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        if last_dim_is_batch:
            raise RuntimeError("AdditiveStructureKernel does not accept the last_dim_is_batch argument.")
        d = x1.shape[-1]
        if d == 1:   # one term: the base kernel itself
            return self.base_kernel(x1, x2, diag=diag, **params)
        same = x2 is x1 or (x1.shape == x2.shape and x1.data_ptr() == x2.data_ptr())
        if additive_native(self, x1, x2) and not (diag and not same):
            base, scale = _additive_base(self)
            if diag:   # k(x, x) = d outputscale: no launch
                one = torch.full(x1.shape[:1], float(d), device=x1.device, dtype=x1.dtype)
                return one if scale is None else one * scale.reshape(())
            spec = KernelSpec("add", x1.detach().mean(dim=-2), code=B.add_code(base.kind))
            os_ = torch.full((1,), float(d), device=x1.device, dtype=x1.dtype) if scale is None else float(d) * scale.reshape(1)
            return FusedKernelLinearOperator(x1, x1 if same else x2, spec, base.lengthscale.expand(1, d), os_)
        if not diag and ski_additive_native(self, x1, x2):   # additive KISS-GP: one interpolation onto d one-dimensional axes
            gk, scale = _ski_additive_base(self)
            return gk.additive_operator(x1, x1 if same else x2, scale)
        from .operators import DenseLinearOperator

        res = additive_dense(self.base_kernel, x1, x2, diag=diag, **params)
        return res if diag else DenseLinearOperator(res)

    @property
    def prediction_strategy(self):
        return self.base_kernel.prediction_strategy

    def num_outputs_per_input(self, x1, x2):
        f = getattr(self.base_kernel, "num_outputs_per_input", None)
        return 1 if f is None else f(x1, x2)


def _ps_structure(kernel, x1, x2, last_dim_is_batch, base_types):
    """(base, inner outputscale or None) when the structural conditions the native forms of a ``ProductStructureKernel`` share hold for a base kernel
    of one of ``base_types``, else None: the conditions of ``additive_native``."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return None
    found = _additive_base(kernel)
    if found is None or type(found[0]) not in base_types:
        return None
    base, scale = found
    ls = base.raw_lengthscale
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or ls.dtype != torch.float32 or (scale is not None and scale.dtype != torch.float32):
        return None
    if x1.requires_grad or x2.requires_grad:
        return None
    d = x1.shape[-1]
    if not (d >= 2 and d == kernel.num_dims and x2.shape[-1] == d) or tuple(ls.shape) not in ((1, 1), (1, d)):
        return None
    return base, scale


def ps_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free (native ``"ps"``, tensor-product Matern) form applies to this call of a ``ProductStructureKernel``.  Pure: it looks at the
    kernel's structure and at the shapes and dtypes of the inputs, never at the device.  All of: float32 parameters and inputs; no batch shape on the
    kernel or the inputs; no ``last_dim_is_batch``; 2 <= d <= 8 and d == ``num_dims``; the base kernel exactly a ``MaternKernel``, optionally inside
    one ``ScaleKernel`` with an unbatched outputscale; a lengthscale shaped [1, 1] or [1, d]; inputs without ``requires_grad`` (the native family has
    no input gradients).  Everything else takes another branch of ``ProductStructureKernel.forward`` (``ps_dense`` under plain autograd at the end)."""
    return _ps_structure(kernel, x1, x2, last_dim_is_batch, (MaternKernel,)) is not None and B.ADD_MIN_DIM <= x1.shape[-1] <= B.ADD_MAX_DIM


def _ski_product_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The exact product KISS-GP form (ONE ``ski.SKIFusedLinearOperator`` on the d-dimensional grid axis^d) applies to this call of a
    ``ProductStructureKernel``: the conditions of ``ski_additive_native`` with d in {2, 3} and m^d <= ``backend.SKI_MAX_NODES`` grid nodes."""
    from .ski import _innermost, columns_native

    x2 = x1 if x2 is None else x2
    found = _ski_additive_base(kernel)
    if found is None or last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return False
    gk, scale = found
    if not columns_native(gk.base_kernel):
        return False
    axis = gk.grid[0]
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or axis.dtype != torch.float32 or (scale is not None and scale.dtype != torch.float32):
        return False
    if x1.requires_grad or x2.requires_grad or x1.device.type != "cuda" or x2.device.type != "cuda":
        return False
    d, m = x1.shape[-1], int(axis.numel())
    if not (d in (2, 3) and d == kernel.num_dims and x2.shape[-1] == d and m >= 4 and m ** d <= B.SKI_MAX_NODES):
        return False
    inner = _innermost(gk.base_kernel)
    k = inner.lengthscale.numel()
    if type(inner) is PeriodicKernel:
        return k == 1 and inner.period_length.numel() == 1
    return k in (1, d)


def ps_dense(base_kernel, x1, x2, diag=False, **params):
    """prod_q k'(x1[..., q], x2[..., q]): the reference's arithmetic (``gpytorch/kernels/product_structure_kernel.py:74-75``: the base kernel under
    ``last_dim_is_batch=True``, multiplied over the dimension batch) in autograd-visible torch ops, any dtype, any batch shape, any device.  Returns
    [..., n, m] ([..., n] with ``diag``).  The one-dimensional covariances are the ones ``additive_dense`` sums (``_dimension_terms``); the
    outputscale of a peeled ``ScaleKernel`` scales every one of the d members there, so it is applied once per dimension here: s^d."""
    terms, scales = _dimension_terms(base_kernel, x1, x2, diag=diag, **params)
    d = terms.shape[-2 if diag else -3]
    res = terms.prod(-2 if diag else -3)
    for sc in scales:                                            # [...]: one outputscale per batch member, on each of the d factors
        scd = sc.pow(d)
        res = res * (scd.unsqueeze(-1) if diag else scd.reshape(*scd.shape, 1, 1))
    return res


class ProductStructureKernel(Kernel):
    r"""k(x, x') = prod_{q<d} k'(x_q, x'_q): product structure over the input dimensions (``gpytorch/kernels/product_structure_kernel.py:12-95``;
    constructor arguments, the ``DeprecationWarning``, the ``last_dim_is_batch`` error, ``is_stationary`` and ``num_outputs_per_input`` are the
    reference's; ``prediction_strategy`` follows ``AdditiveStructureKernel``).  The reference calls the base kernel with ``last_dim_is_batch=True``
    and multiplies a d x n x m tensor down.  Unlike the reference's ``__call__`` nothing is evaluated eagerly: rectangular train x test blocks are
    ordinary matrix-free operators here (the reference evaluates the full joint matrix because it cannot root-decompose a rectangle).

    ``forward``, in this order.  d = 1 is the base kernel's own operator.  With a ``MaternKernel`` base this is the tensor-product (separable)
    Matern covariance: float32, no batches, 2 <= d <= 8 == ``num_dims``, one or d lengthscales, bare or inside one ``ScaleKernel`` -- ONE matrix-free
    operator of the native family ``"ps"`` (``ps_native`` has the rule; csrc/kv_directps.hpp the kernel): one exponential per pair whatever d.  The
    inner outputscale s enters as s^d (under ``last_dim_is_batch`` the reference scales every one of the d members), differentiable, in the
    operator's outputscale slot; the lengthscale travels expanded to [1, d], so a single lengthscale receives the sum of the per-dimension
    gradients.  Gradients with respect to the inputs are not provided on this path.  With an ``RBFKernel`` base (the same conditions, any d >= 2)
    the product of d one-dimensional RBFs IS the RBF with per-dimension lengthscales, exp(-sum_q delta_q^2 / (2 l_q^2)): the operator
    ``RBFKernel(ard_num_dims=d)`` returns for these inputs (native family ``"rbf"``), the scale again s^d.  Over a ``GridInterpolationKernel`` with
    ``num_dims == 1`` and d in {2, 3} (m^d grid nodes within ``backend.SKI_MAX_NODES``; otherwise the conditions of ``ski_additive_native``): ONE
    ``ski.SKIFusedLinearOperator`` on d copies of the shared axis -- EXACT, since a product of d one-dimensional cubic interpolations on one axis is
    the d-dimensional interpolation on axis^d and prod_q W_q T_q W_q^T = (kron W_q)(kron T_q)(kron W_q)^T.  SKIP's Lanczos roots and low-rank
    Hadamard tree are not provided: a grid base at d > 3 is formed densely.  Anything else -- float64, batches, d > 8 over Matern, other base
    kernels, inputs that require grad, ``diag=True`` of two different inputs -- is formed densely by ``ps_dense``."""

    def __init__(self, base_kernel, num_dims, active_dims=None):
        import warnings

        warnings.warn("ProductStructureKernel is deprecated, and will be removed in GPyTorch 2.0. "
                      'Please refer to the "Kernels with Additive or Product Structure" tutorial '
                      "in the GPyTorch docs for how to implement GPs with product structure.", DeprecationWarning)
        super().__init__(active_dims=active_dims)
        self.base_kernel = base_kernel
        self.num_dims = num_dims

    @property
    def is_stationary(self):
        return self.base_kernel.is_stationary

    dims_as_batch_in_forward = True   # (``last_dim_is_batch`` reaches forward, which refuses it as the reference does)

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        if last_dim_is_batch:
            raise RuntimeError("ProductStructureKernel does not accept the last_dim_is_batch argument.")
        d = x1.shape[-1]
        if d == 1:   # one factor: the base kernel itself
            return self.base_kernel(x1, x2, diag=diag, **params)
        same = x2 is x1 or (x1.shape == x2.shape and x1.data_ptr() == x2.data_ptr())
        if not (diag and not same):
            native = ps_native(self, x1, x2)
            found = _additive_base(self) if native else _ps_structure(self, x1, x2, False, (RBFKernel,))
            if found is not None:
                base, scale = found
                sd = None if scale is None else scale.reshape(1).pow(d)   # s^d: the outputscale of each of the d factors
                if diag:   # k(x, x) = s^d: no launch
                    one = torch.ones(x1.shape[:1], device=x1.device, dtype=x1.dtype)
                    return one if sd is None else one * sd
                shift = x1.detach().mean(dim=-2)
                spec = KernelSpec("ps", shift, code=B.ps_code(base.kind)) if native else KernelSpec("rbf", shift)
                args = (x1, x1 if same else x2, spec, base.lengthscale.expand(1, d))
                return FusedKernelLinearOperator(*args) if sd is None else FusedKernelLinearOperator(*args, sd)
            if not diag and _ski_product_native(self, x1, x2):   # exact product KISS-GP on axis^d
                return self._grid_operator(x1, x1 if same else x2)
        from .operators import DenseLinearOperator

        res = ps_dense(self.base_kernel, x1, x2, diag=diag, **params)
        return res if diag else DenseLinearOperator(res)

    def _grid_operator(self, x1, x2):
        from . import ski

        gk, scale = _ski_additive_base(self)
        axis = gk._one_axis(x1, x2)
        d = x1.shape[-1]
        columns = ski.additive_columns(gk.base_kernel, axis, d)
        if len(columns) == 1:   # one lengthscale: the one column on every axis
            columns = columns * d
        return ski.SKIFusedLinearOperator(x1, x2, [axis] * d, columns, scale=None if scale is None else scale.reshape(1).pow(d))

    @property
    def prediction_strategy(self):
        return self.base_kernel.prediction_strategy

    def num_outputs_per_input(self, x1, x2):
        f = getattr(self.base_kernel, "num_outputs_per_input", None)
        return 1 if f is None else f(x1, x2)


def ng_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free (native ``"ng"``) form applies to this call of a ``NewtonGirardAdditiveKernel``.  Pure: it looks at the kernel's structure and at
    the shapes and dtypes of the inputs, never at the device.  All of: float32 parameters and inputs; no batch shape on the kernel, its base kernel
    or the inputs; no ``last_dim_is_batch``; 2 <= d <= 8 and d == ``num_dims``; the base kernel EXACTLY an ``RBFKernel`` or a ``MaternKernel``
    (no ``active_dims``); a lengthscale shaped [1, 1] or [1, d]; inputs without ``requires_grad`` (the native family has no input gradients).
    A ``ScaleKernel`` around the base is NOT native: its outputscale s would enter e_n as s^n, which the per-degree outputscales already cover --
    such a model takes the dense branch (``ng_dense`` under plain autograd), like everything else outside the rule."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return False
    base = kernel.base_kernel
    if type(base) not in (RBFKernel, MaternKernel) or len(base.batch_shape) or base.active_dims is not None:
        return False
    ls = base.raw_lengthscale
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or ls.dtype != torch.float32 or kernel.raw_outputscale.dtype != torch.float32:
        return False
    if x1.requires_grad or x2.requires_grad:
        return False
    d = x1.shape[-1]
    if not (B.ADD_MIN_DIM <= d <= B.ADD_MAX_DIM and d == kernel.num_dims and x2.shape[-1] == d):
        return False
    return tuple(ls.shape) in ((1, 1), (1, d))


def ng_dense(base_kernel, x1, x2, outputscale, max_degree, diag=False, **params):
    """sum_{n=1..max_degree} outputscale[..., n - 1] e_n(z_1 .. z_d), z_q = k'(x1[..., q], x2[..., q]), e_n the n-th elementary symmetric polynomial:
    the covariance of ``gpytorch/kernels/newton_girard_additive_kernel.py:70-128`` in autograd-visible torch ops, any dtype, any batch shape, any
    device.  Returns [..., n, m] ([..., n] with ``diag``).  The z_q are the ones ``additive_dense`` sums (the reference's own distance arithmetic for
    RBF / Matern bases; ScaleKernels around the base scale every z_q, so their outputscale enters e_n as s^n, as in the reference).  e_n by the
    one-pass recursion with positive terms only (``backend.ng_esp``) in the INPUT dtype -- the reference's Newton-Girard power sums are an
    alternating sum, and it allocates e_n in float32 whatever the inputs are."""
    terms, scales = _dimension_terms(base_kernel, x1, x2, diag=diag, **params)
    for sc in scales:
        terms = terms * (sc.reshape(*sc.shape, 1, 1) if diag else sc.reshape(*sc.shape, 1, 1, 1))
    e = B.ng_esp(terms.movedim(-2 if diag else -3, -1), max_degree)
    res = None
    for n in range(max_degree):
        w = outputscale[..., n]
        term = (w.unsqueeze(-1) if diag else w.reshape(*w.shape, 1, 1)) * e[n]
        res = term if res is None else res + term
    return res


class NewtonGirardAdditiveKernel(Kernel):
    r"""k(x, x') = sum_{n=1..R} sigma_n e_n(z_1 .. z_d), z_q = k'(x_q, x'_q), R = ``max_degree`` <= d: Duvenaud's additive GP with interactions up to
    order R (https://arxiv.org/abs/1112.4394; ``gpytorch/kernels/newton_girard_additive_kernel.py:14-128`` -- constructor arguments, the silent cap
    of ``max_degree`` at ``num_dims``, ``raw_outputscale`` [*batch_shape, max_degree] under ``Positive()`` initialised to 1 / max_degree, the
    ``outputscale`` property and setter, the ``DeprecationWarning`` and the ``last_dim_is_batch`` error are the reference's).  Give the base kernel
    ``ard_num_dims=d`` for one lengthscale per dimension.  The reference forms a d x n x m tensor, R power sums of it and R + 1 polynomials.

    float32, no batches, 2 <= d <= 8 == ``num_dims``, the base kernel exactly an ``RBFKernel`` or ``MaternKernel`` (one or d lengthscales): ONE
    matrix-free operator of the native family ``"ng"`` (``ng_native`` has the rule; csrc/kv_directng.hpp the kernel) -- d one-dimensional covariances
    per pair, the polynomials by a one-pass recursion in registers, contracted once.  The operator evaluates k / S, S = sum_n sigma_n C(d, n) (unit
    diagonal); S rides in its outputscale slot and sigma in its learnable-parameter slot, both differentiable, and the lengthscale travels expanded
    to [1, d], so a single lengthscale receives the sum of the per-dimension gradients.  Gradients with respect to the inputs are not provided on
    this path.  Anything else -- float64, batches, d > 8, other base kernels, a ``ScaleKernel`` around the base (its outputscale enters e_n as s^n),
    inputs that require grad, ``diag=True`` of two different inputs -- is formed densely by ``ng_dense``."""

    def __init__(self, base_kernel, num_dims, max_degree=None, active_dims=None, **kwargs):
        import warnings

        warnings.warn("NewtonGirardAdditiveKernel is deprecated, and will be removed in GPyTorch 2.0. "
                      'Please refer to the "Kernels with Additive or Product Structure" tutorial '
                      "in the GPyTorch docs for how to implement GPs with additive structure.", DeprecationWarning)
        super().__init__(active_dims=active_dims, **kwargs)
        self.base_kernel = base_kernel
        self.num_dims = num_dims
        self.max_degree = num_dims if (max_degree is None or max_degree > num_dims) else max_degree   # (the cap is silent, as in the reference)
        self.register_parameter("raw_outputscale", torch.nn.Parameter(torch.zeros(*self._batch_shape, self.max_degree)))
        self.register_constraint("raw_outputscale", Positive())
        self.outputscale = [1 / self.max_degree for _ in range(self.max_degree)]

    @property
    def outputscale(self):
        return self._get_transformed("raw_outputscale")

    @outputscale.setter
    def outputscale(self, value):
        self._set_outputscale(value)

    def _set_outputscale(self, value):
        if not torch.is_tensor(value):
            value = torch.as_tensor(value).to(self.raw_outputscale)
        self._set_transformed("raw_outputscale", value)

    @property
    def is_stationary(self):
        return self.base_kernel.is_stationary

    dims_as_batch_in_forward = True   # (``last_dim_is_batch`` reaches forward, which refuses it as the reference does)

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        if last_dim_is_batch:
            raise RuntimeError("NewtonGirardAdditiveKernel does not accept the last_dim_is_batch argument.")
        d = x1.shape[-1]
        sigma = self.outputscale
        same = x2 is x1 or (x1.shape == x2.shape and x1.data_ptr() == x2.data_ptr())
        if ng_native(self, x1, x2) and not (diag and not same):
            base = self.base_kernel
            scale = (sigma * B.ng_binomials(d, self.max_degree, sigma.device, sigma.dtype)).sum()   # S = k(x, x), differentiable in sigma
            if diag:   # k(x, x) = S: no launch
                return torch.ones(x1.shape[0], device=x1.device, dtype=x1.dtype) * scale
            spec = KernelSpec("ng", x1.detach().mean(dim=-2), code=B.add_code(base.kind), param=sigma)
            return FusedKernelLinearOperator(x1, x1 if same else x2, spec, base.lengthscale.expand(1, d), scale.reshape(1))
        from .operators import DenseLinearOperator

        res = ng_dense(self.base_kernel, x1, x2, sigma, self.max_degree, diag=diag, **params)
        return res if diag else DenseLinearOperator(res)


def _gibbs_lengthscales(lengthscale_fn, x1, x2, same):
    """(l1, l2) = lengthscale_fn of the two inputs (ONE call for identical inputs), with the reference's shape check (``gibbs_kernel.py:67-70``)."""
    l1 = lengthscale_fn(x1)
    if l1.shape[-1] != 1:
        raise ValueError(f"lengthscale_fn must return shape (..., k, 1), got (..., k, {l1.shape[-1]})")
    return l1, (l1 if same else lengthscale_fn(x2))


def _gibbs_from_lengthscales(l1, l2, x1, x2, same, diag=False):
    if diag:    # covar_dist: zeros for identical inputs, else the squared norm of the elementwise difference
        dist_sq = torch.zeros(*x1.shape[:-1], dtype=x1.dtype, device=x1.device) if same else torch.linalg.norm(x1 - x2, dim=-1).pow(2)
        S = (l1.pow(2) + l2.pow(2)).squeeze(-1)
        prod = (l1 * l2).squeeze(-1)
    else:
        dist_sq = _gram_sq_dist(x1, x2, same)
        S = l1.pow(2) + l2.pow(2).transpose(-2, -1)
        prod = l1 * l2.transpose(-2, -1)
    ratio = 2.0 * prod / S
    prefactor = ratio.sqrt() if B.GIBBS_PREFACTOR_EXPONENT == 0.5 else ratio.pow(B.GIBBS_PREFACTOR_EXPONENT)
    return prefactor * (-dist_sq / S).exp()


def gibbs_dense(lengthscale_fn, x1, x2, diag=False):
    """sqrt(2 l1 l2 / (l1^2 + l2^2)) exp(-|x1 - x2|^2 / (l1^2 + l2^2)) with l = ``lengthscale_fn(x)``: the reference's arithmetic
    (``gpytorch/kernels/gibbs_kernel.py:64-82``; squared distances as ``Kernel.covar_dist`` forms them, ``_gram_sq_dist``, elementwise for ``diag``)
    in autograd-visible torch ops, any dtype, any batch shape, any device.  x1 [..., n, d], x2 [..., m, d]; returns [..., n, m] ([..., n] with
    ``diag``).  Identical inputs (``torch.equal``) call ``lengthscale_fn`` once and get an exactly zero distance on the diagonal."""
    same = x2 is x1 or (x1.shape == x2.shape and bool(torch.equal(x1, x2)))
    l1, l2 = _gibbs_lengthscales(lengthscale_fn, x1, x2, same)
    return _gibbs_from_lengthscales(l1, l2, x1, x2, same, diag)


def gibbs_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free (native ``"gibbs"``) form applies to this call of a ``GibbsKernel``.  Pure: it looks at the kernel's structure and at the shapes
    and dtypes of the inputs, never at the device.  All of: float32 inputs, and a ``lengthscale_fn`` whose parameters and buffers are all float32
    (it then returns float32 for float32 inputs; ``forward`` checks what it did return); no batch shape on the kernel or the inputs; no
    ``last_dim_is_batch``; 1 <= d <= 6; inputs without ``requires_grad`` (the native family delivers the gradient with respect to the per-point
    lengthscale only).  Everything else takes the dense branch (``gibbs_dense`` under plain autograd)."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return False
    if x1.dtype != torch.float32 or x2.dtype != torch.float32:
        return False
    fn = kernel.lengthscale_fn
    if isinstance(fn, torch.nn.Module) and any(t.dtype != torch.float32 for t in list(fn.parameters()) + list(fn.buffers()) if t.is_floating_point()):
        return False
    if x1.requires_grad or x2.requires_grad:
        return False
    d = x1.shape[-1]
    return 1 <= d <= B.GIBBS_MAX_DIM and x2.shape[-1] == d


class GibbsKernel(Kernel):
    r"""k(x, x') = sqrt(2 l(x) l(x') / (l(x)^2 + l(x')^2)) exp(-|x - x'|^2 / (l(x)^2 + l(x')^2)): the Gibbs covariance with an input-dependent
    lengthscale l = ``lengthscale_fn(x)``, any ``torch.nn.Module`` that maps [..., n, d] to POSITIVE values [..., n, 1]
    (``gpytorch/kernels/gibbs_kernel.py:13-82``; the constructor, the ``ard_num_dims`` error, ``is_stationary`` / ``has_lengthscale``, the
    ``__getitem__`` batch-shape rule and the shape error of ``lengthscale_fn`` are the reference's).  All learnable parameters live in ``lengthscale_fn``.

    The exponent of the prefactor is 1/2 for EVERY d, as the reference executes it (Gibbs / Paciorek-Schervish have d/2;
    ``families.GIBBS_PREFACTOR_EXPONENT``).  For d = 1 the kernel is positive definite.  For d >= 2 with a varying l it is NOT in general (600 uniform
    points in [0, 1]^2: smallest eigenvalue -0.08 for l in [0.1, 0.4], -1.35 for l in [0.05, 0.6], -4e-7 for l in [0.2, 0.25]): solves, log
    determinants and predictions are meaningful for d = 1, or for d >= 2 with a nearly constant l and enough noise.  This library reproduces the
    reference's values; it does not change the formula.

    float32, no batches, 1 <= d <= 6, inputs that do not require grad: ONE matrix-free operator of the native family ``"gibbs"`` (``gibbs_native`` has
    the rule; csrc/kv_directgibbs.hpp the kernel) where the reference forms about six n x m tensors.  Its points are the augmented clouds
    z = [x.detach() | l]: every row of the prepared cloud carries its own lengthscale, and the derivative pass (csrc/kv_grad_gibbs.hpp) returns the
    gradient with respect to l for every point, which autograd carries into ``lengthscale_fn``.  A ``ScaleKernel`` around it works as around any
    native kernel.  Coordinates are centred, not scaled: the float32 error grows like eps max|x - mean| / min l.  A non-positive or non-finite l gives
    NaN, as in the reference.  Anything else -- float64, batches, d > 6, inputs that require grad, ``diag=True`` of two different inputs -- is formed
    densely by ``gibbs_dense``."""

    is_stationary = False
    has_lengthscale = False

    def __init__(self, lengthscale_fn, **kwargs):
        if kwargs.get("ard_num_dims") is not None:
            raise NotImplementedError("GibbsKernel does not support ARD.")
        super().__init__(**kwargs)
        self.lengthscale_fn = lengthscale_fn

    def __getitem__(self, index):
        """``gibbs_kernel.py:56-62``: the kernel has no batch-shaped parameters, so only the batch shape is indexed."""
        if len(self.batch_shape) == 0:
            return self
        import copy

        new = copy.deepcopy(self)
        index = index if isinstance(index, tuple) else (index,)
        new._batch_shape = torch.empty(self.batch_shape)[index].shape
        return new

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        same = x2 is x1 or (x1.shape == x2.shape and (x1.data_ptr() == x2.data_ptr() or bool(torch.equal(x1, x2))))
        l1, l2 = _gibbs_lengthscales(self.lengthscale_fn, x1, x2, same)
        native = (gibbs_native(self, x1, x2, last_dim_is_batch) and l1.dtype == torch.float32 and l2.dtype == torch.float32
                  and l1.shape == (x1.shape[0], 1) and l2.shape == (x2.shape[0], 1))
        if native and not (diag and not same):
            if diag:   # k(x, x) = 1: no launch
                return torch.ones(x1.shape[0], device=x1.device, dtype=x1.dtype)
            z1 = torch.cat([x1.detach(), l1], dim=-1)
            z2 = z1 if same else torch.cat([x2.detach(), l2], dim=-1)
            shift = torch.cat([x1.detach().mean(dim=-2), x1.new_zeros(1)])   # the coordinates are centred; the l column is not shifted
            ones = torch.ones(1, 1, device=x1.device, dtype=x1.dtype)        # the lengthscale slot: ones, not read, no gradient
            return FusedKernelLinearOperator(z1, z2, KernelSpec("gibbs", shift), ones)
        from .operators import DenseLinearOperator

        res = _gibbs_from_lengthscales(l1, l2, x1, x2, same, diag)
        return res if diag else DenseLinearOperator(res)


def hamming_dense(x1, x2, vocab_size, alpha, beta, diag=False):
    """((1 + alpha) / (alpha + dist))^beta with dist = T - sum_{t, v} x1[.., t, v] x2[.., t, v]: the reference's arithmetic
    (``gpytorch/kernels/hamming_kernel.py:130-160``) in autograd-visible torch ops, any dtype, any batch shape, any device -- but the distance by ONE
    GEMM on the flattened inputs where ``hamming_dist`` broadcasts an n x m x T x V tensor (the sum over (t, v) IS the inner product of the flattened
    rows).  x1 [..., n, T V], x2 [..., m, T V]; returns [..., n, m] ([..., n] with ``diag``).  As the reference executes it: a width that is no
    multiple of ``vocab_size`` is a RuntimeError; identical inputs (``torch.equal``) get an exactly zero distance on the diagonal unless an input
    requires grad, and k0 = ((1 + alpha) / alpha)^beta expanded to [..., n] with ``diag``; distances are clamped at zero, except the elementwise ones
    of ``diag`` on two different inputs; alpha and beta [*batch, 1] broadcast against the distances as they are."""
    if x1.shape[-1] % vocab_size or x2.shape[-1] % vocab_size:
        raise RuntimeError(f"shape '[..., -1, {vocab_size}]' is invalid for an input of width {x1.shape[-1]}: the width must be a multiple of vocab_size")
    t = x1.shape[-1] // vocab_size
    same = x2 is x1 or (x1.shape == x2.shape and bool(torch.equal(x1, x2)))
    if diag:
        if same:
            res = ((1 + alpha) / alpha).pow(beta)
            return res.expand(*([-1] * (res.dim() - 1)), x1.shape[-2])
        dist = t - (x1 * x2).sum(-1)
    else:
        dist = t - x1 @ x2.transpose(-1, -2)
        if same and not x1.requires_grad and not x2.requires_grad:
            dist.diagonal(dim1=-2, dim2=-1).fill_(0)
        dist = dist.clamp_min(0)
    return ((1 + alpha) / (alpha + dist)).pow(beta)


def hamming_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free (native ``"hamming"``) form applies to this call of a ``HammingIMQKernel``.  Pure: it looks at the kernel's structure and at
    the shapes and dtypes of the inputs, never at their values or the device.  All of: float32 inputs and parameters; no batch shape on the kernel or
    the inputs; no ``last_dim_is_batch``; a width that is a multiple of ``vocab_size`` with T <= 128 positions and V <= 126 letters; inputs without
    ``requires_grad`` (packed tokens have no gradient).  ``forward`` asks one thing more, which needs the values: that both clouds are exactly
    one-hot.  Everything else takes the dense branch (``hamming_dense`` under plain autograd)."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or len(kernel.batch_shape) or x1.dim() != 2 or x2.dim() != 2:
        return False
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or kernel.raw_alpha.dtype != torch.float32 or kernel.raw_beta.dtype != torch.float32:
        return False
    if x1.requires_grad or x2.requires_grad:
        return False
    v, width = int(kernel.vocab_size), x1.shape[-1]
    if not 1 <= v <= B.HAMMING_MAX_VOCAB or width == 0 or width % v or x2.shape[-1] != width:
        return False
    return width // v <= B.HAMMING_MAX_POSITIONS


_HAMMING_ONE_HOT: dict = {}   # per source tensor (keyed as backend._ORDER_CACHE is, plus a weak reference): is it exactly one-hot


def _hamming_one_hot(x, vocab_size: int) -> bool:
    """Every position of every row of x has one entry equal to 1 and the others 0 (``backend.hamming_prep``'s validity flag): ONE host read per cloud,
    cached while the tensor lives unmodified."""
    import weakref

    key = (x.data_ptr(), x._version, tuple(x.shape), str(x.device), x.dtype, int(vocab_size))
    hit = _HAMMING_ONE_HOT.get(key)
    if hit is None or hit[0]() is not x:
        while len(_HAMMING_ONE_HOT) >= 8:   # a handful of clouds (train / test inputs of a few models), oldest first out
            _HAMMING_ONE_HOT.pop(next(iter(_HAMMING_ONE_HOT)))
        hit = _HAMMING_ONE_HOT[key] = (weakref.ref(x), bool(B.hamming_prep(x, vocab_size)[1]))
    return hit[1]


class HammingIMQKernel(Kernel):
    r"""k(x, x') = ((1 + alpha) / (alpha + d_Hamming(x, x')))^beta: the inverse-multiquadric Hamming kernel over fixed-length sequences, one-hot
    encoded and flattened to T V columns (``gpytorch/kernels/hamming_kernel.py:14-160``, http://arxiv.org/abs/2304.03775; constructor arguments,
    ``raw_alpha`` / ``raw_beta`` of shape [*batch_shape, 1] under ``Positive()``, the properties, setters and priors, and what ``forward`` returns for
    every combination of ``diag`` and equal inputs are the reference's; ``active_dims`` -- the sequence columns of inputs that carry other covariates
    too -- is an addition).  The reference's ``hamming_dist`` broadcasts an n x m x T x V tensor.

    float32, no batches, T <= 128, V <= 126, inputs that do not require grad and ARE one-hot (one host read of a validity flag per cloud): ONE
    matrix-free operator of the native family ``"hamming"`` (``hamming_native`` has the rule; csrc/kv_directham.hpp the kernel) on sequences stored as
    one byte per position -- a prepared cloud is n T bytes, nothing n x m is formed.  The operator evaluates k~ = (1 + c / alpha)^(-beta) with a
    unit diagonal; k0 = ((1 + alpha) / alpha)^beta rides in its outputscale slot and theta = [alpha, beta] in its learnable-parameter slot, both
    differentiable.  A ``ScaleKernel`` around it works as around any native kernel.  Anything else -- float64, batches, longer sequences, larger
    vocabularies, inputs that are not one-hot or require grad, ``diag=True`` of two different inputs -- is formed densely by ``hamming_dense``: one
    GEMM on the flattened inputs, differentiable in alpha, beta and x."""

    def __init__(self, vocab_size, batch_shape=torch.Size([]), alpha_prior=None, alpha_constraint=None, beta_prior=None, beta_constraint=None,
                 active_dims=None):
        super().__init__(batch_shape=batch_shape, active_dims=active_dims)
        self.vocab_size = vocab_size
        for name, prior, constraint in (("alpha", alpha_prior, alpha_constraint), ("beta", beta_prior, beta_constraint)):
            self.register_parameter(f"raw_{name}", torch.nn.Parameter(torch.zeros(*self._batch_shape, 1)))
            if prior is not None:
                self.register_prior(f"{name}_prior", prior, AttrGetter(name), AttrSetter(f"_set_{name}"))
            self.register_constraint(f"raw_{name}", Positive() if constraint is None else constraint)

    @property
    def alpha(self):
        return self._get_transformed("raw_alpha")

    @alpha.setter
    def alpha(self, value):
        self._set_alpha(value)

    def _set_alpha(self, value):
        self._set_transformed("raw_alpha", value)

    @property
    def beta(self):
        return self._get_transformed("raw_beta")

    @beta.setter
    def beta(self, value):
        self._set_beta(value)

    def _set_beta(self, value):
        self._set_transformed("raw_beta", value)

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        v = self.vocab_size
        alpha, beta = self.alpha, self.beta
        same = x2 is x1 or (x1.shape == x2.shape and x1.data_ptr() == x2.data_ptr())
        if (not (diag and not same) and hamming_native(self, x1, x2, last_dim_is_batch)
                and _hamming_one_hot(x1, v) and (same or _hamming_one_hot(x2, v))):
            k0 = ((1 + alpha) / alpha).pow(beta).reshape(1)   # k(x, x), differentiable in alpha and beta
            if diag:   # no launch
                return k0.expand(x1.shape[0])
            ones = torch.ones(1, 1, device=x1.device, dtype=x1.dtype)   # the lengthscale slot: ones, not read, no gradient
            spec = KernelSpec("hamming", None, code=int(v), param=torch.cat([alpha.reshape(1), beta.reshape(1)]))
            return FusedKernelLinearOperator(x1, x1 if same else x2, spec, ones, k0)
        from .operators import DenseLinearOperator

        res = hamming_dense(x1, x2, v, alpha, beta, diag=diag)
        return res if diag else DenseLinearOperator(res)


def ski_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The matrix-free form (``ski.SKIFusedLinearOperator``) applies to this call of a ``GridInterpolationKernel``.  All of: float32 inputs and grid;
    inputs on the device, without ``requires_grad``; no batch shape on the inputs; no ``last_dim_is_batch``; 1..3 input dimensions; every grid
    axis has at least 4 nodes (fewer is a ``ValueError``: the rule indexes outside the grid) and the grid at most 2^24 nodes in all; a base kernel
    whose Toeplitz columns come from a differentiable dense expression (RBF, Matern, RQ, PiecewisePolynomial, Periodic, bare or under
    ``ScaleKernel``s, without batch shape or ``active_dims`` of their own).  Everything else -- float64, batches, d > 3, gradients with respect to
    the inputs, host tensors -- takes the dense branch (``ski.ski_dense`` under plain autograd).  (A ``GridInterpolationKernel`` called directly
    with inputs that require grad asks ``ski_input_grad_native`` instead.)"""
    x2 = x1 if x2 is None else x2
    return _ski_native_shape(kernel, x1, x2, last_dim_is_batch) and not (x1.requires_grad or x2.requires_grad)


def ski_input_grad_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """``ski_native``'s rule, except that either input may require grad: the matrix-free operator then carries the graph-attached inputs and hands
    them their gradients through the derivative-stencil kernel (``ski.input_grads``; csrc/kv_ski.hpp) -- deep kernel learning over KISS-GP.  What
    ``GridInterpolationKernel.forward`` asks while grad mode is on.  The additive and the product compositions keep ``ski_additive_native`` /
    ``ps_native``: their inputs get gradients on the dense branch."""
    return _ski_native_shape(kernel, x1, x1 if x2 is None else x2, last_dim_is_batch)


def _ski_native_shape(kernel, x1, x2, last_dim_is_batch) -> bool:
    """Everything of ``ski_native`` but ``requires_grad``."""
    from .ski import columns_native

    sizes = [int(g.numel()) for g in kernel.grid]
    if any(m < 4 for m in sizes):
        raise ValueError(f"GridInterpolationKernel needs at least 4 grid points per dimension (got {sizes})")
    if last_dim_is_batch or x1.dim() > 2 or x2.dim() > 2:
        return False
    if x1.dtype != torch.float32 or x2.dtype != torch.float32 or any(g.dtype != torch.float32 for g in kernel.grid):
        return False
    if x1.device.type != "cuda" or x2.device.type != "cuda":
        return False
    d = 1 if x1.dim() == 1 else x1.shape[-1]
    if not (1 <= d <= B.SKI_MAX_DIM and d == len(sizes) and math.prod(sizes) <= B.SKI_MAX_NODES):
        return False
    return columns_native(kernel.base_kernel)


class GridInterpolationKernel(Kernel):
    r"""KISS-GP / structured kernel interpolation (``gpytorch/kernels/grid_interpolation_kernel.py:16-213`` over ``grid_kernel.py``):
    k(x1, x2) ~= w_x1^T K_UU w_x2 with cubic interpolation weights onto a regular grid and K_UU a Kronecker product of per-axis Toeplitz matrices
    of the stationary ``base_kernel``.  Constructor arguments, the buffers ``grid_0 ..`` and ``has_initialized_grid``, ``update_grid``, the dynamic
    grid (``_tight_grid_bounds``, the 2.01-spacing padding of ``forward``) and the out-of-bounds error are the reference's.

    float32 on the device, d <= 3, no batches: ONE matrix-free operator (``ski_native`` has the rule; csrc/kv_ski.hpp the kernels) whose
    interpolation matrix is never stored.  Anything else is formed densely by ``ski.ski_dense``.  Inputs that require grad (a feature extractor in
    front: deep kernel learning) keep the matrix-free operator while grad mode is on (``ski_input_grad_native``) and receive the gradients of
    products and of the marginal log likelihood; the dense branches are differentiable in the inputs through ``ski.interp_axis``.  The gradient
    of a PREDICTION with respect to the inputs is not provided: an eval-mode call returns the numbers of detached inputs.  Every ARD lengthscale of the base kernel sits on
    its own grid axis: the operator converges to ``base_kernel(x1, x2)`` as the grid refines.  ``last_dim_is_batch`` with ``num_dims == 1`` (the
    ``AdditiveStructureKernel`` composition) returns the dimension batch densely (``dimension_batch``); the additive kernel itself takes the
    matrix-free form ``additive_operator`` where ``ski_additive_native`` holds.  The ``ProductStructureKernel`` composition is ONE exact operator on axis^d at d = 2, 3 and dense above.  Not
    provided: SKIP proper (Lanczos roots and the low-rank Hadamard tree for d > 3) and fantasy updates (WISKI)."""

    dims_as_batch_in_forward = True   # (``last_dim_is_batch`` reaches forward: the dimension batch over ONE grid axis)

    def __init__(self, base_kernel, grid_size, num_dims=None, grid_bounds=None, active_dims=None):
        has_initialized_grid = 0
        grid_is_dynamic = True
        if grid_bounds is None:
            if num_dims is None:
                raise RuntimeError("num_dims must be supplied if grid_bounds is None")
            grid_bounds = tuple((-1.0, 1.0) for _ in range(num_dims))      # temporary: the first call replaces them
        else:
            has_initialized_grid = 1
            grid_is_dynamic = False
            if num_dims is None:
                num_dims = len(grid_bounds)
            elif num_dims != len(grid_bounds):
                raise RuntimeError("num_dims ({}) disagrees with the number of supplied grid_bounds ({})".format(num_dims, len(grid_bounds)))
        grid_sizes = [grid_size for _ in range(num_dims)] if isinstance(grid_size, int) else list(grid_size)
        if len(grid_sizes) != num_dims:
            raise RuntimeError("The number of grid sizes provided through grid_size do not match num_dims.")
        if any(m < 4 for m in grid_sizes):
            raise ValueError(f"GridInterpolationKernel needs at least 4 grid points per dimension (got {grid_sizes})")
        super().__init__(active_dims=active_dims)
        from .utils.grid import create_grid

        self.base_kernel = base_kernel
        self.grid_is_dynamic = grid_is_dynamic
        self.num_dims = num_dims
        self.grid_sizes = grid_sizes
        self.grid_bounds = grid_bounds
        for i, g in enumerate(create_grid(grid_sizes, grid_bounds)):
            self.register_buffer(f"grid_{i}", g)
        self.register_buffer("has_initialized_grid", torch.tensor(has_initialized_grid, dtype=torch.bool))
        self._spec = None

    @property
    def grid(self):
        return [getattr(self, f"grid_{i}") for i in range(self.num_dims)]

    @property
    def is_stationary(self):
        return self.base_kernel.is_stationary

    def update_grid(self, grid):
        """Supply a new grid (``grid_kernel.py:84-101``)."""
        if torch.is_tensor(grid):
            grid = [grid[:, i] for i in range(grid.size(-1))]
        if len(grid) != self.num_dims:
            raise RuntimeError("New grid should have the same number of dimensions as before.")
        for i in range(self.num_dims):
            setattr(self, f"grid_{i}", grid[i])
        self._spec = None
        return self

    @property
    def _tight_grid_bounds(self):
        spacings = tuple((bound[1] - bound[0]) / self.grid_sizes[i] for i, bound in enumerate(self.grid_bounds))
        return tuple((bound[0] + 2.01 * spacing, bound[1] - 2.01 * spacing) for bound, spacing in zip(self.grid_bounds, spacings))

    def grid_spec(self):
        """The host description of the grid the interpolation rule works from (cached until the grid changes)."""
        grid = self.grid
        key = tuple((g.data_ptr(), g._version, g.dtype, str(g.device)) for g in grid)
        if self._spec is None or self._spec[0] != key:
            self._spec = (key, B.SkiGridSpec(grid))
        return self._spec[1]

    def _maybe_update_grid(self, x1, x2):
        """``grid_interpolation_kernel.py:150-181``: a dynamic grid is rebuilt when it was never initialised or the data leave its tight bounds."""
        from .utils.grid import create_grid

        same = x1 is x2 or (x1.shape == x2.shape and torch.equal(x1, x2))
        x = x1.reshape(-1, self.num_dims) if same else torch.cat([x1.reshape(-1, self.num_dims), x2.reshape(-1, self.num_dims)])
        x_maxs, x_mins = x.max(0)[0].tolist(), x.min(0)[0].tolist()
        update = (not self.has_initialized_grid.item()) or any(
            x_min < bound[0] or x_max > bound[1] for x_min, x_max, bound in zip(x_mins, x_maxs, self._tight_grid_bounds))
        if update:
            spacings = tuple((x_max - x_min) / (gs - 4.02) for gs, x_min, x_max in zip(self.grid_sizes, x_mins, x_maxs))
            self.grid_bounds = tuple((x_min - 2.01 * sp, x_max + 2.01 * sp) for x_min, x_max, sp in zip(x_mins, x_maxs, spacings))
            self.update_grid(create_grid(self.grid_sizes, self.grid_bounds, dtype=self.grid[0].dtype, device=self.grid[0].device))
            self.has_initialized_grid.fill_(True)

    def forward(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        from . import ski
        from .operators import DenseLinearOperator

        if last_dim_is_batch:
            return self.dimension_batch(x1, x2, diag=diag)
        if x1.shape[-1] != self.num_dims:
            raise RuntimeError(f"GridInterpolationKernel: expected inputs with {self.num_dims} dimensions, got {x1.shape[-1]}")
        if self.grid_is_dynamic:
            self._maybe_update_grid(x1, x2)
        grid = self.grid
        native = ski_input_grad_native(self, x1, x2) if torch.is_grad_enabled() else ski_native(self, x1, x2)
        spec = self.grid_spec()
        ski.check_bounds(x1, spec)
        if x2 is not x1:
            ski.check_bounds(x2, spec)
        columns = ski.toeplitz_columns(self.base_kernel, grid)
        if diag:
            if not (x1 is x2 or (x1.shape == x2.shape and torch.equal(x1, x2))):
                return ski.ski_dense(x1, x2, grid, columns).diagonal(dim1=-2, dim2=-1)
            return ski.ski_dense(x1, x1, grid, columns, diag=True)
        if native:
            return ski.SKIFusedLinearOperator(x1, x2, grid, columns, spec=spec)
        cols = [c.to(x1.dtype) for c in columns]
        return DenseLinearOperator(ski.ski_dense(x1, x2, [g.to(x1.dtype) if g.dtype != x1.dtype else g for g in grid], cols))

    def _one_axis(self, x1, x2):
        """What both forms of the dimension batch start with: the ONE grid axis every input column is interpolated onto
        (``grid_interpolation_kernel.py:132-143``), after the dynamic grid was fitted to ALL columns pooled (``x.reshape(-1, self.num_dims)``,
        ``:150-181``) and every coordinate checked against its bounds."""
        from . import ski

        if self.num_dims != 1:   # (the reference's ``assert num_dim == len(x_grid)`` in ``Interpolation.interpolate``)
            raise AssertionError(f"GridInterpolationKernel: last_dim_is_batch interpolates single input columns and needs num_dims == 1 (got {self.num_dims})")
        if self.grid_is_dynamic:
            self._maybe_update_grid(x1, x2)
        spec = self.grid_spec()
        ski.check_bounds(x1.reshape(-1, 1), spec)
        if x2 is not x1:
            ski.check_bounds(x2.reshape(-1, 1), spec)
        return self.grid[0]

    def dimension_batch(self, x1, x2, diag=False):
        """``forward(last_dim_is_batch=True)``: the d one-dimensional interpolated covariances as a dimension batch, a tensor [..., d, n, m]
        ([..., d, n] with ``diag``), by ``ski.ski_dense`` per input column -- the dense branch: any dtype, the CPU, batches."""
        from . import ski

        axis = self._one_axis(x1, x2)
        d = x1.shape[-1]
        same = x1 is x2 or (x1.shape == x2.shape and torch.equal(x1, x2))
        columns = [c.to(x1.dtype) for c in ski.additive_columns(self.base_kernel, axis, d)]
        grid = [axis.to(x1.dtype) if axis.dtype != x1.dtype else axis]
        terms = []
        for q in range(d):
            c1 = x1[..., q: q + 1]
            c2 = c1 if same else x2[..., q: q + 1]
            col = [columns[q if len(columns) > 1 else 0]]
            if diag and not same:
                terms.append(ski.ski_dense(c1, c2, grid, col).diagonal(dim1=-2, dim2=-1))
            else:
                terms.append(ski.ski_dense(c1, c2, grid, col, diag=diag))
        return torch.stack(terms, dim=-2 if diag else -3)

    def additive_operator(self, x1, x2, scale=None):
        """The additive composition over this kernel (``num_dims == 1``) as ONE matrix-free operator on the concatenation of d copies of the grid
        axis (``ski_additive_native`` has the rule; csrc/kv_ski_add.hpp the kernels).  ``scale``: the outer outputscale or None."""
        from . import ski

        axis = self._one_axis(x1, x2)
        d = x1.shape[-1]
        key = (axis.data_ptr(), axis._version, d)
        if getattr(self, "_add_spec", None) is None or self._add_spec[0] != key:
            self._add_spec = (key, B.SkiGridSpec([axis] * d, additive=True))
        columns = ski.additive_columns(self.base_kernel, axis, d)
        return ski.SKIFusedLinearOperator(x1, x2, [axis] * d, columns, scale=None if scale is None else scale.reshape(1), spec=self._add_spec[1])

    @property
    def prediction_strategy(self):
        from .ski import interpolated_prediction_strategy

        return interpolated_prediction_strategy


__all__ = ["Kernel", "RBFKernel", "MaternKernel", "RQKernel", "PiecewisePolynomialKernel", "PeriodicKernel", "ScaleKernel", "AdditiveKernel", "ProductKernel",
           "SpectralMixtureKernel", "product_factors", "sm_dense", "sm_native", "RBFKernelGrad", "rbfgrad_native", "Matern52KernelGrad", "matern52grad_native", "RBFKernelGradGrad", "rbfgradgrad_native", "GridInterpolationKernel", "ski_native", "ski_input_grad_native", "ski_additive_native",
           "AdditiveStructureKernel", "additive_native", "additive_dense", "NewtonGirardAdditiveKernel", "ng_native", "ng_dense",
           "ProductStructureKernel", "ps_native", "ps_dense",
           "GibbsKernel", "gibbs_native", "gibbs_dense", "HammingIMQKernel", "hamming_native", "hamming_dense"]
_ = (math, Interval)
